"""The kernel routes of bgamd_td_step that the learner's tests reach, as plain data (no torch, no GPU): the BGAMD_TD_* settings of every
route and the kernels the step plan (csrc/bg_td_plan.h) must name under them.  tests/test_gpu_learner_steps.py runs every route on the
device; tests/test_td_plan_cpu.py checks, without one, that a route's setting does reach the kernels named here at those tests' sizes."""

# Kernel routes: the BGAMD_TD_* variables bgamd_td_create reads, and the kernels bgamd_td_step's dispatch then selects for steps of
# 157 ... 1 running games (lock-step) or 7 slots (streamed) -- far below every default threshold (direct_min = fuse_min = 512,
# wide_min = nt_min = 8192, mfma_min = 24576).  Step 0 runs the <true> (FIRST) instance of the trace kernel named.
ROUTES = {
    # n < direct_min: td_forward_kernel<2>; n < wide_min: td_trace_kernel
    "valu": {},
    # n >= direct_min: td_forward_mfma_kernel; FUSE_STEP=0 keeps the step out of the fused launch; n < wide_min: td_trace_kernel
    "direct_slice": {"BGAMD_TD_DIRECT_MIN": "1", "BGAMD_TD_FUSE_STEP": "0"},
    # n >= mfma_min: traj_hidden_bf16x3_kernel + td_epilogue_wave_kernel (and never the fused launch); td_trace_kernel
    "matrix_pipe": {"BGAMD_TD_MFMA_MIN": "1"},
    # td_forward_mfma_kernel; n >= wide_min, pipe, n < nt_min: td_trace_pipe_kernel
    "direct_pipe": {"BGAMD_TD_DIRECT_MIN": "1", "BGAMD_TD_FUSE_STEP": "0", "BGAMD_TD_WIDE_MIN": "1"},
    # ... PIPE=0: td_trace_wide_kernel<., false> (step 0: <true, true>)
    "direct_wide": {"BGAMD_TD_DIRECT_MIN": "1", "BGAMD_TD_FUSE_STEP": "0", "BGAMD_TD_WIDE_MIN": "1", "BGAMD_TD_PIPE": "0"},
    # ... n >= nt_min: td_trace_wide_kernel<false, true>, the nontemporal instance
    "direct_wide_nt": {"BGAMD_TD_DIRECT_MIN": "1", "BGAMD_TD_FUSE_STEP": "0", "BGAMD_TD_WIDE_MIN": "1", "BGAMD_TD_PIPE": "0",
                       "BGAMD_TD_NT_MIN": "1"},
    # n >= direct_min, n >= fuse_min, ceil(n / G) <= CUs: td_step_fused_kernel<., 1>, one slot per workgroup
    "fused_g1": {"BGAMD_TD_DIRECT_MIN": "1", "BGAMD_TD_FUSE_MIN": "1", "BGAMD_TD_FUSE_G": "1"},
    # ... td_step_fused_kernel<., 16>: 16 slots per workgroup, the last workgroup partly filled
    "fused_g16": {"BGAMD_TD_DIRECT_MIN": "1", "BGAMD_TD_FUSE_MIN": "1", "BGAMD_TD_FUSE_G": "16"},
    # the valu route with e <- λ e + ∇ at every step (emul = λ, every pass an ordinary one)
    "ordinary": {"BGAMD_TD_LAZY": "0"},
}
_VARS = ("BGAMD_TD_DIRECT_MIN", "BGAMD_TD_FUSE_STEP", "BGAMD_TD_MFMA_MIN", "BGAMD_TD_WIDE_MIN", "BGAMD_TD_PIPE", "BGAMD_TD_NT_MIN",
         "BGAMD_TD_FUSE_MIN", "BGAMD_TD_FUSE_G", "BGAMD_TD_LAZY", "BGAMD_TD_DENSE", "BGAMD_TD_NG", "BGAMD_TD_NO_WIDE_EVEN", "BGAMD_TD_FUSED")

# What the comments above say, as the plan's own words: route -> (forward route, trace route at step 0, trace route at every later step,
# slots per workgroup of the fused launch, lazily scaled traces).  On 256 CUs, for every step of 1 ... 157 running games.  A trace route
# is the kernel with its template arguments: step 0 takes the FIRST = true instance of the same kernel -- for td_trace_wide_kernel that is
# <true, true>, nontemporal or not.
EXPECTED = {
    "valu":           ("td_forward_kernel<2>", "td_trace_kernel<true>", "td_trace_kernel<false>", 0, True),
    "direct_slice":   ("td_forward_mfma_kernel", "td_trace_kernel<true>", "td_trace_kernel<false>", 0, True),
    "matrix_pipe":    ("traj_hidden_bf16x3_kernel+td_epilogue_wave_kernel", "td_trace_kernel<true>", "td_trace_kernel<false>", 0, True),
    "direct_pipe":    ("td_forward_mfma_kernel", "td_trace_pipe_kernel<true>", "td_trace_pipe_kernel<false>", 0, True),
    "direct_wide":    ("td_forward_mfma_kernel", "td_trace_wide_kernel<true,true>", "td_trace_wide_kernel<false,false>", 0, True),
    "direct_wide_nt": ("td_forward_mfma_kernel", "td_trace_wide_kernel<true,true>", "td_trace_wide_kernel<false,true>", 0, True),
    "fused_g1":       ("none", "td_step_fused_kernel<true,1>", "td_step_fused_kernel<false,1>", 1, True),
    "fused_g16":      ("none", "td_step_fused_kernel<true,16>", "td_step_fused_kernel<false,16>", 16, True),
    "ordinary":       ("td_forward_kernel<2>", "td_trace_kernel<true>", "td_trace_kernel<false>", 0, False),
}
