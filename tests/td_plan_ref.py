"""An independent restatement of the learner's step dispatch, for tests/test_td_plan_cpu.py to hold csrc/bg_td_plan.h against.

Transcribed from the host code of commit 3f1f4b1 ("Fit the value net to rollout targets: a supervised learner step"), the parent of
the change that introduced bg_td_plan.h -- from bgamd_td_create (the getenv lines), bgamd_td_step (the if / else-if chain of its
launches), td_fuse_g_for, td_replay_delayed / bgamd_td_replay (the delayed route) in csrc/bgamd.hip as they stood there (that host code is csrc/bg_learner_host.h now) -- and NOT from
the new header: it follows that function's order of statements, one Python line per C line, so that the two are two derivations."""
import re

import numpy as np

# the constants of csrc/bg_learner.h, bg_eval.h, bg_fit.h at that commit
TD_CHUNK = 8
TD_MAX_GROUPS = 256
TD_FUSED_GAMES = 16
TD_LD = 25664
TD_DELAY_SLICES = (TD_LD + 127) // 128
ROOT3_THREADS = 512
BG_TD_MIN_NG = 4
FIT_TILE = 32
FIT_CHUNK_ROWS = 65536


def _atoi(s):
    """C's atoi / atoll on text that fits: blanks, a sign, digits; anything else ends the number, none at all is 0"""
    m = re.match(r"[ \t\n\v\f\r]*([+-]?[0-9]+)", s)
    return int(m.group(1)) if m else 0


def tuning(env, experimental):
    """bgamd_td_create: env is a dict of the variables that are set -> the members of bgamd_td they decide"""
    u = dict(mfma_min=24576, fused=1, direct_min=512, nt_min=8192, wide_min=8192, pipe=1, fuse_step=1, fuse_min=512, fuse_g=0, slice_ng=0,
             no_wide_even=0, lazy=1, dense=0, fit_chunk=FIT_CHUNK_ROWS, fit_groups=TD_MAX_GROUPS)
    get = env.get
    if get("BGAMD_FIT_CHUNK") is not None:
        c = _atoi(get("BGAMD_FIT_CHUNK"))
        c = FIT_TILE if c < FIT_TILE else ((1 << 22) if c > (1 << 22) else c)
        u["fit_chunk"] = (c + FIT_TILE - 1) // FIT_TILE * FIT_TILE
    if get("BGAMD_FIT_GROUPS") is not None:
        g = _atoi(get("BGAMD_FIT_GROUPS"))
        u["fit_groups"] = 1 if g < 1 else (TD_MAX_GROUPS if g > TD_MAX_GROUPS else g)
    u["mfma_min"] = _atoi(get("BGAMD_TD_MFMA_MIN")) if get("BGAMD_TD_MFMA_MIN") is not None else 24576
    u["dense"] = 1 if get("BGAMD_TD_DENSE") is not None else 0
    if get("BGAMD_TD_WIDE_MIN") is not None:
        u["wide_min"] = _atoi(get("BGAMD_TD_WIDE_MIN"))
    if get("BGAMD_TD_NT_MIN") is not None:
        u["nt_min"] = _atoi(get("BGAMD_TD_NT_MIN"))
    u["pipe"] = int(not (get("BGAMD_TD_PIPE") is not None and _atoi(get("BGAMD_TD_PIPE")) == 0))
    if get("BGAMD_TD_NG") is not None:
        u["slice_ng"] = _atoi(get("BGAMD_TD_NG"))
    u["fuse_step"] = int(not (get("BGAMD_TD_FUSE_STEP") is not None and _atoi(get("BGAMD_TD_FUSE_STEP")) == 0))
    if get("BGAMD_TD_FUSE_MIN") is not None:
        u["fuse_min"] = _atoi(get("BGAMD_TD_FUSE_MIN"))
    if get("BGAMD_TD_FUSE_G") is not None:
        g = _atoi(get("BGAMD_TD_FUSE_G"))
        u["fuse_g"] = g if g in (1, 2, 4, 8, 16) else 0
    u["no_wide_even"] = int(get("BGAMD_TD_NO_WIDE_EVEN") is not None and _atoi(get("BGAMD_TD_NO_WIDE_EVEN")) != 0)
    if experimental:
        u["fused"] = int(not (get("BGAMD_TD_FUSED") is not None and _atoi(get("BGAMD_TD_FUSED")) == 0))
    if get("BGAMD_TD_DIRECT_MIN") is not None:
        u["direct_min"] = _atoi(get("BGAMD_TD_DIRECT_MIN"))
    u["lazy"] = int(not (get("BGAMD_TD_LAZY") is not None and _atoi(get("BGAMD_TD_LAZY")) == 0))
    return u


def scale_step(t, lam, lazy, scale):
    """the scale lines of bgamd_td_step: -> (emul, ginv, cmul as float32, full, the new scale); lam is a float32"""
    emul, ginv, cmul, full = np.float32(lam), np.float32(1.0), np.float32(1.0), 1
    if t == 0:
        scale = 1.0
    else:
        c = float(np.float32(lam)) * scale
        if lazy and 2.0 ** -40 <= c <= 2.0 ** 40:
            scale, emul, ginv, cmul, full = c, np.float32(1.0), np.float32(1.0 / c), np.float32(c), 0
        else:
            emul, scale = np.float32(c), 1.0
    return emul, ginv, cmul, full, scale


def fuse_g_for(u, n_cu, n_active):
    """td_fuse_g_for: slots per workgroup of the fused launch, 0: the step does not take it"""
    fuse_groups_max = n_cu if n_cu < TD_MAX_GROUPS else TD_MAX_GROUPS
    fuse_g = u["fuse_g"] if u["fuse_g"] > 0 else 1
    if u["fuse_g"] <= 0:
        while fuse_g < 16 and (n_active + fuse_g - 1) // fuse_g > fuse_groups_max:
            fuse_g *= 2
    ok = (u["fuse_step"] and u["pipe"] and u["fused"] and n_active >= u["direct_min"] and not u["no_wide_even"] and
          n_active >= u["fuse_min"] and n_active < u["mfma_min"] and n_active < u["nt_min"] and
          (n_active + fuse_g - 1) // fuse_g <= fuse_groups_max)
    return fuse_g if ok else 0


def delay_g(u, n_cu, k):
    """bgamd_td_replay's choice of the delayed route for a replay through a constant k slots: its slots per workgroup, or 0"""
    g = fuse_g_for(u, n_cu, k) if k > 0 else 0
    return g if g > 0 and (k + g - 1) // g >= TD_DELAY_SLICES else 0


def plan(u, n_cu, t, n_active, experimental):
    """bgamd_td_step for n_active > 0 -> (forward kernels, forward grid, trace kernel instance, n_groups, ng, first, fuse_g, full): the
    launches it issues.  `full` is the kernel's last argument for a later step whose scale stays in range (c = 0.7 from 1)."""
    full = scale_step(t, np.float32(0.7), u["lazy"], 1.0)[3]
    # the inline copy of td_fuse_g_for
    fuse_groups_max = n_cu if n_cu < TD_MAX_GROUPS else TD_MAX_GROUPS
    fuse_g = u["fuse_g"] if u["fuse_g"] > 0 else 1
    if u["fuse_g"] <= 0:
        while fuse_g < 16 and (n_active + fuse_g - 1) // fuse_g > fuse_groups_max:
            fuse_g *= 2
    fused_step = bool(u["fuse_step"] and u["pipe"] and u["fused"] and n_active >= u["direct_min"] and not u["no_wide_even"] and
                      n_active >= u["fuse_min"] and n_active < u["mfma_min"] and n_active < u["nt_min"] and
                      (n_active + fuse_g - 1) // fuse_g <= fuse_groups_max)
    if fused_step:
        forward, fgrid = "none", 0
    elif n_active >= u["mfma_min"]:
        n_rows = 2 * n_active
        blocks = ((n_rows + 31) // 32 + ROOT3_THREADS // 64 - 1) // (ROOT3_THREADS // 64)
        if blocks > n_cu:
            blocks = n_cu
        forward, fgrid = "traj_hidden_bf16x3_kernel+td_epilogue_wave_kernel", blocks
    elif n_active >= u["direct_min"] and u["fused"]:
        forward, fgrid = "td_forward_mfma_kernel", (n_active + TD_FUSED_GAMES - 1) // TD_FUSED_GAMES
    elif experimental and n_active >= u["direct_min"]:
        forward, fgrid = "traj_hidden_direct_kernel+td_epilogue_wave_kernel", (2 * n_active + 31) // 32
    elif n_active <= 8192:
        forward, fgrid = "td_forward_kernel<2>", (n_active + 1) // 2
    else:
        forward, fgrid = "td_forward_kernel<4>", (n_active + 3) // 4
    ng = (n_active + TD_MAX_GROUPS - 1) // TD_MAX_GROUPS
    if ng < BG_TD_MIN_NG:
        ng = BG_TD_MIN_NG
    if u["slice_ng"] > 0 and n_active >= 512 and n_active < u["wide_min"]:
        ng = u["slice_ng"]
        if (n_active + ng - 1) // ng > TD_MAX_GROUPS:
            ng = (n_active + TD_MAX_GROUPS - 1) // TD_MAX_GROUPS
    n_groups = (n_active + ng - 1) // ng
    per_wave_of_blocks = n_cu * TD_CHUNK
    wide_even = (not u["no_wide_even"] and n_active >= per_wave_of_blocks and u["wide_min"] > per_wave_of_blocks and
                 n_active * 20 >= ((n_active + per_wave_of_blocks - 1) // per_wave_of_blocks) * per_wave_of_blocks * 19)
    first = "true" if t == 0 else "false"
    if n_active >= u["wide_min"] or wide_even or fused_step:
        n_groups = (n_active + TD_CHUNK - 1) // TD_CHUNK
        if n_groups > n_cu:
            n_groups = n_cu
        if n_groups > TD_MAX_GROUPS:
            n_groups = TD_MAX_GROUPS
        nt = n_active >= u["nt_min"]
        if fused_step:
            n_groups = (n_active + fuse_g - 1) // fuse_g
            trace = "td_step_fused_kernel<%s,%d>" % (first, fuse_g)
        elif u["pipe"] and not nt and n_active <= n_cu * TD_CHUNK * 4:
            trace = "td_trace_pipe_kernel<%s>" % first
        elif t == 0:
            trace = "td_trace_wide_kernel<true,true>"
        elif nt:
            trace = "td_trace_wide_kernel<false,true>"
        else:
            trace = "td_trace_wide_kernel<false,false>"
    else:
        trace = "td_trace_kernel<%s>" % first
    return forward, fgrid, trace, n_groups, ng, int(t == 0), fuse_g if fused_step else 0, 1 if t == 0 else full
