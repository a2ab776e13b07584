// Driver for the learner's host-only step plan (csrc/bg_td_plan.h), built by tests/test_td_plan_cpu.py (plain) and by
// tests/test_sanitizers_cpu.py (g++ -fsanitize=address,undefined).  The tuning comes from the environment through the header's own
// parser, as in bgamd_td_create.
//   td_plan_driver tuning <experimental>            every field of the tuning, one "name value" line each
//   td_plan_driver plan <experimental> <n_cu>       "t n_active" pairs on stdin -> one line per plan:
//                                                   n_cu t n_active | forward forward_grid | trace n_groups ng | first fuse_g full
//   td_plan_driver delay <experimental> <n_cu>      slot counts on stdin -> "k g": slots per workgroup of the delayed replay's step, or 0
//   td_plan_driver scale <lambda> <steps>           the trace scale over steps 0 .. steps - 1: emul ginv cmul as float32 bit patterns, full, c
// The kernels are named the way bgamd_td_step's two switches launch them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "bg_td_plan.h"

static std::string forward_name(const bg::TdPlan &p)
{
    switch (p.forward) {
        case bg::TdForward::NONE: return "none";
        case bg::TdForward::MATRIX_PIPE: return "traj_hidden_bf16x3_kernel+td_epilogue_wave_kernel";
        case bg::TdForward::MFMA_FUSED: return "td_forward_mfma_kernel";
        case bg::TdForward::DIRECT: return "traj_hidden_direct_kernel+td_epilogue_wave_kernel";
        case bg::TdForward::VALU2: return "td_forward_kernel<2>";
        case bg::TdForward::VALU4: return "td_forward_kernel<4>";
    }
    return "?";
}

static std::string trace_name(const bg::TdPlan &p)
{
    const std::string first = p.first ? "true" : "false";
    switch (p.trace) {
        case bg::TdTrace::SLICE: return "td_trace_kernel<" + first + ">";
        case bg::TdTrace::WIDE: return "td_trace_wide_kernel<false,false>";
        case bg::TdTrace::WIDE_NT: return "td_trace_wide_kernel<" + first + ",true>";
        case bg::TdTrace::PIPE: return "td_trace_pipe_kernel<" + first + ">";
        case bg::TdTrace::FUSED: return "td_step_fused_kernel<" + first + "," + std::to_string(p.fuse_g) + ">";
    }
    return "?";
}

static unsigned bits(float f)
{
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    if (mode == "scale") {
        if (argc != 4) return 2;
        const bg::TdTuning u = bg::td_tuning_from_env(getenv, false);
        const float lambda = strtof(argv[2], nullptr);
        double scale = 123.0;                                  // (step 0 sets it)
        for (long long t = 0, n = atoll(argv[3]); t < n; ++t) {
            const bg::TdScale s = bg::td_scale_step(t, lambda, u.lazy != 0, scale);
            std::printf("%lld %08x %08x %08x %d %a\n", t, bits(s.emul), bits(s.ginv), bits(s.cmul), s.full, scale);
        }
        return 0;
    }
    const bg::TdTuning u = bg::td_tuning_from_env(getenv, atoi(argv[2]) != 0);
    if (mode == "tuning") {
        std::printf("mfma_min %lld\nfused %lld\ndirect_min %lld\nnt_min %lld\nwide_min %lld\npipe %lld\nfuse_step %lld\nfuse_min %lld\n"
                    "fuse_g %lld\nslice_ng %lld\nno_wide_even %lld\nlazy %lld\ndense %lld\nfit_chunk %lld\nfit_groups %lld\n",
                    u.mfma_min, u.fused, u.direct_min, u.nt_min, u.wide_min, u.pipe, u.fuse_step, u.fuse_min, u.fuse_g, u.slice_ng,
                    u.no_wide_even, u.lazy, u.dense, u.fit_chunk, u.fit_groups);
        return 0;
    }
    if (argc != 4) return 2;
    const int n_cu = atoi(argv[3]);
    long long t = 0, n = 0;
    if (mode == "plan") {
        // `full` of a later step whose scale stays in range: 0 with lazily scaled traces, 1 without
        while (std::scanf("%lld %lld", &t, &n) == 2) {
            const bg::TdPlan p = bg::td_plan(u, n_cu, t, n, u.lazy ? 0 : 1);
            std::printf("%d %lld %lld | %s %lld | %s %d %lld | %d %d %d\n", n_cu, t, n, forward_name(p).c_str(), p.forward_grid,
                        trace_name(p).c_str(), p.n_groups, p.ng, p.first ? 1 : 0, p.fuse_g, p.full);
        }
        return 0;
    }
    if (mode == "delay") {
        while (std::scanf("%lld", &n) == 1) std::printf("%lld %d\n", n, bg::td_delay_g(u, n_cu, n));
        return 0;
    }
    return 2;
}
