// bg_td_plan.h -- host-only part of the TD(lambda) learner's step: which kernels a step of a given size runs, with which grids, and
// the scale of the lazily scaled traces.  Plain C++ (no HIP), like bg_schedule.h: bg_learner_host.h issues the launches a TdPlan names,
// tests/test_td_plan_cpu.py holds it against an independent restatement without a GPU, tests/test_sanitizers_cpu.py runs it under
// AddressSanitizer + UBSan (tests/sanitize/td_plan_driver.cpp).  The kernels themselves: bg_learner.h, bg_fit.h, bg_eval.h.
//
// This is the ONE place where the learner's thresholds, their defaults and their BGAMD_TD_* / BGAMD_FIT_* variables live.
#pragma once
#include <cstdlib>

namespace bg {

// ---- the constants the plan shares with the kernels (defined here only; bg_eval.h, bg_learner.h and bg_fit.h include this header) ----
constexpr int ROOT3_THREADS = 512;       // threads of a workgroup of the LDS-staged bf16 x 3 root pass (bg_eval.h): a wave per 32-row tile
constexpr int TD_LD = 25664;             // trace row stride in floats (multiple of 64)
#ifndef BG_TD_CHUNK
#define BG_TD_CHUNK 8
#endif
constexpr int TD_CHUNK = BG_TD_CHUNK;    // games staged in LDS at a time by the trace kernel
#ifndef BG_TD_MAX_GROUPS
#define BG_TD_MAX_GROUPS 256
#endif
constexpr int TD_MAX_GROUPS = BG_TD_MAX_GROUPS;
#ifndef BG_TD_MIN_NG
#define BG_TD_MIN_NG 4
#endif
constexpr int TD_FUSED_GAMES = 16;       // slots per workgroup of td_forward_mfma_kernel
constexpr int TD_DELAY_SLICE = 128;                                              // parameters (internal order) per workgroup and slice: 4 cache lines
constexpr int TD_DELAY_SLICES = (TD_LD + TD_DELAY_SLICE - 1) / TD_DELAY_SLICE;   // 201 (the last one reads 64 floats past a row: the next row, or the zeroed tail)
constexpr int FIT_TILE = 32;                 // rows per tile = the M of the forward product, the K of the gradient product
constexpr long long FIT_CHUNK_ROWS = 65536;  // 256 workgroups x 8 tiles

// ---- tuning: every threshold and switch of the step's dispatch, read once at bgamd_td_create ----
// (all long long so that one table can name them; the switches are 0 / 1)
struct TdTuning {
    long long mfma_min = 24576;            // running games from which the forward pass uses the LDS-staged matrix-pipe kernel (BGAMD_TD_MFMA_MIN;
                                           //   measured equal to the direct one from there up, slower below: 153 vs 132 ms per round at 3 072 slots)
    long long fused = 1;                   // ... with its epilogue in the same launch (BGAMD_TD_FUSED=0: two launches)
    long long direct_min = 512;            // ... from which it runs as one workgroup per 32-row tile, weights from the L2 (BGAMD_TD_DIRECT_MIN)
    long long nt_min = 8192;               // ... from which the whole-row trace pass uses nontemporal loads / stores (BGAMD_TD_NT_MIN)
    long long wide_min = 8192;             // running games from which the trace pass uses the whole-row workgroups (BGAMD_TD_WIDE_MIN)
    long long pipe = 1;                    // mid-sized steps: the software-pipelined whole-row pass (BGAMD_TD_PIPE=0: td_trace_wide_kernel)
    long long fuse_step = 1;               // ... with the forward pass of the same slots in the same launch (BGAMD_TD_FUSE_STEP=0: two launches)
    long long fuse_min = 512;              // ... from this many running slots (measured: 512 slots 27 vs 31 us per step, 256 slots 28 vs 26) up to 16 per CU (BGAMD_TD_FUSE_MIN)
    long long fuse_g = 0;                  // ... slots per workgroup of that launch: 0 = by step size (BGAMD_TD_FUSE_G = 1, 2, 4, 8, 16)
    long long slice_ng = 0;                // BGAMD_TD_NG: games per group of the slice kernel at mid-sized steps (0: as many groups as allowed)
    long long no_wide_even = 0;            // BGAMD_TD_NO_WIDE_EVEN=1: mid-sized steps never take the whole-row kernels
    long long lazy = 1;                    // lazily scaled traces (bg_learner.h); BGAMD_TD_LAZY=0: e <- λ e + ∇ every step
    long long dense = 0;                   // BGAMD_TD_DENSE=1: every column active from the first step (the dense pass)
    // the supervised step (bgamd_td_fit_step, bg_fit.h)
    long long fit_chunk = FIT_CHUNK_ROWS;  // rows per kernel pair (BGAMD_FIT_CHUNK, a multiple of 32)
    long long fit_groups = TD_MAX_GROUPS;  // most workgroups of a launch (BGAMD_FIT_GROUPS, 1 .. 256: tests reach several tiles per workgroup with few rows)
};

// how a variable's text becomes its field's value
enum class TdRule {
    NUMBER,          // set: atoll of it
    SWITCH,          // set: on unless atoi of it is 0 (so =0 turns a default-on switch off, =1 a default-off one on)
    ON_IF_SET,       // a switch that is on when the variable is set at all, whatever it says
    FUSE_G,          // 1, 2, 4, 8 or 16; anything else: 0 (by step size)
    FIT_CHUNK,       // clamped to [FIT_TILE, 2^22], rounded up to a multiple of FIT_TILE
    FIT_GROUPS,      // clamped to [1, TD_MAX_GROUPS]
};
constexpr struct { const char *var; long long TdTuning::*field; TdRule rule; bool experimental_only; } TD_TUNING_VARS[] = {
    {"BGAMD_TD_MFMA_MIN", &TdTuning::mfma_min, TdRule::NUMBER, false},
    {"BGAMD_TD_FUSED", &TdTuning::fused, TdRule::SWITCH, true},            // (the unfused matrix-pipe forward: experimental build only)
    {"BGAMD_TD_DIRECT_MIN", &TdTuning::direct_min, TdRule::NUMBER, false},
    {"BGAMD_TD_NT_MIN", &TdTuning::nt_min, TdRule::NUMBER, false},
    {"BGAMD_TD_WIDE_MIN", &TdTuning::wide_min, TdRule::NUMBER, false},
    {"BGAMD_TD_PIPE", &TdTuning::pipe, TdRule::SWITCH, false},
    {"BGAMD_TD_FUSE_STEP", &TdTuning::fuse_step, TdRule::SWITCH, false},
    {"BGAMD_TD_FUSE_MIN", &TdTuning::fuse_min, TdRule::NUMBER, false},
    {"BGAMD_TD_FUSE_G", &TdTuning::fuse_g, TdRule::FUSE_G, false},
    {"BGAMD_TD_NG", &TdTuning::slice_ng, TdRule::NUMBER, false},
    {"BGAMD_TD_NO_WIDE_EVEN", &TdTuning::no_wide_even, TdRule::SWITCH, false},
    {"BGAMD_TD_LAZY", &TdTuning::lazy, TdRule::SWITCH, false},
    {"BGAMD_TD_DENSE", &TdTuning::dense, TdRule::ON_IF_SET, false},
    {"BGAMD_FIT_CHUNK", &TdTuning::fit_chunk, TdRule::FIT_CHUNK, false},
    {"BGAMD_FIT_GROUPS", &TdTuning::fit_groups, TdRule::FIT_GROUPS, false},
};

// The defaults above, overridden by the variables that are set.  get: name -> text or nullptr (getenv, or a test's own).
template <class GetEnv>
inline TdTuning td_tuning_from_env(GetEnv get, bool experimental)
{
    TdTuning u;
    for (const auto &d : TD_TUNING_VARS) {
        const char *s = get(d.var);
        if (!s || (d.experimental_only && !experimental)) continue;
        long long &x = u.*d.field;
        switch (d.rule) {
            case TdRule::NUMBER: x = atoll(s); break;
            case TdRule::SWITCH: x = atoi(s) != 0; break;
            case TdRule::ON_IF_SET: x = 1; break;
            case TdRule::FUSE_G: { const int g = atoi(s); x = (g == 1 || g == 2 || g == 4 || g == 8 || g == 16) ? g : 0; break; }
            case TdRule::FIT_CHUNK: {
                long long c = atoll(s);
                c = c < FIT_TILE ? FIT_TILE : (c > (1ll << 22) ? (1ll << 22) : c);
                x = (c + FIT_TILE - 1) / FIT_TILE * FIT_TILE;
                break;
            }
            case TdRule::FIT_GROUPS: { const int g = atoi(s); x = g < 1 ? 1 : (g > TD_MAX_GROUPS ? TD_MAX_GROUPS : g); break; }
        }
    }
    return u;
}

// ---- the scale of the stored traces (bg_learner.h), one step of it ----
// t = 0 writes ∇ at c = 1; afterwards c <- λ c, folded back in by an ordinary pass when it leaves [2^-40, 2^40] (λ > 1 is the
// caller's business, but it must not overflow either).  scale: c, the same for every game of the replay, kept by the caller.
struct TdScale {
    float emul, ginv, cmul;              // the trace kernels' arguments: ê <- emul ê + ginv ∇, the sums take cmul ê
    int full;                            // an ordinary pass: every active column is written
};
inline TdScale td_scale_step(long long t, float lambda, bool lazy, double &scale)
{
    TdScale r{lambda, 1.0f, 1.0f, 1};
    if (t == 0) scale = 1.0;
    else {
        const double c = (double)lambda * scale;
        if (lazy && c >= 0x1p-40 && c <= 0x1p40) { scale = c; r = TdScale{1.0f, (float)(1.0 / c), (float)c, 0}; }
        else { r.emul = (float)c; scale = 1.0; }
    }
    return r;
}

// ---- the fused launch ----
// Mid-sized steps whose trace pass takes the pipelined whole-row kernel: forward pass and trace pass in ONE launch (bg_learner.h).
// -> slots per workgroup: the smallest of 1, 2, 4, 8, 16 that asks for no more workgroups than CUs (BGAMD_TD_FUSE_G pins it), or 0
// when a step of n_active slots does not take that launch.
// (BGAMD_TD_FUSED=0 / BGAMD_TD_DIRECT_MIN choose the forward kernel: a step that is to run the unfused or the VALU forward pass cannot
//  take the launch that contains the fused one)
inline int td_fuse_g(const TdTuning &u, int n_cu, long long n_active)
{
    const long long groups_max = n_cu < TD_MAX_GROUPS ? n_cu : TD_MAX_GROUPS;
    int g = u.fuse_g > 0 ? (int)u.fuse_g : 1;
    if (u.fuse_g <= 0) while (g < 16 && (n_active + g - 1) / g > groups_max) g *= 2;
    const bool ok = u.fuse_step && u.pipe && u.fused && n_active >= u.direct_min && !u.no_wide_even && n_active >= u.fuse_min &&
                    n_active < u.mfma_min && n_active < u.nt_min && (n_active + g - 1) / g <= groups_max;
    return ok ? g : 0;
}
// The delayed replay's one-launch step exists for the steps that take the fused launch with at least TD_DELAY_SLICES workgroups: a streamed
// replay through a constant number k of slots in that range (512 ... 4 096 on 256 CUs).  -> its slots per workgroup, or 0: replay exactly.
inline int td_delay_g(const TdTuning &u, int n_cu, long long k)
{
    const int g = k > 0 ? td_fuse_g(u, n_cu, k) : 0;
    return g > 0 && (k + g - 1) / g >= TD_DELAY_SLICES ? g : 0;
}

// ---- the plan of one step ----
enum class TdForward {
    NONE,            // inside the fused launch
    MATRIX_PIPE,     // traj_hidden_bf16x3_kernel, then td_epilogue_wave_kernel
    MFMA_FUSED,      // td_forward_mfma_kernel: the product and its epilogue in one launch
    DIRECT,          // traj_hidden_direct_kernel, then td_epilogue_wave_kernel (experimental build: only BGAMD_TD_FUSED=0 leads here)
    VALU2, VALU4,    // td_forward_kernel<2>, <4>
};
enum class TdTrace {
    SLICE,           // td_trace_kernel: slices x groups of ng games
    WIDE,            // td_trace_wide_kernel<false, false>
    WIDE_NT,         // td_trace_wide_kernel<FIRST, true>: nontemporal -- and what step 0 of a whole-row step without the pipelined pass runs, nt or not
    PIPE,            // td_trace_pipe_kernel
    FUSED,           // td_step_fused_kernel<FIRST, fuse_g>
};
struct TdPlan {
    TdForward forward;
    long long forward_grid;              // workgroups of the forward launch (MATRIX_PIPE, DIRECT: of the product; the epilogue has a wave per slot)
    TdTrace trace;
    bool first;                          // step 0: the FIRST instance of the trace kernel
    int fuse_g;                          // FUSED: slots per workgroup (else 0)
    int n_groups;                        // workgroups of the trace launch (SLICE: x TD_SLICES) = partial-sum rows the reduce kernel reads
    long long ng;                        // SLICE: games per group
    int full;                            // the kernel's `full` argument: the scale step's, and 1 at step 0
};

// full: TdScale::full of the same step
inline TdPlan td_plan(const TdTuning &u, int n_cu, long long t, long long n_active, int full = 1)
{
    TdPlan p{};
    p.first = t == 0;
    p.full = p.first ? 1 : full;
    p.fuse_g = td_fuse_g(u, n_cu, n_active);
    if (p.fuse_g) {
        p.forward = TdForward::NONE;
    } else if (n_active >= u.mfma_min) {
        // the [2 G x 198] · [198 x 128] product of the step on the matrix pipe (exact bf16 x 3 split of fc1.weight, fp32
        // accumulation: the env's root pass), then the epilogue per game
        p.forward = TdForward::MATRIX_PIPE;
        const long long n_rows = 2 * n_active;
        p.forward_grid = ((n_rows + 31) / 32 + ROOT3_THREADS / 64 - 1) / (ROOT3_THREADS / 64);
        if (p.forward_grid > n_cu) p.forward_grid = n_cu;
    } else if (n_active >= u.direct_min && u.fused) {
        // mid-sized steps: the product and its epilogue in one launch (bg_learner.h)
        p.forward = TdForward::MFMA_FUSED;
        p.forward_grid = (n_active + TD_FUSED_GAMES - 1) / TD_FUSED_GAMES;
    } else if (n_active >= u.direct_min) {
        // mid-sized steps: the same product, a workgroup per 32-row tile and the weight planes straight from the L2 (bg_eval.h)
        p.forward = TdForward::DIRECT;
        p.forward_grid = (2 * n_active + 31) / 32;
    } else if (n_active <= 8192) {
        p.forward = TdForward::VALU2;
        p.forward_grid = (n_active + 1) / 2;
    } else {
        p.forward = TdForward::VALU4;
        p.forward_grid = (n_active + 3) / 4;
    }
    // games per group: >= BG_TD_MIN_NG, and at most TD_MAX_GROUPS groups
    p.ng = (n_active + TD_MAX_GROUPS - 1) / TD_MAX_GROUPS;
    if (p.ng < BG_TD_MIN_NG) p.ng = BG_TD_MIN_NG;
    if (u.slice_ng > 0 && n_active >= 512 && n_active < u.wide_min) {           // mid-sized steps on the slice kernel: fewer, larger groups
        p.ng = u.slice_ng;                                                       //   (fewer partial rows for the reduce kernel to read)
        if ((n_active + p.ng - 1) / p.ng > TD_MAX_GROUPS) p.ng = (n_active + TD_MAX_GROUPS - 1) / TD_MAX_GROUPS;
    }
    p.n_groups = (int)((n_active + p.ng - 1) / p.ng);
    p.trace = TdTrace::SLICE;
    // whole-row workgroups take chunks of TD_CHUNK games: below wide_min they pay only when the chunks divide evenly over the CUs
    // (a streamed replay through 2 048 or 4 096 slots: 143 vs 147 and 110 vs 118 ms per 65 536-game round)
    const long long per_wave_of_blocks = (long long)n_cu * TD_CHUNK;
    const bool wide_even = !u.no_wide_even && n_active >= per_wave_of_blocks && u.wide_min > per_wave_of_blocks &&
                           n_active * 20 >= ((n_active + per_wave_of_blocks - 1) / per_wave_of_blocks) * per_wave_of_blocks * 19;
    if (n_active >= u.wide_min || wide_even || p.fuse_g) {
        // large rounds: a workgroup per whole trace row and strided chunks of games (bg_learner.h)
        p.n_groups = (int)((n_active + TD_CHUNK - 1) / TD_CHUNK);
        if (p.n_groups > n_cu) p.n_groups = n_cu;
        if (p.n_groups > TD_MAX_GROUPS) p.n_groups = TD_MAX_GROUPS;
        const bool nt = n_active >= u.nt_min;
        if (p.fuse_g) {
            p.trace = TdTrace::FUSED;
            p.n_groups = (int)((n_active + p.fuse_g - 1) / p.fuse_g);
        } else if (u.pipe && !nt && n_active <= (long long)n_cu * TD_CHUNK * 4) {
            p.trace = TdTrace::PIPE;     // mid-sized steps (at most a few chunks per CU): the software-pipelined whole-row pass (bg_learner.h)
        } else {
            p.trace = p.first || nt ? TdTrace::WIDE_NT : TdTrace::WIDE;
        }
    }
    return p;
}

}  // namespace bg
