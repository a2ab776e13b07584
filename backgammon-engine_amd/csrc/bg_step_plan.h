// bg_step_plan.h -- host-only part of the env's greedy step: which kernels a run of steps on an env of a given size launches, with
// which grids, and how its rows are laid out.  Plain C++ (no HIP), like bg_td_plan.h and bg_schedule.h: bgamd.hip issues the launches
// a StepPlan names, tests/test_step_plan_cpu.py holds it against an independent restatement without a GPU and runs it under
// AddressSanitizer + UBSan (tests/sanitize/step_plan_driver.cpp).  The kernels themselves: bg_staged_kernels.h, bg_eval.h,
// bg_root_resident.h, bg_sample.h, bg_random_kernels.h.
//
// This is the ONE place where the step's thresholds, their defaults and their BGAMD_* variables live.
#pragma once
#include <cstdlib>
#include "../../include/bgamd.h"         // the precisions (BGAMD_F32 ...)
#include "bg_td_plan.h"                  // ROOT3_THREADS

namespace bg {

// ---- the constants the plan shares with the kernels (defined here only; bg_staged.h and bg_eval.h include this header) ----
// lane-per-game kernels of the step boundary: threads per workgroup (measured 64 .. 1 024: 256 and 512 tie, smaller is
// slower -- every workgroup pays two allocation atomics in the roots)
#ifndef BG_LANE_NT
#define BG_LANE_NT 256
#endif
constexpr int LANE_NT = BG_LANE_NT;
// expand_kernel / doubles_kernel, threads per workgroup: every block iteration costs one same-address allocation atomic, so the leaf
// stage (2 000 block iterations of 256) takes big workgroups; the doubles plies are small and latency-bound and take smaller ones
#ifndef BG_EXPAND_NT_PLY
#define BG_EXPAND_NT_PLY 512
#endif
#ifndef BG_EXPAND_NT_LEAF
#define BG_EXPAND_NT_LEAF 1024
#endif
constexpr int EXPAND_NT_PLY = BG_EXPAND_NT_PLY, EXPAND_NT_LEAF = BG_EXPAND_NT_LEAF;
#ifndef BG_XALL_NT
#define BG_XALL_NT 512
#endif
constexpr int XALL_NT = BG_XALL_NT;      // threads of a workgroup of expand_all_kernel
#ifdef BG_XALL_WG_PER_CU                 // (the round-5 co-residency experiment: fewer, so that one fits beside a value-net workgroup)
constexpr int XALL_WG_PER_CU = BG_XALL_WG_PER_CU;
#else
constexpr int XALL_WG_PER_CU = 1024 / XALL_NT;           // 16 waves of expand_all_kernel per CU
#endif
constexpr int LIST_SHARDS = 4;           // parts of the roots' node lists (StagedView::shards)
constexpr int N_ARENAS = 4;              // row arenas of the incremental value net (StagedView::b_base)
#ifndef BG_DELTA_THREADS
#define BG_DELTA_THREADS 1024
#endif
constexpr int DELTA_THREADS = BG_DELTA_THREADS;         // 16 waves per CU, one workgroup per CU (LDS: W1^T + the lists).  -DBG_DELTA_THREADS=512/768: the round-5
                                                        // co-residency experiment (2 / 3 waves per SIMD at 128 VGPRs: room for another kernel's workgroup on the CU)
constexpr int EVAL_THREADS = 768;        // 12 waves per CU (3 per SIMD): block-sparse tiles leave the MFMA pipe ~50 % busy, more waves fill it
constexpr int ROOTR_THREADS = 256;       // root_hidden_resident_kernel
constexpr int BROOT_THREADS = 256;       // = LANE_NT of the boundary launch: four waves
// games per workgroup of the boundary launch with the root pass inside (bg_root_resident.h)
#ifndef BG_BROOT_GPW
#define BG_BROOT_GPW 128
#endif
constexpr int BROOT_GPW = BG_BROOT_GPW;
constexpr int D16_THREADS = 256;         // eval_rows_d16_kernel: 4 waves, one per 32-unit column tile
#ifndef BG_D16_WAVES
#define BG_D16_WAVES 3                   // waves per SIMD the register allocation aims at (= workgroups per CU)
#endif
constexpr int SRCH_NT = 256;             // the search's, the sampled step's and the analysis' row kernels

// What a step is expected to produce, per game: the grids are sized by it (more than the estimate only means more iterations per workgroup)
constexpr long long EST_ROWS = 24;       // afterstate rows: a greedy step averages ~18 rows per game
constexpr long long EST_DBL_NODES = 4;   // ply-1 nodes of the doubles turns (a sixth of the lanes x <= 15)
constexpr long long EST_LEAF_PARENTS = 16;   // leaf parents

// ---- tuning: every switch of the step's dispatch, read once at env_create ----
// (all int so that one table can name them; the switches are 0 / 1).  The default build reads no variable: there ten of the twelve
// never leave their default, root_in_boundary goes by the env's size and overlap is off.
constexpr long long ROOT_IN_BOUNDARY_MIN = 24576;
struct StepTuning {
    int mfma_delta = 0;                  // BGAMD_MFMA_DELTA=1: eval_rows_mdelta_kernel instead of eval_rows_delta_kernel.  Round 3's K-compacted MFMA delta kernel
                                         //   (bg_eval_mfma.h) is correct and canonical but measured 10 % slower than the VALU kernel on the same box (NOTEBOOK.md)
    int d16 = 0;                         // BGAMD_F16X2_RESIDENT=1: eval_rows_d16_kernel (W1 resident in registers) for BGAMD_F16X2 -- measured 6 % slower than round 1's eval_rows_f16x2_kernel
    int list_shards = 1;                 // the roots' node lists in LIST_SHARDS parts (BGAMD_LIST_SHARDS=0: one list each)
    int split_arena = 1;                 // the greedy step (incremental value net) keeps hit-free rows and the others in separate arenas (BGAMD_SPLIT_ARENA=0: one)
    int expand_merged = 1;               // doubles plies + leaf stage in one launch (expand_all_kernel); BGAMD_EXPAND_MERGED=0: two launches
    int expand_parts = 3;                // timing experiments (BGAMD_EXPAND_PARTS): 1 = only the doubles turns are expanded, 2 = only the others
    int expand_dbl_npb = 128;            // ply-1 nodes a doubles workgroup takes per iteration (BGAMD_EXPAND_DBL_NPB: 64 .. XALL_NT)
    int expand_dbl_pct = 0;              // share of that launch's workgroups that takes the doubles turns (BGAMD_EXPAND_DBL_PCT: 5 .. 95; 0 = by env
                                         //   size: step_plan), the others take the non-doubles leaf stage
    int root_in_boundary = 1;            // inside a run the root pass of step t + 1 runs in the boundary launch of step t (bg_root_resident.h);
                                         //   BGAMD_ROOT_IN_BOUNDARY=0: a launch of its own every step, as up to round 3.
                                         //   By default from ROOT_IN_BOUNDARY_MIN lanes (round 4, profiles/r04_lanes_32768_anatomy.txt, r04_ab_root_pass_in_boundary.txt)
                                         //   -- there a boundary workgroup owns 128 games (BROOT_GPW), so 32 768 lanes still put a workgroup on every CU: 94.5 vs
                                         //   98.7 us per step with the pass as a launch of its own (65 536: 143.2 vs 143.6; 16 384: 72.0 vs 71.7, a tie: smaller
                                         //   envs keep the launch) -- and always on the caller's stream
    int overlap = 0;                     // BGAMD_OVERLAP=1: the root pass on the env's second stream beside the doubles plies; BGAMD_NO_OVERLAP set: everything
                                         //   on the caller's stream whatever BGAMD_OVERLAP says
    int root_f32_mfma = 0;               // root term by the f32 MFMA chain instead of the f16 / bf16 split (BGAMD_ROOT_F32=1)
    int root_resident = 1;               // the root pass with W1 resident in registers (BGAMD_ROOT_RESIDENT=0: the LDS-staged bf16 x 3 kernel).
                                         //   The leaf stage starts less obstructed beside it: with the counters packed (rounds 2-3a) the value net paid that
                                         //   back (step 0.1501 vs 0.1504 ms); with every counter on its own line it does not (leaf stage 0.0302 -> 0.0260,
                                         //   doubles plies 0.0180 -> 0.0195, step 0.1458 -> 0.1445 ms, same box, three interleaved runs)
};

// how a variable's text becomes its field's value
enum class StepRule {
    SWITCH,          // set: on unless atoi of it is 0 (so =0 turns a default-on switch off, =1 a default-off one on; "" and "x" read as 0)
    IN_RANGE,        // set and lo <= atoi <= hi: that number; anything else is ignored
    IN_RANGE_64,     // ... rounded down to a multiple of 64
    OFF_IF_SET,      // a switch that is off when the variable is set at all, whatever it says
};
// Round 5: the kernels and launch structures that lost their A/B (rounds 1-4) are honoured by the EXPERIMENTAL build only, as bit-identity
// references (tests/test_gpu_experimental.py).  In table order: BGAMD_NO_OVERLAP after BGAMD_OVERLAP, which it overrides.
constexpr struct { const char *var; int StepTuning::*field; StepRule rule; int lo, hi; } STEP_TUNING_VARS[] = {
    {"BGAMD_ROOT_F32", &StepTuning::root_f32_mfma, StepRule::SWITCH, 0, 0},
    {"BGAMD_ROOT_RESIDENT", &StepTuning::root_resident, StepRule::SWITCH, 0, 0},
    {"BGAMD_MFMA_DELTA", &StepTuning::mfma_delta, StepRule::SWITCH, 0, 0},
    {"BGAMD_F16X2_RESIDENT", &StepTuning::d16, StepRule::SWITCH, 0, 0},
    {"BGAMD_ROOT_IN_BOUNDARY", &StepTuning::root_in_boundary, StepRule::SWITCH, 0, 0},       // (overrides the size rule)
    {"BGAMD_EXPAND_MERGED", &StepTuning::expand_merged, StepRule::SWITCH, 0, 0},
    {"BGAMD_EXPAND_DBL_PCT", &StepTuning::expand_dbl_pct, StepRule::IN_RANGE, 5, 95},
    {"BGAMD_LIST_SHARDS", &StepTuning::list_shards, StepRule::SWITCH, 0, 0},
    {"BGAMD_SPLIT_ARENA", &StepTuning::split_arena, StepRule::SWITCH, 0, 0},
    {"BGAMD_EXPAND_PARTS", &StepTuning::expand_parts, StepRule::IN_RANGE, 1, 3},
    {"BGAMD_EXPAND_DBL_NPB", &StepTuning::expand_dbl_npb, StepRule::IN_RANGE_64, 64, XALL_NT},
    {"BGAMD_OVERLAP", &StepTuning::overlap, StepRule::SWITCH, 0, 0},
    {"BGAMD_NO_OVERLAP", &StepTuning::overlap, StepRule::OFF_IF_SET, 0, 0},
};

// The tuning of an env of n_games lanes.  get: name -> text or nullptr (getenv, or a test's own); experimental false (the default
// build): no variable is read, the result depends on n_games alone.
template <class GetEnv>
inline StepTuning step_tuning_from_env(GetEnv get, bool experimental, long long n_games)
{
    StepTuning u;
    u.root_in_boundary = n_games >= ROOT_IN_BOUNDARY_MIN;
    if (experimental)
        for (const auto &d : STEP_TUNING_VARS) {
            const char *s = get(d.var);
            if (!s) continue;
            int &x = u.*d.field;
            const int v = atoi(s);
            switch (d.rule) {
                case StepRule::SWITCH: x = v != 0; break;
                case StepRule::IN_RANGE: if (v >= d.lo && v <= d.hi) x = v; break;
                case StepRule::IN_RANGE_64: if (v >= d.lo && v <= d.hi) x = v & ~63; break;
                case StepRule::OFF_IF_SET: x = 0; break;
            }
        }
    if (LANE_NT != BROOT_THREADS) u.root_in_boundary = 0;        // (the in-launch root pass is written for 256-thread workgroups)
    return u;
}

// ---- grids that callers outside a run size too (bgamd_evaluate*, the rollout's truncation evaluator, the random step) ----
inline long long clamp_grid(long long b, long long lim) { return b < 1 ? 1 : (b > lim ? lim : b); }

// The dense evaluators.  Every workgroup first stages W1 in LDS: no more workgroups than the rows can use.
struct EvalGrids {
    long long lds;                       // eval_rows_f32 / bf16 / f16x2_kernel: a wave per 32-row tile, at most a workgroup per CU
    long long d16;                       // eval_rows_d16_kernel: a workgroup per tile, BG_D16_WAVES 4-wave workgroups per CU
};
inline EvalGrids eval_grids(long long est_rows, int n_cu)
{
    const long long rows_per_wg = (EVAL_THREADS / 64) * 32;
    return EvalGrids{clamp_grid((est_rows + rows_per_wg - 1) / rows_per_wg, n_cu), clamp_grid((est_rows + 31) / 32, (long long)BG_D16_WAVES * n_cu)};
}

// The incremental value net.  Every workgroup first copies W1^T (117 KB) into LDS: small envs get only as many as their rows can use.
inline long long delta_grid(long long est_rows, int n_cu) { return clamp_grid((est_rows + DELTA_THREADS - 1) / DELTA_THREADS, n_cu); }

// Its root pass: hidden[n][N_HID] = W1 x + b1 of the n root rows (one dense product per GAME)
enum class RootPass {
    NONE,            // a dense value-net mode: no root term
    RESIDENT,        // root_hidden_resident_kernel (the only one of the default build, and the only one that also runs inside boundary_kernel<true>)
    LDS_STAGED,      // root_hidden_bf16x3_kernel (BGAMD_ROOT_RESIDENT=0)
    F32_CHAIN,       // eval_rows_f32_kernel<true> (BGAMD_ROOT_F32=1; honoured by the step only: honours_f32)
};
inline RootPass root_pass_kind(const StepTuning &u, bool honours_f32)
{
    return honours_f32 && u.root_f32_mfma ? RootPass::F32_CHAIN : (u.root_resident ? RootPass::RESIDENT : RootPass::LDS_STAGED);
}
inline long long root_pass_grid(RootPass kind, long long n, int n_cu)
{
    if (kind == RootPass::F32_CHAIN) return n_cu;
    if (kind == RootPass::LDS_STAGED) return clamp_grid(((n + 31) / 32 + ROOT3_THREADS / 64 - 1) / (ROOT3_THREADS / 64), n_cu);
    return clamp_grid((n + 31) / 32, 2ll * n_cu);                // two 4-wave workgroups per CU (256 VGPRs each wave)
}

// rnd_count_kernel over `tasks` expected tasks (the random step: 64 per game; the exploring lanes of a greedy step: the figure of EST_DBL_NODES)
inline long long rnd_count_grid(long long tasks, int n_cu)
{
    const long long b = (tasks + 255) / 256, lim = (long long)n_cu * 8;
    return b > lim ? lim : b;
}

// ---- the plan of a run of greedy steps ----
struct StepPlan {
    bool incremental;                    // the incremental value net (BGAMD_F32): root pass + delta kernel; else one of the dense evaluators
    bool mfma_delta;                     // ... by eval_rows_mdelta_kernel (one row arena), else eval_rows_delta_kernel
    long long b_base;                    // StagedView::b_base: rows per arena, 0 = one arena
    long long xall_nd, xall_nl;          // expand_all_kernel: workgroups for the doubles turns / for the non-doubles leaf stage
    int shards;                          // StagedView::shards
    long long ply2_grid, leaf_grid;      // the two-launch expansion (BGAMD_EXPAND_MERGED=0): doubles_kernel, expand_kernel<MODE_LEAF>
    long long delta_grid;                // the incremental value net
    EvalGrids eval;                      // the dense evaluators
    RootPass root;                       // the root pass as a launch of its own
    long long root_grid;
    bool root_in_boundary;               // the root pass of step t + 1 may run inside the boundary launch of step t
    bool fused_with_more;                // a step that has a successor ends in the boundary launch (apply + the next roots), else apply, clear, roots
    long long sample_score_grid, sample_pick_grid;       // the sampled step's two passes
    long long rnd_count_grid;            // the exploring lanes' count launch
    int choice_eval, choice_root;        // bgamd_env_kernel_choice [0], and [1] of a step whose root pass is a launch of its own
};

// expand_kernel / doubles_kernel with nt threads: 48 B of LDS per thread, 2 048 threads per CU -- but one workgroup per CU for the
// 1 024-thread leaf stage (82 VGPRs: that is what fits; a second round of workgroups would start its latency chain from scratch, a
// second iteration of the same workgroup has its nodes prefetched)
inline long long expand_grid(long long max_items, int nt, int n_cu)
{
    return clamp_grid((max_items + nt - 1) / nt, (long long)n_cu * (nt >= 1024 ? 1 : 2048 / nt));
}

// n: lanes of the env; cap_rows: its row arena; wm_ok: the weight slot's W1 fits the MFMA delta kernel's f16 planes
inline StepPlan step_plan(const StepTuning &u, long long n, int n_cu, long long cap_rows, int precision, bool wm_ok)
{
    StepPlan p{};
    p.incremental = precision == BGAMD_F32;
    p.mfma_delta = p.incremental && u.mfma_delta && wm_ok;
    // separate row arenas (by class) for the VALU incremental value net; every other value-net kernel reads one
    p.b_base = (p.incremental && u.split_arena && !p.mfma_delta) ? (cap_rows / N_ARENAS) & ~63ll : 0;
    {   // grid of expand_all_kernel: two 512-thread workgroups per CU are resident, the first xall_nd take the doubles turns (one of each kind
        // per CU at the default share); the roots' lists in LIST_SHARDS parts when both counts divide
        const long long slots = (long long)XALL_WG_PER_CU * n_cu;
        long long nd = (n * EST_DBL_NODES + 63) / 64;               // doubles: ~64 ply-1 nodes per workgroup in a small env
        // the share of workgroups for the doubles turns: BGAMD_EXPAND_DBL_PCT, else by env size -- the doubles chains are what the launch waits
        // for, and the fewer lanes, the more so (32 768 lanes: 70 % 22.9 us, 50 % 25.1; 65 536: 62 % 28.5, 50 % 29.2; 16 384: 50 % 20.7, 63 % 21.3)
        const int pct = u.expand_dbl_pct > 0 ? u.expand_dbl_pct : (n >= 49152 ? 62 : (n >= 24576 ? 70 : 50));
        long long nd_lim = slots * pct / 100;
        if (nd_lim >= LIST_SHARDS) nd_lim -= nd_lim % LIST_SHARDS;  // (both counts multiples of the list parts: a full launch keeps the lists in parts)
        nd = nd < 1 ? 1 : (nd > nd_lim ? nd_lim : nd);
        const long long nl_lim = slots - nd_lim < 1 ? 1 : slots - nd_lim;
        p.xall_nd = nd;
        p.xall_nl = clamp_grid((n * EST_LEAF_PARENTS + XALL_NT - 1) / XALL_NT, nl_lim);
        p.shards = (u.expand_merged && u.list_shards && p.xall_nd % LIST_SHARDS == 0 && p.xall_nl % LIST_SHARDS == 0) ? LIST_SHARDS : 1;
    }
    p.ply2_grid = expand_grid(n * EST_DBL_NODES, EXPAND_NT_PLY, n_cu);
    p.leaf_grid = expand_grid(n * EST_LEAF_PARENTS, EXPAND_NT_LEAF, n_cu);
    p.delta_grid = delta_grid(n * EST_ROWS, n_cu);
    p.eval = eval_grids(n * EST_ROWS, n_cu);
    p.root = p.incremental ? root_pass_kind(u, true) : RootPass::NONE;
    p.root_grid = p.incremental ? root_pass_grid(p.root, n, n_cu) : 0;
    p.root_in_boundary = u.root_in_boundary && p.root == RootPass::RESIDENT;     // (the other root passes exist as launches only)
    // inside a run the apply of a step and the roots of the next share a launch; the counter set those roots allocate from is cleared
    // earlier in the step, while nothing uses it: by the expansion launch (every value-net mode), else by the incremental value net
    p.fused_with_more = p.incremental || u.expand_merged;
    // the sampled step.  Pass A is arithmetic (three Philox blocks and two logarithms per row) and takes every wave slot; pass B is a
    // compare per row and ends in one atomic per workgroup and counter
    const long long want = (n * EST_ROWS + SRCH_NT - 1) / SRCH_NT;
    p.sample_score_grid = clamp_grid(want, (long long)n_cu * 8);
    p.sample_pick_grid = clamp_grid(want, (long long)n_cu * 2);
    p.rnd_count_grid = rnd_count_grid(n * EST_DBL_NODES, n_cu);
    p.choice_eval = p.incremental ? (p.mfma_delta ? 1 : 0) : (precision == BGAMD_F32_DENSE ? 2 : precision == BGAMD_F16X2 ? (u.d16 ? 4 : 3) : 5);
    p.choice_root = (int)p.root;                                 // 0 none, 1 resident, 2 LDS-staged, 3 f32 chain
    return p;
}

// ---- the per-step facts ----
// root_ready: the boundary launch of the step before has already run this step's root pass
inline bool own_root_launch(const StepPlan &p, bool root_ready) { return p.incremental && !root_ready; }
// bgamd_env_kernel_choice [1]: 4 = the root pass ran inside the boundary launch before
inline int step_choice_root(const StepPlan &p, bool root_ready) { return p.incremental && root_ready ? 4 : p.choice_root; }
// bit 0 of bgamd_env_kernel_choice [2]: the root pass on the env's second stream (second_stream: the run has one, StepTuning::overlap)
inline int step_choice_forked(const StepPlan &p, bool root_ready, bool second_stream) { return own_root_launch(p, root_ready) && second_stream ? 1 : 0; }

}  // namespace bg
