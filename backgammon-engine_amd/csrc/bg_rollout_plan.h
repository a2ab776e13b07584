// bg_rollout_plan.h -- host-only part of the Monte Carlo rollout (bgamd_env_rollout_grouped, include/bgamd.h): whether a call is
// refused and with which code, how many lanes play its trials, how long a run between two refill points is, which buffers it needs
// and how big, and when the loop that waits for the trials stops.  Plain C++ (no HIP), like bg_step_plan.h: bgamd.hip's RolloutCall
// issues what a RolloutPlan names, tests/test_rollout_plan_cpu.py holds it against an independent restatement without a GPU and runs
// it under AddressSanitizer + UBSan (tests/sanitize/rollout_plan_driver.cpp).  The kernels: bg_rollout.h, bg_rollout_groups.h, bg_vr.h.
//
// This is the ONE place where the rollout's sizing rules and their constants live.
#pragma once
#include "../../include/bgamd.h"         // the flags and the error codes
#include "bg_search_plan.h"              // SEARCH_CHUNK, search_lanes: the scratch env of the 2-ply trials and of the luck pass

namespace bg {

// Default lanes of the scratch env that plays the trials (a 65 536-lane env: ~1.7 GB); fewer when the call has fewer trials.
constexpr long long ROLLOUT_LANES = 65536;
// Turns per run between two refill points (M > 0: the largest divisor of the turns a trial has left at its start not above it).  A trial
// that ends inside a run leaves its lane idle for the rest of the run: R / 2 turns per trial on average, against ~83 per game.
constexpr int ROLLOUT_RUN = 8;
constexpr int ROLLOUT_READ_TURNS = 16;   // turns between two reads of the trials-done counter, about
constexpr int ROLLOUT_DEFAULT_K = 8;     // candidates per lane the 2-ply trials' scratch env is sized for when top_k sets no limit
constexpr int ROLLOUT_FAN = 36;          // ordered dice pairs: the fan entries of a position under rotation, at most
constexpr int ROLLOUT_ROLLS = 21;        // rolls per position of the pre-roll evaluation and the search (= SRCH_ROLLS, bg_search_order.h)
// turns the done counter may stand still beyond the kernels' own limit (RO_TURN_LIMIT, bg_rollout.h) before the loop gives up
constexpr long long ROLLOUT_STALL_SLACK = 64;

// (SEARCH_CHUNK, the virtual lanes per scoring pass, and search_lanes: bg_search_plan.h)

// the arguments of a call that decide anything, and the env's sticky settings
struct RolloutRequest {
    int flags;
    long long n_positions, position_offset, trials, max_plies, lanes;
    bool has_states, has_group;          // d_states28 / d_group given
    int ro_plies, ro_top_k;              // bgamd_env_rollout_policy
    bool cube_on;                        // bgamd_env_rollout_cube
    bool has_weights[2];                 // the env's two weight slots
};

// elements per capacity of the env's buffer groups (RolloutState), 0 = not needed by this call
struct RolloutNeeds {
    long long pos, fan, trials, lanes;   // the positions, the rotation fan, per trial, per lane
    long long vtrials, vlanes, vpos;     // the luck pass
    long long group;                     // the group table
    long long ctrials, cstart;           // the cube
};

struct RolloutPlan {
    int rc;                              // BGAMD_OK, or the code the call returns before anything is issued: nothing below is set then
    long long P, T, N, M;                // positions, trials of each, trials in all, the horizon (0: whole games)
    bool rotate, vr, cube, grouped, two_ply;
    int slot, run_flags;                 // the weight slot, and the flags every step of the trial env gets
    long long F, n_fan;                  // fan entries per position and in all
    long long L;                         // lanes of the trial env (exactly)
    long long fan_chunks;                // steps of the trial env that play the fan, L entries at a time
    bool fan_eval;                       // M = 1: a rotated trial ends with its fan entry, scored by the value net
    unsigned long long lane_offset;      // the trial env's: trial jl plays game id position_offset T + jl as episode jl + L - g of lane g
    int R, G;                            // turns per run, and runs between two reads of the trials-done counter
    bool truncates;                      // a refill also scores the trials that reached the horizon
    long long search_scratch_lanes;      // two_ply: lanes of the env the search's virtual roots are scored on (0: not asked for)
    long long preroll_positions, preroll_lanes;      // vr: what the pre-roll passes score at most at once, and that env's lanes
    RolloutNeeds needs;
    long long stall_turns, stall_limit;  // a read-back without progress counts stall_turns (G R) turns; more than stall_limit: give up
};

// turn_limit: RO_TURN_LIMIT of the kernels (bg_rollout.h)
inline RolloutPlan rollout_plan(const RolloutRequest &q, long long turn_limit)
{
    RolloutPlan p{};
    const int known = BGAMD_ROLLOUT_ROTATE | BGAMD_WEIGHTS_SLOT1 | BGAMD_ROLLOUT_VR;
    p.rc = BGAMD_E_INVALID;
    if (!q.has_states || q.n_positions < 1 || q.trials < 1 || q.max_plies < 0 || q.lanes < 0 || q.position_offset < 0) return p;
    if (q.flags & ~known) return p;
    if (q.n_positions >= (1ll << 31) || q.trials >= (1ll << 31) || q.n_positions * q.trials >= (1ll << 31) || q.lanes > (1ll << 30)) return p;
    // the cube rides on the luck pass's pre-roll means: without them there is nothing to decide on
    if (q.cube_on && !(q.flags & BGAMD_ROLLOUT_VR)) return p;
    const int slot = (q.flags & BGAMD_WEIGHTS_SLOT1) ? 1 : 0;
    if (!q.has_weights[slot]) { p.rc = BGAMD_E_NOWEIGHTS; return p; }
    p.rc = BGAMD_OK;
    p.slot = slot;

    p.P = q.n_positions; p.T = q.trials; p.N = p.P * p.T; p.M = q.max_plies;
    p.rotate = (q.flags & BGAMD_ROLLOUT_ROTATE) != 0;
    p.vr = (q.flags & BGAMD_ROLLOUT_VR) != 0;
    p.cube = q.cube_on;
    p.grouped = q.has_group;
    p.two_ply = q.ro_plies == 2;
    p.run_flags = q.flags & BGAMD_WEIGHTS_SLOT1;
    p.F = p.rotate ? (p.T < ROLLOUT_FAN ? p.T : ROLLOUT_FAN) : 0;
    p.n_fan = p.P * p.F;
    p.L = q.lanes > 0 ? q.lanes : (p.N < ROLLOUT_LANES ? ((p.N + 255) / 256) * 256 : ROLLOUT_LANES);
    p.fan_chunks = (p.n_fan + p.L - 1) / p.L;
    p.fan_eval = p.rotate && p.M == 1;
    p.lane_offset = (unsigned long long)q.position_offset * (unsigned long long)p.T - (unsigned long long)p.L;

    // refill points every R turns; M > 0: R divides M - (first ply), so every trial's M-th turn ends a run
    p.R = ROLLOUT_RUN;
    if (p.M > 0) {
        const long long D = p.M - (p.rotate ? 1 : 0);
        p.R = D < 1 ? 1 : (int)(D < ROLLOUT_RUN ? D : ROLLOUT_RUN);
        while (D > 0 && D % p.R) --p.R;
    }
    if (p.two_ply) p.R = 1;              // a search turn is a step of its own: a refill after every turn
    p.G = p.R >= ROLLOUT_READ_TURNS ? 1 : ROLLOUT_READ_TURNS / p.R;
    p.truncates = p.M > 0;

    // plies = 2 (bgamd_env_rollout_policy): every turn is one filtered search step of the trial env.  Its virtual roots are scored on
    // the CALLER's env's scratch env, lent to the trial env for the step: the luck pass uses the same one between the steps (everything
    // is stream-ordered), and a second env of up to SEARCH_CHUNK lanes (~3.4 GB) would buy nothing.  It is sized once, for top_k (8 when
    // there is no limit) candidates per lane, so that a turn with many candidates does not re-create it; the search's per-lane and
    // candidate buffers of the trial env come to ~0.2 GB at 65 536 lanes and top_k 5 (2 x 67 MB of row indices and ranks, 43 MB of candidates).
    p.search_scratch_lanes = p.two_ply ? search_lanes(p.L * (long long)(q.ro_top_k > 0 ? q.ro_top_k : ROLLOUT_DEFAULT_K) * ROLLOUT_ROLLS) : 0;
    // the luck pass scores the P positions once (rotation: turn 0's luck), then the L trial lanes before every turn
    p.preroll_positions = p.vr ? ((p.rotate ? p.P : 0) > p.L ? p.P : p.L) : 0;
    p.preroll_lanes = p.vr ? search_lanes(p.preroll_positions * ROLLOUT_ROLLS) : 0;

    p.needs.pos = p.P; p.needs.fan = p.n_fan; p.needs.trials = p.N; p.needs.lanes = p.L;
    if (p.vr) { p.needs.vtrials = p.N; p.needs.vlanes = p.L; p.needs.vpos = p.P; }
    if (p.grouped) p.needs.group = p.P;
    if (p.cube) { p.needs.ctrials = p.N; p.needs.cstart = p.P; }

    p.stall_turns = (long long)p.G * p.R;
    p.stall_limit = turn_limit + ROLLOUT_STALL_SLACK;       // (cannot be reached: the kernels' own limit fires first)
    return p;
}

// The loop's decision on a read-back of (trials done, the rollout's error bits, the trial env's error bits)
struct RolloutProgress {
    enum Verdict { GO_ON = 0, FINISHED = 1, STALLED = 2 };
    long long N, stall_turns, stall_limit;
    unsigned long long last_done = 0;
    long long stalled = 0;               // turns issued since the done counter last moved

    explicit RolloutProgress(const RolloutPlan &p) : N(p.N), stall_turns(p.stall_turns), stall_limit(p.stall_limit) {}
    Verdict read(unsigned long long done, unsigned long long ro_err, unsigned long long env_err)
    {
        if (done >= (unsigned long long)N || ro_err || env_err) return FINISHED;     // (an error ends the loop: the caller reads it afterwards)
        stalled = done == last_done ? stalled + stall_turns : 0;
        last_done = done;
        return stalled > stall_limit ? STALLED : GO_ON;
    }
};

}  // namespace bg
