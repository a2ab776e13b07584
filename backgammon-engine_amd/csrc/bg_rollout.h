// bg_rollout.h -- kernels of the batched Monte Carlo rollout (bgamd_env_rollout, include/bgamd.h).  Included by bgamd.hip inside its
// anonymous namespace, after the 2-ply search's kernels.
//
//   prep      pack_rows_kernel                 : the P positions as 32-byte rows (turn bit = side to move), bad states flagged
//   rotation  ro_fan_seed / greedy step / ro_fan_collect : one greedy step with injected dice on P x min(T, 36) virtual lanes of
//             the scratch env gives every position's first-turn afterstates (row, turn bit = the side now to move)
//   loop      ro_refill (lane per scratch lane) : a lane whose trial ended (frozen) or reached M turns hands its result to the trial's
//             slot and takes the next unstarted trial; truncated trials go to a compact row list scored by the dense fp32 evaluator
//             (launch_eval, what bgamd_evaluate_slot runs) and ro_trunc_scatter; between refills the greedy step's own kernels play
//             R turns of every lane (GreedyRun), R dividing the turns a trial has left at its start when M > 0
//   reduce    ro_reduce (wave per position)    : mean, stderr, turns, truncated in a fixed order; per-trial outputs
//   outcomes  ro_outcome_reduce (wave per position, launched by bgamd_env_rollout_outcomes_read) : every trial's points
//             (outcome_points of the board it was scored from, bg_outcome.h; 0 = truncated) -> the six counts and the equity
#pragma once

constexpr int RO_NT = 256;
constexpr uint32_t RO_NONE = 0xFFFFFFFFu;            // lane_trial of a lane without a trial
constexpr uint32_t RO_TRUNC = 1u << 30;              // internal trial_turns: the trial was scored by the net
constexpr int RO_PTS_SHIFT = 17;                     // internal trial_turns, bits 17..19: the trial's points (outcome_points, bg_outcome.h) as a
constexpr uint32_t RO_TURN_MASK = (1u << RO_PTS_SHIFT) - 1u;   // 3-bit two's complement, 0 = truncated; the turns (<= RO_TURN_LIMIT + 1 < 2^17) below
constexpr uint32_t RO_TURN_LIMIT = 100000;           // M = 0: a trial still running after this many turns is an error
enum { RO_NEXT = 0, RO_DONE = 1, RO_NTRUNC = 2, RO_ERR = 3, RO_CTRS = 4 };
enum { ERRF_RO_LONG = 8, ERRF_RO_PLY = 16 };
enum { ERRF_RO_GROUP = 256 };                        // intake word, beside ERRF_STATE: a bad group table (bg_rollout_groups.h)
enum { ERRF_RO_CUBE = 512 };                         // intake word: a bad entry of the cube's start tables (bg_cube.h)

struct RoView {
    long long N, T, M;                                // trials in all, per position, turn limit (0 = none)
    int rotate;
    long long F;                                      // rotation: fan entries per position (min(T, 36))
    const uint4 *pos_rows;                            // [P][2]
    const uint4 *fan_rows;                            // [P * F][2]
    const float *fan_val;                             // [P * F] (M == 1 only)
    uint32_t *lane_trial;                             // [L]
    float *t_val;                                     // [N]
    uint32_t *t_turns;                                // [N] turns | points << RO_PTS_SHIFT | RO_TRUNC
    uint4 *trows;                                     // [L][2] truncated trials of this refill
    uint32_t *tids;                                   // [L]
    unsigned long long *ctr;                          // RO_*
    const int32_t *group;                             // [P] dice group of every position (bgamd_env_rollout_grouped), NULL: its own
};

// One global atomic per workgroup: the lanes with `want` get consecutive slots of *ctr in thread order.  Every thread of the workgroup
// calls it.  -> the lane's slot (undefined without want); *tot = the workgroup's count (the same in every thread)
__device__ __forceinline__ unsigned long long ro_block_alloc(bool want, unsigned long long *ctr, uint32_t *tot)
{
    __shared__ uint32_t s_wcnt[RO_NT / 64];
    __shared__ unsigned long long s_base;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(want);
    const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wcnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < RO_NT / 64; ++w) {
        const uint32_t c = s_wcnt[w];
        before += w < wave ? c : 0u;
        all += c;
    }
    if (threadIdx.x == 0 && all) s_base = atomicAdd(ctr, (unsigned long long)all);
    __syncthreads();
    const unsigned long long base = all ? s_base : 0ull;
    __syncthreads();                                  // s_wcnt / s_base are rewritten by the next call
    *tot = all;
    return base + before + rank;
}

// a scored trial's word: its turns and the points of the board it was scored from, in the one store the turns always took
__device__ __forceinline__ uint32_t ro_turns_word(uint32_t turns, const uint32_t (&p)[8])
{
    return turns | (((uint32_t)outcome_points(p) & 7u) << RO_PTS_SHIFT);
}
__device__ __forceinline__ int ro_word_points(uint32_t w) { return (int)(w << (29 - RO_PTS_SHIFT)) >> 29; }

__device__ __forceinline__ void ro_row(const uint32_t (&p)[8], int turn, uint4 *dst)
{
    dst[0] = make_uint4(p[0] | (turn ? TURN_BIT : 0u), p[1], p[2], p[3]);
    dst[1] = make_uint4(p[4], p[5], p[6], p[7]);
}
__device__ __forceinline__ int ro_unrow(const uint4 *src, uint32_t (&p)[8])
{
    const uint4 a = src[0], b = src[1];
    p[0] = a.x & ~TURN_BIT; p[1] = a.y; p[2] = a.z; p[3] = a.w; p[4] = b.x; p[5] = b.y; p[6] = b.z; p[7] = b.w;
    return (a.x & TURN_BIT) ? 1 : 0;
}

// virtual lane l = fan entry v = v0 + l = (position v / F, ordered dice pair v % F): the position with pair r = v % F's dice,
// d1 = 1 + r / 6, d2 = 1 + r % 6.  Past the list, or on a finished position: a frozen lane (no roots, no rows).
__global__ __launch_bounds__(RO_NT) void ro_fan_seed_kernel(EnvView e, long long v0, long long n_fan, RoView r)
{
    const long long l = (long long)blockIdx.x * RO_NT + threadIdx.x;
    if (l >= e.n) return;
    const long long v = v0 + l;
    uint32_t p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t meta = META_FINISHED;
    if (v < n_fan) {
        const int turn = ro_unrow(r.pos_rows + 2 * (v / r.F), p);
        const int k = (int)(v % r.F);
        if (!over_code(p)) meta = meta_pack(turn, 1 + k / 6, 1 + k % 6, false);
    }
    store_planes(e, l, p);
    e.meta[l] = meta; e.ply[l] = 0; e.episode[l] = 0; e.flags[l] = 0;
}

// the afterstate of every fan entry as a row with the turn bit of the side now to move (a game that ended: the board decides)
__global__ __launch_bounds__(RO_NT) void ro_fan_collect_kernel(EnvView e, long long v0, long long n_fan, uint4 *__restrict__ fan_rows)
{
    const long long l = (long long)blockIdx.x * RO_NT + threadIdx.x;
    if (l >= e.n || v0 + l >= n_fan) return;
    uint32_t p[8];
    load_planes(e, l, p);
    ro_row(p, (int)(e.meta[l] & 1u), fan_rows + 2 * (v0 + l));
}

// Refill point.  Lane g: a frozen lane's trial ended (1.0 if PLAYER1 won, turns = ply + 1: finish_turn does not advance the ply of a
// game's last turn); a live lane at ply M is truncated (its row goes to the compact list, scored after this launch).  Every place that
// scores a trial from a board also records its points (single game / gammon / backgammon) above the turns; a truncated trial's are 0.
// A lane without a trial then takes the next unstarted one, trial jl = p T + i: at ply 0 from position p, or -- rotation -- at ply 1 from fan entry
// p F + i % 36.  Trials that are over before a turn is played on a lane (a finished position: 0 turns; rotation: a first turn that
// ended the game, or M = 1) are scored here and the lane takes the next.  The lane plays trial jl as episode jl + L - g with lane_stride 1
// and lane_offset = base - L: game id base + jl, the dice of trial j = base + jl at every ply.  With a group table (r.group) the slot
// and the dice id are two numbers: the trial's result still goes to slot jl, but it is played as episode group[p] T + i + L - g with
// lane_offset = group_offset T - L: game id (group_offset + group[p]) T + i, the same dice for trial i of every position of a group.
__global__ __launch_bounds__(RO_NT) void ro_refill_kernel(EnvView e, RoView r)
{
    const long long g = (long long)blockIdx.x * RO_NT + threadIdx.x;
    const bool in = g < e.n;
    uint32_t j = in ? r.lane_trial[g] : RO_NONE;
    bool want = in, trunc = false;
    uint32_t done = 0, err = 0;
    uint32_t p[8];
    if (j != RO_NONE) {
        load_planes(e, g, p);
        const uint32_t meta = e.meta[g], ply = e.ply[g];
        if (meta & META_FINISHED) {
            r.t_val[j] = over_code(p) == 1 ? 1.0f : 0.0f;
            r.t_turns[j] = ro_turns_word(ply + 1u, p);
            ++done;
        } else if (r.M > 0 && (long long)ply >= r.M) {
            if ((long long)ply > r.M) err |= ERRF_RO_PLY;
            r.t_turns[j] = ply | RO_TRUNC;
            trunc = true;
            ++done;
        } else {
            if (ply >= RO_TURN_LIMIT) err |= ERRF_RO_LONG;
            want = false;                                      // still running
        }
    }
    const bool was_free = want;
    // truncated rows: one compact list for the evaluator
    uint32_t tot;
    const unsigned long long k = ro_block_alloc(trunc, &r.ctr[RO_NTRUNC], &tot);
    if (trunc) {
        ro_row(p, (int)(e.meta[g] & 1u), r.trows + 2 * k);
        r.tids[k] = j;
    }
    // seat: rounds of one trial per lane that wants one, until every such lane has one or none is left
    bool seated = false;
    for (;;) {
        const unsigned long long jj = ro_block_alloc(want, &r.ctr[RO_NEXT], &tot);
        if (tot == 0) break;                                   // (the same in every thread)
        if (!want) continue;
        if (jj >= (unsigned long long)r.N) { want = false; continue; }     // nothing left: the lane idles
        const uint32_t jl = (uint32_t)jj;
        const long long pi = (long long)jl / r.T, i = (long long)jl % r.T;
        int turn = ro_unrow(r.pos_rows + 2 * pi, p);
        int oc = over_code(p);
        uint32_t ply = 0;
        if (!oc && r.rotate) {
            const long long f = pi * r.F + i % 36;
            turn = ro_unrow(r.fan_rows + 2 * f, p);
            oc = over_code(p);
            ply = 1;
            if (!oc && r.M == 1) { r.t_val[jl] = r.fan_val[f]; r.t_turns[jl] = 1u | RO_TRUNC; ++done; continue; }
        }
        if (oc) {                                              // over before this lane plays a turn of it
            r.t_val[jl] = oc == 1 ? 1.0f : 0.0f;
            r.t_turns[jl] = ro_turns_word(ply, p);
            ++done;
            continue;
        }
        store_planes(e, g, p);
        e.meta[g] = meta_pack(turn, 0, 0, false);
        e.ply[g] = ply;
        e.episode[g] = (r.group ? (uint32_t)r.group[pi] * (uint32_t)r.T + (uint32_t)i : jl) + (uint32_t)e.n - (uint32_t)g;
        e.flags[g] = 0;
        r.lane_trial[g] = jl;
        seated = true;
        want = false;
    }
    if (was_free && !seated) {                                 // an idle lane: frozen, no trial
        e.meta[g] = META_FINISHED;
        r.lane_trial[g] = RO_NONE;
    }
    // done / error words: one atomic per workgroup
    __shared__ uint32_t s_done, s_err;
    if (threadIdx.x == 0) { s_done = 0; s_err = 0; }
    __syncthreads();
    if (done) atomicAdd(&s_done, done);
    if (err) atomicOr(&s_err, err);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_done) atomicAdd(&r.ctr[RO_DONE], (unsigned long long)s_done);
        if (s_err) atomicOr(&r.ctr[RO_ERR], (unsigned long long)s_err);
    }
}

// the evaluator's values of this refill's truncated trials into their slots; the list is emptied for the next refill
__global__ __launch_bounds__(RO_NT) void ro_trunc_scatter_kernel(RoView r, const float *__restrict__ vals)
{
    const unsigned long long n = r.ctr[RO_NTRUNC];
    for (unsigned long long k = (unsigned long long)blockIdx.x * RO_NT + threadIdx.x; k < n; k += (unsigned long long)gridDim.x * RO_NT)
        r.t_val[r.tids[k]] = vals[k];
}

// wave per position: sums over the position's T trial slots in a fixed order (lane i takes trials i, i + 64, ...; then a fixed
// butterfly, lane 0's result) -- the same bits for any lane count of the scratch env
__device__ __forceinline__ double ro_wave_sum(double s)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    return __shfl(s, 0, 64);
}
__global__ __launch_bounds__(64) void ro_reduce_kernel(long long T, const float *__restrict__ t_val, const uint32_t *__restrict__ t_turns,
                                                       double *__restrict__ mean, double *__restrict__ serr, int64_t *__restrict__ turns,
                                                       int32_t *__restrict__ truncated, float *__restrict__ o_val, int32_t *__restrict__ o_turns)
{
    const long long p = blockIdx.x, base = p * T;
    const int lane = threadIdx.x;
    double s = 0.0;
    unsigned long long ts = 0;
    uint32_t tr = 0;
    for (long long i = lane; i < T; i += 64) {
        const float x = t_val[base + i];
        const uint32_t w = t_turns[base + i];
        s += (double)x;
        ts += w & RO_TURN_MASK;
        tr += (w & RO_TRUNC) ? 1u : 0u;
        if (o_val) o_val[base + i] = x;
        if (o_turns) o_turns[base + i] = (int32_t)(w & RO_TURN_MASK);
    }
    const double m = ro_wave_sum(s) / (double)T;
    double q = 0.0;
    for (long long i = lane; i < T; i += 64) {
        const double d = (double)t_val[base + i] - m;
        q += d * d;
    }
    q = ro_wave_sum(q);
    unsigned long long t64 = ts;
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)t64, k, 64), hi = __shfl_xor((uint32_t)(t64 >> 32), k, 64);
        t64 += ((unsigned long long)hi << 32) | lo;
    }
    const unsigned long long trs = wave_sum_u32(tr);
    if (lane == 0) {
        if (mean) mean[p] = m;
        if (serr) serr[p] = T > 1 ? sqrt(q / ((double)T * (double)(T - 1))) : 0.0;
        if (turns) turns[p] = (int64_t)t64;
        if (truncated) truncated[p] = (int32_t)trs;
    }
}

// Outcomes of the trials, wave per position in ro_reduce_kernel's order (lane i takes trials i, i + 64, ...; the same butterfly; lane 0
// writes).  counts[p][6]: PLAYER1 single / gammon / backgammon, PLAYER2 single / gammon / backgammon.  Equity of a trial in points:
// its points when it was played out, 2 x - 1 of its fp32 net value x when it was truncated (the net knows wins only).
template <int LAST>                                   // (a template for its place in the code object: bg_outcome.h)
__global__ __launch_bounds__(64) void ro_outcome_reduce_kernel(long long T, const float *__restrict__ t_val, const uint32_t *__restrict__ t_turns,
                                                               int64_t *__restrict__ counts, double *__restrict__ equity,
                                                               double *__restrict__ eq_serr, int8_t *__restrict__ o_pts)
{
    const long long p = blockIdx.x, base = p * T;
    const int lane = threadIdx.x;
    auto eq = [&](long long i) -> double {
        const int w = ro_word_points(t_turns[base + i]);
        return w ? (double)w : 2.0 * (double)t_val[base + i] - 1.0;
    };
    double s = 0.0;
    uint32_t c[6] = {0, 0, 0, 0, 0, 0};
    for (long long i = lane; i < T; i += 64) {
        const int w = ro_word_points(t_turns[base + i]);
        s += eq(i);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c[k] += w == k + 1 ? 1u : 0u;
            c[3 + k] += w == -(k + 1) ? 1u : 0u;
        }
        if (o_pts) o_pts[base + i] = (int8_t)w;
    }
    const double m = ro_wave_sum(s) / (double)T;
    double q = 0.0;
    for (long long i = lane; i < T; i += 64) {
        const double d = eq(i) - m;
        q += d * d;
    }
    q = ro_wave_sum(q);
    unsigned long long cs[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) cs[k] = wave_sum_u32(c[k]);
    if (lane == 0) {
        if (counts) {
#pragma unroll
            for (int k = 0; k < 6; ++k) counts[p * 6 + k] = (int64_t)cs[k];
        }
        if (equity) equity[p] = m;
        if (eq_serr) eq_serr[p] = T > 1 ? sqrt(q / ((double)T * (double)(T - 1))) : 0.0;
    }
}
