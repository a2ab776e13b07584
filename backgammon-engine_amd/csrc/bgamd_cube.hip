// bgamd_cube.hip -- the kernels of the doubling cube on the rollout's trials and their launches (bg_cube.h holds the record, the rule's
// parameters and the prototypes; include/bgamd.h, bgamd_env_rollout_cube, states the rule).  A translation unit of its own, linked into
// libbgamd.so behind bgamd_search3.hip: its kernels are a third gfx950 code object, and bgamd.hip's does not change when one is added
// here.  It shares with bgamd.hip only what both must agree on: the row format (bg_board.h) and the constants bg_cube.h restates.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bg_board.h"
#include "bg_cube.h"
#include "bg_match.h"

using namespace bg;
using bg::cube::Rule;
using bg::cube::Trial;

namespace {
constexpr int CUBE_NT = 256;

// pre_mean of bg_vr.h, operation for operation: the sum over the 21 rolls in order of w_r (double) f_r, a rounded fp64 product and a
// rounded fp64 sum per roll -- the mean bgamd_env_evaluate_preroll returns and ro_vr_luck_kernel subtracts, bit for bit
__device__ __forceinline__ double cube_pre_mean(const float *__restrict__ f)
{
    double s = 0.0;
#pragma unroll
    for (int idx = 0, a = 1; a <= 6; ++a)
#pragma unroll
        for (int d = a; d <= 6; ++d, ++idx) s = __dadd_rn(s, __dmul_rn(a == d ? 1.0 / 36.0 : 2.0 / 36.0, (double)f[idx]));
    return s;
}

// The decision before turn k of a trial whose position is not over: `mover` (0 PLAYER1, 1 PLAYER2) is to roll, mean = mean(s_k).
// -> the record changed
__device__ __forceinline__ bool cube_offer(Trial &t, int mover, double mean, uint32_t k, const Rule &r)
{
    const uint32_t owner = t.info & cube::INFO_OWNER;
    if (t.dropped >= 0 || t.value >= r.max_cube || !(owner == 0u || owner == (uint32_t)mover + 1u)) return false;
    const double w = mover ? 1.0 - mean : mean;
    if (!(r.double_at <= w && w <= r.too_good_at)) return false;
    const uint32_t opp = 2u - (uint32_t)mover;             // the other side's number: PLAYER2 = 2 when PLAYER1 rolls
    if (w > r.pass_at) {
        t.dropped = (int32_t)k;
        t.info |= opp << cube::INFO_PASSED_SHIFT;
    } else {
        t.value *= 2u;
        t.info = ((t.info & ~cube::INFO_OWNER) | opp) + (1u << cube::INFO_TURNS_SHIFT);
    }
    return true;
}

template <int NT>
__global__ __launch_bounds__(NT) void ro_cube_intake_kernel(long long P, const int32_t *__restrict__ d_value, const int32_t *__restrict__ d_owner,
                                                            uint32_t *__restrict__ start, unsigned long long *err, unsigned long long err_bit)
{
    const long long p = (long long)blockIdx.x * NT + threadIdx.x;
    if (p >= P) return;
    const int32_t v = d_value ? d_value[p] : 1, o = d_owner ? d_owner[p] : 0;
    const bool bad = v < 1 || v > (1 << 30) || (v & (v - 1)) != 0 || o < 0 || o > 2;
    if (bad) atomicOr(err, err_bit);
    start[p] = bad ? 1u : (uint32_t)v;
    start[P + p] = bad ? 0u : (uint32_t)o;
}

// thread per trial jl = p T + i: the record's start, and the decision before a rotated turn 0 (turn index 0, the position's own mean)
template <int NT>
__global__ __launch_bounds__(NT) void ro_cube_init_kernel(long long N, long long T, int rotate, const uint4 *__restrict__ pos_rows,
                                                          const uint32_t *__restrict__ start, long long P, const double *__restrict__ mean0,
                                                          Rule rule, Trial *__restrict__ trials)
{
    const long long jl = (long long)blockIdx.x * NT + threadIdx.x;
    if (jl >= N) return;
    const long long pi = jl / T;
    Trial t{start[pi], -1, start[P + pi], 0u};
    if (rotate && !rule.hold_turn0) {
        const uint4 a = pos_rows[2 * pi], b = pos_rows[2 * pi + 1];
        const uint32_t p[8] = {a.x & ~TURN_BIT, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        if (!over_code(p)) cube_offer(t, (a.x & TURN_BIT) ? 1 : 0, mean0[pi], 0u, rule);
    }
    *reinterpret_cast<uint4 *>(trials + jl) = make_uint4(t.value, (uint32_t)t.dropped, t.info, 0u);
}

// thread per trial lane g, after the pre-roll pass of the turn at hand (f[g][21]): a live lane's trial j gets the decision before its turn
// ply[g].  A trial is on one lane at a time, so its record has one writer.  ctr: lane-turns played, and those of them played after the
// trial's drop, the turn the drop is made before included (one atomic pair per wave).
template <int NT>
__global__ __launch_bounds__(NT) void ro_cube_turn_kernel(long long L, const uint32_t *__restrict__ meta, const uint32_t *__restrict__ ply,
                                                          const uint32_t *__restrict__ lane_trial, const float *__restrict__ f, Rule rule,
                                                          Trial *__restrict__ trials, unsigned long long *__restrict__ ctr)
{
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    bool live = false, after = false;
    if (g < L) {
        const uint32_t m = meta[g], j = lane_trial[g];
        live = !(m & cube::LANE_FINISHED) && j != cube::LANE_NONE;
        if (live) {
            const uint4 w = *reinterpret_cast<const uint4 *>(trials + j);
            Trial t{w.x, (int32_t)w.y, w.z, w.w};
            const uint32_t k = ply[g];
            if (t.dropped < 0 && !(rule.hold_turn0 && k == 0u) && cube_offer(t, (int)(m & 1u), cube_pre_mean(f + g * cube::ROLLS), k, rule))
                *reinterpret_cast<uint4 *>(trials + j) = make_uint4(t.value, (uint32_t)t.dropped, t.info, w.w);
            after = t.dropped >= 0;                        // (the turn a drop is made before is played after it)
        }
    }
    const unsigned long long nl = (unsigned long long)__popcll(__ballot(live)), na = (unsigned long long)__popcll(__ballot(after));
    if ((threadIdx.x & 63) == 0) {
        if (nl) atomicAdd(&ctr[cube::CTR_TURNS], nl);
        if (na) atomicAdd(&ctr[cube::CTR_AFTER_DROP], na);
    }
}

__device__ __forceinline__ double cube_wave_sum(double s)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s = __dadd_rn(s, __shfl_xor(s, m, 64));
    return __shfl(s, 0, 64);
}
__device__ __forceinline__ unsigned long long cube_wave_sum_u64(unsigned long long s)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)s, m, 64), hi = __shfl_xor((uint32_t)(s >> 32), m, 64);
        s += ((unsigned long long)hi << 32) | lo;
    }
    return s;
}

// the cubeful equity of a trial from PLAYER1's side: a drop pays the cube as it stood (the side that did not pass wins it); a trial that
// ended on the board pays cube x points (Jacoby, the cube never turned in the trial: cube x the sign of the points); a truncated one
// cube x (2 x - 1) of its fp32 net value x
__device__ __forceinline__ double cube_equity(const Trial &t, float x, uint32_t word, int jacoby)
{
    const double c = (double)t.value;
    if (t.dropped >= 0) return ((t.info >> cube::INFO_PASSED_SHIFT) & 3u) == 2u ? c : -c;
    int pts = (int)(word << (29 - cube::WORD_PTS_SHIFT)) >> 29;
    if (pts == 0) return __dmul_rn(c, __dsub_rn(__dmul_rn(2.0, (double)x), 1.0));
    if (jacoby && (t.info >> cube::INFO_TURNS_SHIFT) == 0u) pts = pts > 0 ? 1 : -1;
    return __dmul_rn(c, (double)pts);
}

// Wave per position in ro_reduce_kernel's order: lane k takes trials k, k + 64, ...; the xor butterfly; lane 0 writes.  Every sum is a
// chain of rounded fp64 additions (no fused multiply-add), so a host restates it exactly.  counts[p][4]: trials PLAYER1 passed, trials
// PLAYER2 passed, cube turns in all, trials whose final cube is >= max_cube.
template <int NT>
__global__ __launch_bounds__(NT) void ro_cube_reduce_kernel(long long T, const float *__restrict__ t_val, const uint32_t *__restrict__ t_turns,
                                                            const Trial *__restrict__ trials, Rule rule, double *__restrict__ t_eq,
                                                            double *__restrict__ mean, double *__restrict__ serr, int64_t *__restrict__ counts,
                                                            double *__restrict__ o_eq, int32_t *__restrict__ o_cube, int32_t *__restrict__ o_dropped)
{
    static_assert(NT == 64, "one wave per position");
    const long long p = blockIdx.x, base = p * T;
    const int lane = threadIdx.x;
    double s = 0.0;
    unsigned long long c[4] = {0ull, 0ull, 0ull, 0ull};
    for (long long i = lane; i < T; i += 64) {
        const uint4 w = *reinterpret_cast<const uint4 *>(trials + base + i);
        const Trial t{w.x, (int32_t)w.y, w.z, w.w};
        const double e = cube_equity(t, t_val[base + i], t_turns[base + i], rule.jacoby);
        s = __dadd_rn(s, e);
        const uint32_t passed = (t.info >> cube::INFO_PASSED_SHIFT) & 3u;
        c[0] += passed == 1u ? 1ull : 0ull;
        c[1] += passed == 2u ? 1ull : 0ull;
        c[2] += t.info >> cube::INFO_TURNS_SHIFT;
        c[3] += t.value >= rule.max_cube ? 1ull : 0ull;
        t_eq[base + i] = e;
        if (o_eq) o_eq[base + i] = e;
        if (o_cube) o_cube[base + i] = (int32_t)t.value;
        if (o_dropped) o_dropped[base + i] = t.dropped;
    }
    const double m = cube_wave_sum(s) / (double)T;
    double q = 0.0;
    for (long long i = lane; i < T; i += 64) {
        const uint4 w = *reinterpret_cast<const uint4 *>(trials + base + i);
        const Trial t{w.x, (int32_t)w.y, w.z, w.w};
        const double d = __dsub_rn(cube_equity(t, t_val[base + i], t_turns[base + i], rule.jacoby), m);
        q = __dadd_rn(q, __dmul_rn(d, d));
    }
    q = cube_wave_sum(q);
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = cube_wave_sum_u64(c[k]);
    if (lane == 0) {
        if (mean) mean[p] = m;
        if (serr) serr[p] = T > 1 ? sqrt(q / ((double)T * (double)(T - 1))) : 0.0;
        if (counts) {
#pragma unroll
            for (int k = 0; k < 4; ++k) counts[p * 4 + k] = (int64_t)c[k];
        }
    }
}

// bgamd_env_rollout_paired_read's which = 3: ro_pair_reduce_kernel's rule (bg_rollout_groups.h) on the per-trial cubeful equities that
// ro_cube_reduce_kernel left in t_eq.  Reference r = ref[p] outside [0, P) or in another dice group (group NULL: the identity): NaN, NaN.
template <int NT>
__global__ __launch_bounds__(NT) void ro_cube_pair_kernel(long long P, long long T, const int32_t *__restrict__ ref, const int32_t *__restrict__ group,
                                                          const double *__restrict__ t_eq, double *__restrict__ diff_mean,
                                                          double *__restrict__ diff_serr)
{
    static_assert(NT == 64, "one wave per position");
    const long long p = blockIdx.x;
    const int lane = threadIdx.x;
    const long long r = ref[p];
    const bool ok = r >= 0 && r < P && (group ? group[r] == group[p] : r == p);
    if (!ok) {                                             // (the same in every lane)
        if (lane == 0) {
            if (diff_mean) diff_mean[p] = __builtin_nan("");
            if (diff_serr) diff_serr[p] = __builtin_nan("");
        }
        return;
    }
    const long long bp = p * T, br = r * T;
    double s = 0.0;
    for (long long i = lane; i < T; i += 64) s = __dadd_rn(s, __dsub_rn(t_eq[bp + i], t_eq[br + i]));
    const double m = cube_wave_sum(s) / (double)T;
    double q = 0.0;
    for (long long i = lane; i < T; i += 64) {
        const double d = __dsub_rn(__dsub_rn(t_eq[bp + i], t_eq[br + i]), m);
        q = __dadd_rn(q, __dmul_rn(d, d));
    }
    q = cube_wave_sum(q);
    if (lane == 0) {
        if (diff_mean) diff_mean[p] = m;
        if (diff_serr) diff_serr[p] = T > 1 ? sqrt(q / ((double)T * (double)(T - 1))) : 0.0;
    }
}

// ---- match play (bg_match.h): the cube's init and turn with a match score's conditions and thresholds; a trial's worth as an MWC ------
using bg::match::Table;

// the fields of a position's word
__device__ __forceinline__ uint32_t match_away(uint32_t word, int side) { return (word >> (side ? 8 : 0)) & 0xFFu; }
__device__ __forceinline__ uint32_t match_state(uint32_t word) { return (word >> 16) & 3u; }

// after(a1, a2, state) of bg_match.h: the MWC of the side needing a1.  a1, a2 <= M whenever the table is read.
__device__ __forceinline__ double match_after(long long a1, long long a2, uint32_t state, const Table &tab)
{
    if (a1 <= 0) return 1.0;
    if (a2 <= 0) return 0.0;
    if (state != 0u && a2 == 1) return tab.met_pc[a1 - 1];
    if (state != 0u && a1 == 1) return __dsub_rn(1.0, tab.met_pc[a2 - 1]);
    return tab.met[(a1 - 1) * tab.M + (a2 - 1)];
}

// cube_offer under a match: no decision in the Crawford game or on a dead cube (c >= the roller's away: the trial is marked); else the
// table's entry for (state, c, roller's away, opponent's away) in the place of the call's double_at and pass_at.  -> the record changed
__device__ __forceinline__ bool match_offer(Trial &t, int mover, double mean, uint32_t k, const Rule &r, const Table &tab, uint32_t word)
{
    const uint32_t owner = t.info & cube::INFO_OWNER;
    if (t.dropped >= 0 || t.value >= r.max_cube || !(owner == 0u || owner == (uint32_t)mover + 1u)) return false;
    const uint32_t st = match_state(word);
    if (st == 1u) return false;
    const uint32_t a = match_away(word, mover), b = match_away(word, mover ^ 1);
    if (t.value >= a) {
        if (t.spare & match::TRIAL_DEAD) return false;
        t.spare |= match::TRIAL_DEAD;
        return true;
    }
    const int level = __ffs((int)t.value) - 1;         // (t.value < a <= M: level < levels)
    const double2 th = tab.thr[(((long long)(st ? 1 : 0) * tab.levels + level) * tab.M + (a - 1u)) * tab.M + (b - 1u)];
    const double w = mover ? 1.0 - mean : mean;
    if (!(th.x <= w && w <= r.too_good_at)) return false;
    const uint32_t opp = 2u - (uint32_t)mover;
    if (w > th.y) {
        t.dropped = (int32_t)k;
        t.info |= opp << cube::INFO_PASSED_SHIFT;
    } else {
        t.value *= 2u;
        t.info = ((t.info & ~cube::INFO_OWNER) | opp) + (1u << cube::INFO_TURNS_SHIFT);
    }
    return true;
}

// thread per position: the caller's score tables into one word each; away outside 1 .. M, a state outside 0 .. 2, or a state that does
// not go with the score (1 and 2 iff a side is 1-away) sets err_bit in the intake word, and the word is that of a Crawford game at 1-1
template <int NT>
__global__ __launch_bounds__(NT) void ro_match_intake_kernel(long long P, int M, const int32_t *__restrict__ d_away1,
                                                             const int32_t *__restrict__ d_away2, const int32_t *__restrict__ d_state,
                                                             uint32_t *__restrict__ words, unsigned long long *err, unsigned long long err_bit)
{
    const long long p = (long long)blockIdx.x * NT + threadIdx.x;
    if (p >= P) return;
    const int32_t a1 = d_away1[p], a2 = d_away2[p], st = d_state[p];
    bool bad = a1 < 1 || a1 > M || a2 < 1 || a2 > M || st < 0 || st > 2;
    if (!bad) bad = ((a1 < a2 ? a1 : a2) == 1) != (st != 0);
    if (bad) atomicOr(err, err_bit);
    words[p] = bad ? (1u | 1u << 8 | 1u << 16) : ((uint32_t)a1 | (uint32_t)a2 << 8 | (uint32_t)st << 16);
}

// ro_cube_init_kernel under a match
template <int NT>
__global__ __launch_bounds__(NT) void ro_match_init_kernel(long long N, long long T, int rotate, const uint4 *__restrict__ pos_rows,
                                                           const uint32_t *__restrict__ start, long long P, const double *__restrict__ mean0,
                                                           Rule rule, Table tab, const uint32_t *__restrict__ words, Trial *__restrict__ trials)
{
    const long long jl = (long long)blockIdx.x * NT + threadIdx.x;
    if (jl >= N) return;
    const long long pi = jl / T;
    Trial t{start[pi], -1, start[P + pi], 0u};
    if (rotate && !rule.hold_turn0) {
        const uint4 a = pos_rows[2 * pi], b = pos_rows[2 * pi + 1];
        const uint32_t p[8] = {a.x & ~TURN_BIT, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        if (!over_code(p)) match_offer(t, (a.x & TURN_BIT) ? 1 : 0, mean0[pi], 0u, rule, tab, words[pi]);
    }
    *reinterpret_cast<uint4 *>(trials + jl) = make_uint4(t.value, (uint32_t)t.dropped, t.info, t.spare);
}

// ro_cube_turn_kernel under a match: trial j belongs to position j / T
template <int NT>
__global__ __launch_bounds__(NT) void ro_match_turn_kernel(long long L, uint32_t T, const uint32_t *__restrict__ meta,
                                                           const uint32_t *__restrict__ ply, const uint32_t *__restrict__ lane_trial,
                                                           const float *__restrict__ f, Rule rule, Table tab, const uint32_t *__restrict__ words,
                                                           Trial *__restrict__ trials, unsigned long long *__restrict__ ctr)
{
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    bool live = false, after = false;
    if (g < L) {
        const uint32_t m = meta[g], j = lane_trial[g];
        live = !(m & cube::LANE_FINISHED) && j != cube::LANE_NONE;
        if (live) {
            const uint4 w = *reinterpret_cast<const uint4 *>(trials + j);
            Trial t{w.x, (int32_t)w.y, w.z, w.w};
            const uint32_t k = ply[g];
            if (t.dropped < 0 && !(rule.hold_turn0 && k == 0u) &&
                match_offer(t, (int)(m & 1u), cube_pre_mean(f + g * cube::ROLLS), k, rule, tab, words[j / T]))
                *reinterpret_cast<uint4 *>(trials + j) = make_uint4(t.value, (uint32_t)t.dropped, t.info, t.spare);
            after = t.dropped >= 0;
        }
    }
    const unsigned long long nl = (unsigned long long)__popcll(__ballot(live)), na = (unsigned long long)__popcll(__ballot(after));
    if ((threadIdx.x & 63) == 0) {
        if (nl) atomicAdd(&ctr[cube::CTR_TURNS], nl);
        if (na) atomicAdd(&ctr[cube::CTR_AFTER_DROP], na);
    }
}

// PLAYER1's MWC of a trial (bg_match.h); ended: +1 the trial ended the match for PLAYER1, -1 for PLAYER2, 0 neither (or truncated)
__device__ __forceinline__ double match_mwc(const Trial &t, float x, uint32_t word_t, uint32_t word_p, const Table &tab, int &ended)
{
    // (the compiler contracts a product and a sum into a fused multiply-add unless told otherwise, through __dmul_rn / __dadd_rn too,
    // which are a plain product and sum to it: the truncated payoff, the one place of the rule where that would change a bit, is
    // written with operators under this pragma)
#pragma clang fp contract(off)
    const long long c = (long long)t.value, a1 = (long long)match_away(word_p, 0), a2 = (long long)match_away(word_p, 1);
    const uint32_t st = match_state(word_p);
    long long r;
    if (t.dropped >= 0) r = ((t.info >> cube::INFO_PASSED_SHIFT) & 3u) == 2u ? c : -c;
    else {
        const int pts = (int)(word_t << (29 - cube::WORD_PTS_SHIFT)) >> 29;
        if (pts == 0) {
            ended = 0;
            const double xd = (double)x;
            const double won = xd * match_after(a1 - c, a2, st, tab), lost = (1.0 - xd) * match_after(a1, a2 - c, st, tab);
            return won + lost;                         // (dadd(dmul(x, .), dmul(dsub(1, x), .)): three roundings, by the pragma above)
        }
        r = c * (long long)pts;
    }
    const long long b1 = a1 - (r > 0 ? r : 0), b2 = a2 - (r < 0 ? -r : 0);
    ended = b1 <= 0 ? 1 : (b2 <= 0 ? -1 : 0);
    return match_after(b1, b2, st, tab);
}

// ro_cube_reduce_kernel's two passes and butterfly on the trials' MWC.  counts[p][3]: trials that ended the match for PLAYER1, for
// PLAYER2, trials in which some decision was withheld by a dead cube.
template <int NT>
__global__ __launch_bounds__(NT) void ro_match_reduce_kernel(long long T, const float *__restrict__ t_val, const uint32_t *__restrict__ t_turns,
                                                             const Trial *__restrict__ trials, Table tab, const uint32_t *__restrict__ words,
                                                             double *__restrict__ t_mwc, double *__restrict__ mean, double *__restrict__ serr,
                                                             int64_t *__restrict__ counts, double *__restrict__ o_mwc)
{
    // (no product is contracted with a sum in here: the sum of squares is the chain of rounded products and sums a host restates)
#pragma clang fp contract(off)
    static_assert(NT == 64, "one wave per position");
    const long long p = blockIdx.x, base = p * T;
    const int lane = threadIdx.x;
    const uint32_t word_p = words[p];
    double s = 0.0;
    unsigned long long c[3] = {0ull, 0ull, 0ull};
    for (long long i = lane; i < T; i += 64) {
        const uint4 w = *reinterpret_cast<const uint4 *>(trials + base + i);
        const Trial t{w.x, (int32_t)w.y, w.z, w.w};
        int ended;
        const double e = match_mwc(t, t_val[base + i], t_turns[base + i], word_p, tab, ended);
        s = __dadd_rn(s, e);
        c[0] += ended > 0 ? 1ull : 0ull;
        c[1] += ended < 0 ? 1ull : 0ull;
        c[2] += (t.spare & match::TRIAL_DEAD) ? 1ull : 0ull;
        t_mwc[base + i] = e;
        if (o_mwc) o_mwc[base + i] = e;
    }
    const double m = cube_wave_sum(s) / (double)T;
    double q = 0.0;
    for (long long i = lane; i < T; i += 64) {
        const uint4 w = *reinterpret_cast<const uint4 *>(trials + base + i);
        const Trial t{w.x, (int32_t)w.y, w.z, w.w};
        int ended;
        const double d = match_mwc(t, t_val[base + i], t_turns[base + i], word_p, tab, ended) - m;
        const double dd = d * d;
        q = q + dd;
    }
    q = cube_wave_sum(q);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = cube_wave_sum_u64(c[k]);
    if (lane == 0) {
        if (mean) mean[p] = m;
        if (serr) serr[p] = T > 1 ? sqrt(q / ((double)T * (double)(T - 1))) : 0.0;
        if (counts) {
#pragma unroll
            for (int k = 0; k < 3; ++k) counts[p * 3 + k] = (int64_t)c[k];
        }
    }
}

}  // namespace

// ---- the launches (bg_cube.h) ---------------------------------------------------------------------------------------------------------
namespace bg {
namespace cube {
static dim3 grid1(long long n, int bs) { return dim3((unsigned)((n + bs - 1) / bs)); }

void intake(hipStream_t s, long long P, const int32_t *d_value, const int32_t *d_owner, uint32_t *start, unsigned long long *err_word,
            unsigned long long err_bit)
{
    hipLaunchKernelGGL(ro_cube_intake_kernel<128>, grid1(P, 128), dim3(128), 0, s, P, d_value, d_owner, start, err_word, err_bit);
}
void init(hipStream_t s, long long N, long long T, int rotate, const uint4 *pos_rows, const uint32_t *start, long long P,
          const double *mean0, Rule rule, Trial *trials)
{
    hipLaunchKernelGGL(ro_cube_init_kernel<CUBE_NT>, grid1(N, CUBE_NT), dim3(CUBE_NT), 0, s, N, T, rotate, pos_rows, start, P, mean0, rule, trials);
}
void turn(hipStream_t s, long long L, const uint32_t *meta, const uint32_t *ply, const uint32_t *lane_trial, const float *f, Rule rule,
          Trial *trials, unsigned long long *ctr)
{
    hipLaunchKernelGGL(ro_cube_turn_kernel<CUBE_NT>, grid1(L, CUBE_NT), dim3(CUBE_NT), 0, s, L, meta, ply, lane_trial, f, rule, trials, ctr);
}
void reduce(hipStream_t s, long long P, long long T, const float *t_val, const uint32_t *t_turns, const Trial *trials, Rule rule,
            double *t_eq, double *mean, double *serr, int64_t *counts, double *o_eq, int32_t *o_cube, int32_t *o_dropped)
{
    hipLaunchKernelGGL(ro_cube_reduce_kernel<64>, dim3((unsigned)P), dim3(64), 0, s, T, t_val, t_turns, trials, rule, t_eq, mean, serr, counts,
                       o_eq, o_cube, o_dropped);
}
void paired(hipStream_t s, long long P, long long T, const int32_t *ref, const int32_t *group, const double *t_eq, double *diff_mean,
            double *diff_serr)
{
    hipLaunchKernelGGL(ro_cube_pair_kernel<64>, dim3((unsigned)P), dim3(64), 0, s, P, T, ref, group, t_eq, diff_mean, diff_serr);
}

}  // namespace cube

// ---- the launches (bg_match.h) --------------------------------------------------------------------------------------------------------
namespace match {
static dim3 grid1(long long n, int bs) { return dim3((unsigned)((n + bs - 1) / bs)); }

void intake(hipStream_t s, long long P, int M, const int32_t *d_away1, const int32_t *d_away2, const int32_t *d_state, uint32_t *words,
            unsigned long long *err_word, unsigned long long err_bit)
{
    hipLaunchKernelGGL(ro_match_intake_kernel<128>, grid1(P, 128), dim3(128), 0, s, P, M, d_away1, d_away2, d_state, words, err_word, err_bit);
}
void init(hipStream_t s, long long N, long long T, int rotate, const uint4 *pos_rows, const uint32_t *start, long long P, const double *mean0,
          cube::Rule rule, Table tab, const uint32_t *words, cube::Trial *trials)
{
    hipLaunchKernelGGL(ro_match_init_kernel<CUBE_NT>, grid1(N, CUBE_NT), dim3(CUBE_NT), 0, s, N, T, rotate, pos_rows, start, P, mean0, rule, tab,
                       words, trials);
}
void turn(hipStream_t s, long long L, long long T, const uint32_t *meta, const uint32_t *ply, const uint32_t *lane_trial, const float *f,
          cube::Rule rule, Table tab, const uint32_t *words, cube::Trial *trials, unsigned long long *ctr)
{
    hipLaunchKernelGGL(ro_match_turn_kernel<CUBE_NT>, grid1(L, CUBE_NT), dim3(CUBE_NT), 0, s, L, (uint32_t)T, meta, ply, lane_trial, f, rule, tab,
                       words, trials, ctr);
}
void reduce(hipStream_t s, long long P, long long T, const float *t_val, const uint32_t *t_turns, const cube::Trial *trials, Table tab,
            const uint32_t *words, double *t_mwc, double *mean, double *serr, int64_t *counts, double *o_mwc)
{
    hipLaunchKernelGGL(ro_match_reduce_kernel<64>, dim3((unsigned)P), dim3(64), 0, s, T, t_val, t_turns, trials, tab, words, t_mwc, mean, serr,
                       counts, o_mwc);
}

}  // namespace match
}  // namespace bg
