// bg_analysis.h -- kernels of the move analysis (bgamd_env_analyze_moves, include/bgamd.h): a played afterstate per lane judged against
// the 2-ply search.  Included by bgamd.hip inside its anonymous namespace, after every other kernel header.
//
//   stage A  as the search's (bg_search.h): roots, expansion, incremental value net on the env's own lanes, rows grouped by game
//   match    ana_match (wave per game)  : the played state packed to planes and looked up among the game's rows -> status, and the
//                                         played afterstate's distinct representative (of copies: the smallest key)
//   stage B  ana_select (wave per game) : srch_select's ranking; kept = the top K and the played row, wherever it ranks (its slot in
//                                         the list is its rank, or K when it ranks outside); distinct count, rank1
//            srch_scan, srch_emit       : as the search's
//   stage C  as the search's: srch_fanout, the scratch env's scoring passes, srch_collect
//   stage D  ana_reduce (lane per game) : V2 as srch_reduce forms it, best over the kept set, rank2, error, the best row
//            ana_summary (one workgroup): the twelve numbers in a fixed order
// Nothing is applied.  The kernels are templates: their code is emitted behind the other kernels', whose addresses stay where they were
// (where the step kernels lie decides ~1 % of the greedy step: DESIGN 6d).
#pragma once

constexpr uint32_t ANA_NONE = 0xFFFFFFFFu;
constexpr int ANA_SUMMARY = 12;
constexpr int ANA_SUM_NT = 1024;
enum { ANA_OK = 0, ANA_IDLE = 1, ANA_NO_MOVE = 2, ANA_NOT_FOUND = 3 };

// per-lane results [n] (best: [n][2] rows), and what the stages hand one another: ppos = the played row's place in grp (ANA_NONE: none),
// pslot = its place in the lane's kept list
struct AnaView {
    int32_t *status, *distinct, *rank1, *rank2;
    float *v1_played, *v1_best, *v2_played, *v2_best, *error;
    uint4 *best;
    uint32_t *ppos, *pslot;
};

__device__ __forceinline__ unsigned long long ana_wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

// One wave per game.  Every lane packs the played state (one wave-uniform address per load); lane i compares rows i, i + 64, ... of the
// game by planes; the match with the smallest key is the representative srch_select / ana_select keep of that position.  A state that
// cannot be packed (|count| > 15) matches nothing.  The lane takes part as lane_derive decides for the greedy step's roots.
template <int W>
__global__ __launch_bounds__(W) void ana_match_kernel(EnvView e, int flags, const int32_t *__restrict__ played,
                                                      const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                                                      const uint32_t *__restrict__ grp, const uint4 *__restrict__ rows,
                                                      const uint2 *__restrict__ info, AnaView a)
{
    const long long g = blockIdx.x;
    const int lane = threadIdx.x;
    int32_t s[28];
#pragma unroll
    for (int q = 0; q < 28; ++q) s[q] = played[g * 28 + q];
    uint32_t p[8];
    int bad = 0;
    planes_from_state28(s, p, &bad);
    const uint32_t meta = e.meta[g];
    const int turn = meta & 1;
    const bool live = !(meta & META_FINISHED) && !((flags & BGAMD_ONLY_P1) && turn != 0) && !((flags & BGAMD_ONLY_P2) && turn != 1);
    const uint32_t m = cnt[g], base = off[g];
    unsigned long long found = ~0ull;                       // key << 32 | place in the game's rows
    if (live && !bad)
        for (uint32_t i = lane; i < m; i += W) {
            const uint32_t row = grp[base + i];
            const uint4 x = rows[2 * (long long)row], y = rows[2 * (long long)row + 1];
            const uint32_t q[8] = {x.x & ~TURN_BIT, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
            const unsigned long long mine = ((unsigned long long)(info[row].y & 0x7FFFFFFFu) << 32) | i;
            if (srch_same(p, q) && mine < found) found = mine;
        }
    found = ana_wave_min_u64(found);
    if (lane == 0) {
        const bool hit = found != ~0ull;
        a.status[g] = !live ? ANA_IDLE : (m == 0 ? ANA_NO_MOVE : (hit ? ANA_OK : ANA_NOT_FOUND));
        a.ppos[g] = hit ? base + (uint32_t)found : ANA_NONE;
    }
}

// srch_select_kernel with the played row forced in: rank[pos] = rank (< k_lim), k_lim for the played row when it ranks outside, -1
// (distinct, not kept) or -2 (copy); kept[g] = min(k_lim, distinct) + 1 if the played row ranks outside.  The same two passes and the
// same wave-uniform inner loops.  Also: distinct[g], rank1[g] = the played row's true rank (-1: no played row), pslot[g].
template <int W>
__global__ __launch_bounds__(W) void ana_select_kernel(long long n, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                                                       const uint32_t *__restrict__ grp, const uint4 *__restrict__ rows,
                                                       const uint2 *__restrict__ info, const float *__restrict__ values, uint32_t k_lim,
                                                       int32_t *__restrict__ rank, uint32_t *__restrict__ kept, AnaView a)
{
    const long long g = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t m = cnt[g], base = off[g], pp = a.ppos[g];
    for (uint32_t i = lane; i < m; i += W) {
        const SrchCand ci = srch_cand(rows, info, values, grp[base + i]);
        bool copy = false;
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t rj = grp[base + j];
            copy |= (info[rj].y & 0x7FFFFFFFu) < ci.key && srch_same(ci.p, srch_cand(rows, info, values, rj).p);
        }
        rank[base + i] = copy ? -2 : 0;
    }
    __syncthreads();
    uint32_t distinct = 0, my_slot = ANA_NONE;
    int32_t my_rank1 = -1;
    bool outside = false;
    for (uint32_t i0 = 0; i0 < m; i0 += W) {               // (wave-uniform trip count: the barriers below are safe)
        const uint32_t i = i0 + lane;
        const bool mine = i < m && rank[base + i] != -2;
        int32_t r = -2;
        if (mine) {
            const uint32_t ri = grp[base + i];
            const SrchCand ci = srch_cand(rows, info, values, ri);
            const int mover = (rows[2 * (long long)ri].x & TURN_BIT) ? 1 : 0;
            const unsigned long long pi = srch_pack(ci.v, ci.key, mover);
            uint32_t better = 0;
            for (uint32_t j = 0; j < m; ++j) {
                if (rank[base + j] == -2) continue;
                const SrchCand cj = srch_cand(rows, info, values, grp[base + j]);
                better += srch_pack(cj.v, cj.key, mover) > pi ? 1u : 0u;
            }
            r = better < k_lim ? (int32_t)better : -1;
            if (base + i == pp) {
                my_rank1 = (int32_t)better;
                my_slot = better < k_lim ? better : k_lim;
                r = (int32_t)my_slot;
            }
        }
        distinct += (uint32_t)__popcll(__ballot(mine));
        __syncthreads();                                   // every lane has read this round's flags before they change
        if (i < m) rank[base + i] = r;
        __syncthreads();
    }
    const unsigned long long who = __ballot(my_slot != ANA_NONE);
    outside = __ballot(my_slot != ANA_NONE && (uint32_t)my_rank1 >= k_lim) != 0ull;
    if (who ? lane == __ffsll((long long)who) - 1 : lane == 0) { a.rank1[g] = my_rank1; a.pslot[g] = my_slot; }
    if (lane == 0) {
        kept[g] = (distinct < k_lim ? distinct : k_lim) + (outside ? 1u : 0u);
        a.distinct[g] = (int32_t)distinct;
    }
}

// Lane per game: V2 of every kept candidate with srch_reduce_kernel's arithmetic (repeated here, not shared: that kernel's code stays as
// it is), the best for the mover (ties: the smaller key), the played candidate's place in that order, the error; the scratch env's
// error bits into the env's.  Status ANA_NOT_FOUND: the kept list is the top K alone and only the best side is filled.
template <int NT>
__global__ __launch_bounds__(NT) void ana_reduce_kernel(long long n, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ koff,
                                                        const uint4 *__restrict__ c_rows, const uint32_t *__restrict__ c_key,
                                                        const float *__restrict__ c_v1, const float *__restrict__ rval,
                                                        float *__restrict__ c_v2, AnaView a, unsigned long long *__restrict__ err,
                                                        unsigned long long *__restrict__ scratch_err)
{
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    if (g == 0 && scratch_err) {
        const unsigned long long x = *scratch_err;
        if (x) { atomicOr(err, x); *scratch_err = 0ull; }
    }
    if (g >= n) return;
    const int st = a.status[g];
    const uint32_t k = kept[g], j0 = koff[g], ps = a.pslot[g];
    unsigned long long b = 0ull, pp = 0ull;
    uint32_t bi = 0;
    float v2b = 0.0f, v2p = 0.0f;
    int mover = 0;
    for (uint32_t i = 0; i < k; ++i) {
        const long long j = (long long)j0 + i;
        const uint32_t key = c_key[j];
        mover = (c_rows[2 * j].x & TURN_BIT) ? 1 : 0;
        float v2;
        if (key & 0x80000000u) v2 = c_v1[j];
        else {
            float sd = 0.0f, so = 0.0f;                     // (sum over the doubles + 2 x sum over the other rolls) / 36, each in roll order
            const float *r = rval + j * SRCH_ROLLS;
#pragma unroll
            for (int idx = 0, x = 1; x <= 6; ++x)
#pragma unroll
                for (int d = x; d <= 6; ++d, ++idx) {
                    if (x == d) sd += r[idx];
                    else so += r[idx];
                }
            v2 = (sd + 2.0f * so) * (1.0f / 36.0f);
        }
        c_v2[j] = v2;
        const unsigned long long pk = srch_pack(v2, key & 0x7FFFFFFFu, mover);
        if (i == ps) { pp = pk; v2p = v2; }
        if (pk > b) { b = pk; bi = i; v2b = v2; }
    }
    const bool ok = st == ANA_OK, best_side = (ok || st == ANA_NOT_FOUND) && k > 0;
    int32_t r2 = 0;
    if (ok)
        for (uint32_t i = 0; i < k; ++i) {
            const long long j = (long long)j0 + i;
            r2 += srch_pack(c_v2[j], c_key[j] & 0x7FFFFFFFu, mover) > pp ? 1 : 0;
        }
    uint4 r0 = make_uint4(0u, 0u, 0u, 0u), r1 = r0;
    if (best_side) {
        r0 = c_rows[2 * ((long long)j0 + bi)]; r1 = c_rows[2 * ((long long)j0 + bi) + 1];
        r0.x &= ~TURN_BIT;
    }
    a.best[2 * g] = r0; a.best[2 * g + 1] = r1;
    a.rank1[g] = ok ? a.rank1[g] : (st == ANA_NOT_FOUND ? -1 : 0);
    a.rank2[g] = ok ? r2 : (st == ANA_NOT_FOUND ? -1 : 0);
    a.v1_best[g] = best_side ? c_v1[j0] : 0.0f;
    a.v2_best[g] = best_side ? v2b : 0.0f;
    a.v1_played[g] = ok ? c_v1[(long long)j0 + ps] : 0.0f;
    a.v2_played[g] = ok ? v2p : 0.0f;
    a.error[g] = ok ? (mover ? v2p - v2b : v2b - v2p) : 0.0f;
}

// One workgroup.  Thread t takes lanes t, t + NT, ... in that order; the threads' partial results meet in a wave butterfly and then, wave
// by wave, in thread 0: a fixed order whatever the device does, and a side's numbers do not depend on the other side's lanes.
// out[0..4] PLAYER1, [5..9] PLAYER2: analysed, unforced, mistakes, sum of (double) error, largest error; [10] no move, [11] not found.
template <int NT>
__global__ __launch_bounds__(NT) void ana_summary_kernel(EnvView e, AnaView a, double *__restrict__ out)
{
    __shared__ double s_part[NT / 64][ANA_SUMMARY];
    double v[ANA_SUMMARY];
#pragma unroll
    for (int q = 0; q < ANA_SUMMARY; ++q) v[q] = 0.0;
    for (long long g = threadIdx.x; g < e.n; g += NT) {
        const int st = a.status[g];
        v[10] += st == ANA_NO_MOVE ? 1.0 : 0.0;
        v[11] += st == ANA_NOT_FOUND ? 1.0 : 0.0;
        if (st != ANA_OK) continue;
        const bool p2 = (e.meta[g] & 1u) != 0;
        const double er = (double)a.error[g], unf = a.distinct[g] >= 2 ? 1.0 : 0.0, mis = er > 0.0 ? 1.0 : 0.0;
#pragma unroll
        for (int side = 0; side < 2; ++side) {              // (both sides' slots by constant index: v stays in registers)
            const bool on = p2 == (side == 1);
            v[5 * side] += on ? 1.0 : 0.0;
            v[5 * side + 1] += on ? unf : 0.0;
            v[5 * side + 2] += on ? mis : 0.0;
            v[5 * side + 3] += on ? er : 0.0;
            v[5 * side + 4] = on && er > v[5 * side + 4] ? er : v[5 * side + 4];
        }
    }
#pragma unroll
    for (int q = 0; q < ANA_SUMMARY; ++q) {
        const bool is_max = q == 4 || q == 9;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double o = __shfl_xor(v[q], m, 64);
            v[q] = is_max ? (o > v[q] ? o : v[q]) : v[q] + o;
        }
    }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int q = 0; q < ANA_SUMMARY; ++q) s_part[threadIdx.x >> 6][q] = v[q];
    __syncthreads();
    if (threadIdx.x < ANA_SUMMARY) {
        const int q = threadIdx.x;
        const bool is_max = q == 4 || q == 9;
        double r = s_part[0][q];
        for (int w = 1; w < NT / 64; ++w) r = is_max ? (s_part[w][q] > r ? s_part[w][q] : r) : r + s_part[w][q];
        out[q] = r;
    }
}

// bgamd_env_analysis_read: the per-lane results into the caller's arrays (any may be NULL), the best row unpacked to 28 counts
template <int NT>
__global__ __launch_bounds__(NT) void ana_read_kernel(long long n, AnaView a, const double *__restrict__ summary, AnaView o,
                                                      int32_t *__restrict__ best28, double *__restrict__ o_summary)
{
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    if (g < ANA_SUMMARY && o_summary) o_summary[g] = summary[g];
    if (g >= n) return;
    if (o.status) o.status[g] = a.status[g];
    if (o.distinct) o.distinct[g] = a.distinct[g];
    if (o.rank1) o.rank1[g] = a.rank1[g];
    if (o.rank2) o.rank2[g] = a.rank2[g];
    if (o.v1_played) o.v1_played[g] = a.v1_played[g];
    if (o.v1_best) o.v1_best[g] = a.v1_best[g];
    if (o.v2_played) o.v2_played[g] = a.v2_played[g];
    if (o.v2_best) o.v2_best[g] = a.v2_best[g];
    if (o.error) o.error[g] = a.error[g];
    if (best28) {
        const uint4 x = a.best[2 * g], y = a.best[2 * g + 1];
        const uint32_t p[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
        int32_t s[28];
        state28_from_planes(p, s);
#pragma unroll
        for (int q = 0; q < 28; ++q) best28[g * 28 + q] = s[q];
    }
}
