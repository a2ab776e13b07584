// bg_filter.h -- kernels of the filtered 2-ply search step (bgamd_env_step_search_filtered, include/bgamd.h): the search of bg_search.h
// with GNU Backgammon's move filter -- a candidate is searched only while its 1-ply value lies within a margin of the best one -- and
// without any search for a lane that keeps a single candidate.  Included by bgamd.hip inside its anonymous namespace, after every other
// kernel header.
//
//   stage A  as the search's: roots, expansion, incremental value net on the env's own lanes, rows grouped by game
//   stage B  flt_select (wave per game) : srch_select's ranking with the margin rule; kept[g], and skept[g] = kept[g] when the lane is
//                                         searched (kept >= 2), else 0
//            srch_scan x 2, srch_emit   : the kept candidates as one list (candidate j = koff[g] + rank), as the search's
//            flt_vmap (lane per game)   : the SEARCHED candidates as a second compact list, jv = soff[g] + rank -> j: a singleton lane has
//                                         no entry, so it costs no virtual root
//   stage C  flt_fanout: virtual root v = (searched candidate v / 21, opponent roll v % 21); scoring passes and srch_collect as the search's,
//            over the list's real length
//   stage D  flt_reduce (lane per game) : a singleton's candidate is the choice with V2 = v1; a searched lane as srch_reduce
//   info     flt_info (one workgroup)   : the four counts of bgamd_env_search_info, for either kind of search step
// The kernels are templates: their code is emitted behind the other kernels', whose addresses stay where they were.
#pragma once

// srch_select_kernel with the margin: a distinct row of rank r (the number of distinct rows that beat it in the (v1 for the mover,
// smaller key) order) is kept iff r < k_lim and d <= margin, d = one fp32 subtraction from rank 0's v1 on the mover's side (never
// negative); rank 0 is always kept.  d does not fall as the rank grows, so the kept rows are ranks 0 .. kept - 1 and a row's rank is its
// slot.  rank[pos] = rank, -1 (distinct, not kept) or -2 (copy).  The same two passes and wave-uniform inner loops.
template <int W>
__global__ __launch_bounds__(W) void flt_select_kernel(long long n, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                                                       const uint32_t *__restrict__ grp, const uint4 *__restrict__ rows,
                                                       const uint2 *__restrict__ info, const float *__restrict__ values, uint32_t k_lim,
                                                       float margin, int32_t *__restrict__ rank, uint32_t *__restrict__ kept,
                                                       uint32_t *__restrict__ skept)
{
    const long long g = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t m = cnt[g], base = off[g];
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
    uint32_t n_kept = 0;
    for (uint32_t i0 = 0; i0 < m; i0 += W) {               // (wave-uniform trip count: the barriers below are safe)
        const uint32_t i = i0 + lane;
        const bool mine = i < m && rank[base + i] != -2;
        int32_t r = -2;
        bool keep = false;
        if (mine) {
            const uint32_t ri = grp[base + i];
            const SrchCand ci = srch_cand(rows, info, values, ri);
            const int mover = (rows[2 * (long long)ri].x & TURN_BIT) ? 1 : 0;
            const unsigned long long pi = srch_pack(ci.v, ci.key, mover);
            unsigned long long pb = 0ull;                   // rank 0 of the game: the largest pack (this row's own takes part)
            float vb = ci.v;
            uint32_t better = 0;
            for (uint32_t j = 0; j < m; ++j) {
                if (rank[base + j] == -2) continue;
                const SrchCand cj = srch_cand(rows, info, values, grp[base + j]);
                const unsigned long long pj = srch_pack(cj.v, cj.key, mover);
                better += pj > pi ? 1u : 0u;
                if (pj > pb) { pb = pj; vb = cj.v; }
            }
            const float d = mover ? ci.v - vb : vb - ci.v;
            keep = better < k_lim && (better == 0 || d <= margin);
            r = keep ? (int32_t)better : -1;
        }
        n_kept += (uint32_t)__popcll(__ballot(keep));
        __syncthreads();                                   // every lane has read this round's flags before they change
        if (i < m) rank[base + i] = r;
        __syncthreads();
    }
    if (lane == 0) { kept[g] = n_kept; skept[g] = n_kept >= 2 ? n_kept : 0u; }
}

// the searched candidates: entry soff[g] + i of the compact list is candidate koff[g] + i, for the lanes with kept >= 2
template <int NT>
__global__ __launch_bounds__(NT) void flt_vmap_kernel(long long n, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ koff,
                                                      const uint32_t *__restrict__ soff, uint32_t *__restrict__ vmap)
{
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    if (g >= n) return;
    const uint32_t k = kept[g];
    if (k < 2) return;
    const uint32_t j0 = koff[g], s0 = soff[g];
    for (uint32_t i = 0; i < k; ++i) vmap[s0 + i] = j0 + i;
}

// srch_fanout_kernel over the searched list: virtual lane l of a chunk = virtual root v = v0 + l = (entry v / 21, opponent roll v % 21).
// Past the list, or under a terminal candidate: a finished lane (no roots, no rows).
template <int NT>
__global__ __launch_bounds__(NT) void flt_fanout_kernel(EnvView e, long long v0, const uint32_t *__restrict__ total,
                                                        const uint32_t *__restrict__ vmap, const uint4 *__restrict__ c_rows,
                                                        const uint32_t *__restrict__ c_key)
{
    const long long l = (long long)blockIdx.x * NT + threadIdx.x;
    if (l >= e.n) return;
    const long long v = v0 + l, jv = v / SRCH_ROLLS;
    uint32_t p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t meta = META_FINISHED;
    if (jv < (long long)*total) {
        const long long j = vmap[jv];
        if (!(c_key[j] & 0x80000000u)) {
            const uint4 a = c_rows[2 * j], b = c_rows[2 * j + 1];
            p[0] = a.x & ~TURN_BIT; p[1] = a.y; p[2] = a.z; p[3] = a.w; p[4] = b.x; p[5] = b.y; p[6] = b.z; p[7] = b.w;
            const int opp = (a.x & TURN_BIT) ? 0 : 1;
            int d1, d2;
            srch_roll((int)(v % SRCH_ROLLS), d1, d2);
            meta = meta_pack(opp, d1, d2, false);
        }
    }
    store_planes(e, l, p);
    e.meta[l] = meta; e.ply[l] = 0; e.episode[l] = 0; e.flags[l] = 0;
}

// srch_reduce_kernel with the singleton path.  A lane with one kept candidate was not searched: V2 = v1 and the candidate is the choice.
// A searched lane: V2 with srch_reduce_kernel's arithmetic (repeated here, not shared: that kernel's code stays as it is) from the roll
// values of its entries in the searched list, arg-best for the mover (ties: the smaller key).  The winner into best[g] as (ordered value
// bits, ~key) -- what apply_kernel decodes -- and the scratch env's error bits into the env's.
template <int NT>
__global__ __launch_bounds__(NT) void flt_reduce_kernel(long long n, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ koff,
                                                        const uint32_t *__restrict__ soff, const uint4 *__restrict__ c_rows,
                                                        const uint32_t *__restrict__ c_key, const float *__restrict__ c_v1,
                                                        const float *__restrict__ rval, float *__restrict__ c_v2,
                                                        unsigned long long *__restrict__ best, unsigned long long *__restrict__ err,
                                                        unsigned long long *__restrict__ scratch_err)
{
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    if (g == 0 && scratch_err) {
        const unsigned long long x = *scratch_err;
        if (x) { atomicOr(err, x); *scratch_err = 0ull; }
    }
    if (g >= n) return;
    const uint32_t k = kept[g], j0 = koff[g], s0 = soff[g];
    unsigned long long b = 0ull;
    for (uint32_t i = 0; i < k; ++i) {
        const long long j = (long long)j0 + i;
        const uint32_t key = c_key[j];
        const int mover = (c_rows[2 * j].x & TURN_BIT) ? 1 : 0;
        float v2;
        if (k < 2 || (key & 0x80000000u)) v2 = c_v1[j];
        else {
            float sd = 0.0f, so = 0.0f;                     // (sum over the doubles + 2 x sum over the other rolls) / 36, each in roll order
            const float *r = rval + ((long long)s0 + i) * SRCH_ROLLS;
#pragma unroll
            for (int idx = 0, a = 1; a <= 6; ++a)
#pragma unroll
                for (int d = a; d <= 6; ++d, ++idx) {
                    if (a == d) sd += r[idx];
                    else so += r[idx];
                }
            v2 = (sd + 2.0f * so) * (1.0f / 36.0f);
        }
        c_v2[j] = v2;
        const unsigned long long pk = srch_pack(v2, key & 0x7FFFFFFFu, mover);
        b = pk > b ? pk : b;
    }
    best[g] = b;
}

// bgamd_env_search_info.  One workgroup; integer sums, so the order does not matter.  out[0] lanes with a kept candidate, [1] lanes
// searched (kept >= min_searched: 2 after a filtered step, 1 after a plain one), [2] kept candidates, [3] virtual roots scored = 21 x
// the non-terminal candidates of the searched lanes.
template <int NT>
__global__ __launch_bounds__(NT) void flt_info_kernel(long long n, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ koff,
                                                      const uint32_t *__restrict__ c_key, uint32_t min_searched,
                                                      unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long s_sum[4];
    if (threadIdx.x < 4) s_sum[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long v[4] = {0ull, 0ull, 0ull, 0ull};
    for (long long g = threadIdx.x; g < n; g += NT) {
        const uint32_t k = kept[g], j0 = koff[g];
        if (k == 0) continue;
        v[0] += 1ull;
        v[2] += k;
        if (k < min_searched) continue;
        v[1] += 1ull;
        for (uint32_t i = 0; i < k; ++i) v[3] += (c_key[(long long)j0 + i] & 0x80000000u) ? 0ull : (unsigned long long)SRCH_ROLLS;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (v[q]) atomicAdd(&s_sum[q], v[q]);
    __syncthreads();
    if (threadIdx.x < 4) out[threadIdx.x] = s_sum[threadIdx.x];
}
