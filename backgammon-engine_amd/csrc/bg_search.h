// bg_search.h -- kernels of the 2-ply expectimax step (bgamd_env_step_search, include/bgamd.h).  Included by bgamd.hip inside
// its anonymous namespace, after the staged greedy kernels.
//
//   stage A  the greedy step's roots, expansion and incremental value net on the env's own lanes (GreedyRun, no apply)
//   stage B  srch_count / srch_scan / srch_scatter : the step's rows (four arenas, no order) grouped by game
//            srch_select (wave per game)          : copies dropped, rank by (value for the mover, smaller key), top K kept
//            srch_scan, srch_emit                 : the kept candidates as one compact list (candidate j = koff[game] + rank)
//   stage C  per chunk of virtual lanes: srch_fanout writes (candidate, opponent roll) roots into the scratch env, the greedy
//            step's roots / expansion / value net score them there (GreedyRun, no apply), srch_collect decodes each lane's best
//            reply value (or the pass value from the root pass's hidden layer) into rval[v]
//   stage D  srch_reduce (lane per game): V2 in the fixed roll order, arg-best, the winner's key into sv.best -> apply_kernel
#pragma once

#include "bg_search_order.h"              // SRCH_ROLLS, srch_pack: shared with the 3-ply step's kernels, which are compiled apart
// (SRCH_NT = 256 threads per workgroup: bg_step_plan.h)

// the 21 unordered rolls in the fixed order (1,1), (1,2), ..., (1,6), (2,2), ..., (6,6)
__device__ __forceinline__ void srch_roll(int r, int &a, int &b)
{
    int x = 1, k = r;
    while (k >= 7 - x) { k -= 7 - x; ++x; }
    a = x; b = x + k;
}

// rows of the last step's arenas: arena k is rows [k bb, k bb + min(count_k, bb)) (bb == 0: one arena of cap_rows rows)
struct SrchRows {
    long long start[N_ARENAS], count[N_ARENAS], total;
};
__device__ __forceinline__ SrchRows srch_rows(const unsigned long long *__restrict__ tops, long long bb, long long cap_rows)
{
    SrchRows r;
    r.total = 0;
    const int na = bb > 0 ? N_ARENAS : 1;
    const long long cap_a = bb > 0 ? bb : cap_rows;
#pragma unroll
    for (int k = 0; k < N_ARENAS; ++k) {
        long long c = k < na ? (long long)tops[arena_counter(k)] : 0;
        c = c < cap_a ? c : cap_a;
        r.start[k] = (long long)k * bb; r.count[k] = c; r.total += c;
    }
    return r;
}
__device__ __forceinline__ long long srch_row_at(const SrchRows &r, long long i)
{
#pragma unroll
    for (int k = 0; k < N_ARENAS - 1; ++k) {
        if (i < r.count[k]) return r.start[k] + i;
        i -= r.count[k];
    }
    return r.start[N_ARENAS - 1] + i;
}

__global__ __launch_bounds__(SRCH_NT) void srch_count_kernel(const unsigned long long *__restrict__ tops, long long bb, long long cap_rows,
                                                             const uint2 *__restrict__ info, uint32_t *__restrict__ cnt)
{
    const SrchRows R = srch_rows(tops, bb, cap_rows);
    for (long long i = (long long)blockIdx.x * SRCH_NT + threadIdx.x; i < R.total; i += (long long)gridDim.x * SRCH_NT)
        atomicAdd(&cnt[info[srch_row_at(R, i)].x], 1u);
}

// exclusive scan of in[0, n) -> out[0, n], out[n] = total; *mx = max.  One workgroup of 1 024 threads (n is a lane count).
__global__ __launch_bounds__(1024) void srch_scan_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, long long n,
                                                         uint32_t *__restrict__ mx)
{
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_carry, s_max;
    if (threadIdx.x == 0) { s_carry = 0; s_max = 0; }
    uint32_t m = 0;
    for (long long b = 0; b < n; b += 1024) {
        const long long i = b + threadIdx.x;
        const uint32_t v = i < n ? in[i] : 0u;
        m = v > m ? v : m;
        uint32_t tot;
        const uint32_t ex = block_scan_256<16>(v, &tot, s_wave);      // (leads with a barrier: s_carry of the block before is in)
        const uint32_t carry = s_carry;
        if (i < n) out[i] = carry + ex;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = carry + tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) out[n] = s_carry;
    atomicMax(&s_max, m);
    __syncthreads();
    if (threadIdx.x == 0 && mx) *mx = s_max;
}

__global__ __launch_bounds__(SRCH_NT) void srch_scatter_kernel(const unsigned long long *__restrict__ tops, long long bb, long long cap_rows,
                                                               const uint2 *__restrict__ info, const uint32_t *__restrict__ off,
                                                               uint32_t *__restrict__ fill, uint32_t *__restrict__ grp)
{
    const SrchRows R = srch_rows(tops, bb, cap_rows);
    for (long long i = (long long)blockIdx.x * SRCH_NT + threadIdx.x; i < R.total; i += (long long)gridDim.x * SRCH_NT) {
        const long long row = srch_row_at(R, i);
        const uint32_t g = info[row].x;
        grp[off[g] + atomicAdd(&fill[g], 1u)] = (uint32_t)row;
    }
}

// one row of a game as the search sees it: planes (turn bit cleared), key, 1-ply value (exact outcome when the mover has won:
// over_code's test of the mover's side)
struct SrchCand {
    uint32_t p[8];
    uint32_t key;
    float v;
    bool term;
};
__device__ __forceinline__ SrchCand srch_cand(const uint4 *__restrict__ rows, const uint2 *__restrict__ info, const float *__restrict__ values,
                                              uint32_t row)
{
    SrchCand c;
    const uint4 a = rows[2 * (long long)row], b = rows[2 * (long long)row + 1];
    c.p[0] = a.x & ~TURN_BIT; c.p[1] = a.y; c.p[2] = a.z; c.p[3] = a.w; c.p[4] = b.x; c.p[5] = b.y; c.p[6] = b.z; c.p[7] = b.w;
    c.key = info[row].y & 0x7FFFFFFFu;
    // terminal = the MOVER has borne off its 15th checker (a position handed in with the other side already home is not)
    const int mover = (a.x & TURN_BIT) ? 1 : 0;
    const uint32_t off15 = mover ? (c.p[4] & c.p[5] & c.p[6] & c.p[7] & 1u) : (c.p[0] & c.p[1] & c.p[2] & c.p[3] & (1u << 25));
    c.term = off15 != 0;
    c.v = c.term ? (mover ? 0.0f : 1.0f) : values[row];
    return c;
}
__device__ __forceinline__ bool srch_same(const uint32_t (&x)[8], const uint32_t (&y)[8])
{
    uint32_t d = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) d |= x[k] ^ y[k];
    return d == 0;
}

// One 64-thread workgroup (one wave) per game.  Pass 1: a row is a copy when a row with a smaller key holds the same position
// (rank[] = -2, read back by the other lanes after the barrier).  Pass 2: the rank of a distinct row = the number of distinct rows
// that beat it; rank[pos] = rank (< k_lim), -1 (distinct, not kept) or -2 (copy); kept[g] = min(k_lim, distinct).
// O(m^2) per game over its m rows (~18 on average): the inner loops read wave-uniform addresses.
__global__ __launch_bounds__(64) void srch_select_kernel(long long n, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                                                         const uint32_t *__restrict__ grp, const uint4 *__restrict__ rows,
                                                         const uint2 *__restrict__ info, const float *__restrict__ values,
                                                         uint32_t k_lim, int32_t *__restrict__ rank, uint32_t *__restrict__ kept)
{
    const long long g = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t m = cnt[g], base = off[g];
    for (uint32_t i = lane; i < m; i += 64) {
        const SrchCand ci = srch_cand(rows, info, values, grp[base + i]);
        bool copy = false;
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t rj = grp[base + j];
            copy |= (info[rj].y & 0x7FFFFFFFu) < ci.key && srch_same(ci.p, srch_cand(rows, info, values, rj).p);
        }
        rank[base + i] = copy ? -2 : 0;
    }
    __syncthreads();
    uint32_t distinct = 0;
    for (uint32_t i0 = 0; i0 < m; i0 += 64) {               // (wave-uniform trip count: the barriers below are safe)
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
        }
        distinct += (uint32_t)__popcll(__ballot(mine));
        __syncthreads();                                   // every lane has read this round's flags before they change
        if (i < m) rank[base + i] = r;
        __syncthreads();
    }
    if (lane == 0) kept[g] = distinct < k_lim ? distinct : k_lim;
}

// the kept rows as candidates j = koff[g] + rank: row (mover's turn bit kept), key | terminal << 31, 1-ply value
__global__ __launch_bounds__(64) void srch_emit_kernel(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                                                       const uint32_t *__restrict__ grp, const uint4 *__restrict__ rows,
                                                       const uint2 *__restrict__ info, const float *__restrict__ values,
                                                       const int32_t *__restrict__ rank, const uint32_t *__restrict__ koff,
                                                       uint4 *__restrict__ c_rows, uint32_t *__restrict__ c_key, float *__restrict__ c_v1)
{
    const long long g = blockIdx.x;
    const uint32_t m = cnt[g], base = off[g], k0 = koff[g];
    for (uint32_t i = threadIdx.x; i < m; i += 64) {
        const int32_t r = rank[base + i];
        if (r < 0) continue;
        const uint32_t row = grp[base + i];
        const SrchCand c = srch_cand(rows, info, values, row);
        const long long j = (long long)k0 + r;
        c_rows[2 * j] = rows[2 * (long long)row];
        c_rows[2 * j + 1] = rows[2 * (long long)row + 1];
        c_key[j] = c.key | (c.term ? 0x80000000u : 0u);
        c_v1[j] = c.v;
    }
}

// virtual lane l of a chunk = virtual root v = v0 + l = (candidate v / 21, opponent roll v % 21): the afterstate with the
// opponent to move and the roll's dice.  Past the list, or under a terminal candidate: a finished lane (no roots, no rows).
__global__ __launch_bounds__(SRCH_NT) void srch_fanout_kernel(EnvView e, long long v0, const uint32_t *__restrict__ total,
                                                              const uint4 *__restrict__ c_rows, const uint32_t *__restrict__ c_key)
{
    const long long l = (long long)blockIdx.x * SRCH_NT + threadIdx.x;
    if (l >= e.n) return;
    const long long v = v0 + l, j = v / SRCH_ROLLS;
    const bool live = j < (long long)*total && !(c_key[j] & 0x80000000u);
    uint32_t p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t meta = META_FINISHED;
    if (live) {
        const uint4 a = c_rows[2 * j], b = c_rows[2 * j + 1];
        p[0] = a.x & ~TURN_BIT; p[1] = a.y; p[2] = a.z; p[3] = a.w; p[4] = b.x; p[5] = b.y; p[6] = b.z; p[7] = b.w;
        const int opp = (a.x & TURN_BIT) ? 0 : 1;
        int d1, d2;
        srch_roll((int)(v % SRCH_ROLLS), d1, d2);
        meta = meta_pack(opp, d1, d2, false);
    }
    store_planes(e, l, p);
    e.meta[l] = meta; e.ply[l] = 0; e.episode[l] = 0; e.flags[l] = 0;
}

// R(c, r) of every live virtual lane: the greedy reply's value from best (ordered bits, mover-dependent), or -- no legal reply --
// the net's value of the position with the opponent's turn bit from the root pass's hidden layer (stored as -log2(e) (W1 x + b1))
__global__ __launch_bounds__(SRCH_NT) void srch_collect_kernel(EnvView e, const unsigned long long *__restrict__ best,
                                                               const float *__restrict__ root_hidden, const float *__restrict__ w2,
                                                               const float *__restrict__ b2, long long v0, float *__restrict__ rval)
{
    const long long l = (long long)blockIdx.x * SRCH_NT + threadIdx.x;
    if (l >= e.n) return;
    const uint32_t meta = e.meta[l];
    if (meta & META_FINISHED) return;
    const unsigned long long pk = best[l];
    float r;
    if (pk != 0ull) {
        const uint32_t vb = (uint32_t)(pk >> 32);
        r = __uint_as_float((meta & 1u) ? ~vb : vb);
    } else {
        const float *h = root_hidden + l * N_HID;
        float s = 0.0f;
        for (int k = 0; k < N_HID; ++k) s = fmaf(w2[k], __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(h[k])), s);
        r = fast_sigmoid(s + *b2);
    }
    rval[v0 + l] = r;
}

// lane per game: V2 of every kept candidate (terminal: its outcome), arg-best for the mover (ties: smaller key), the winner into
// best[g] as (ordered V2 bits, ~key) -- what apply_kernel decodes -- and the scratch env's error bits into the env's
__global__ __launch_bounds__(SRCH_NT) void srch_reduce_kernel(long long n, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ koff,
                                                              const uint4 *__restrict__ c_rows, const uint32_t *__restrict__ c_key,
                                                              const float *__restrict__ c_v1, const float *__restrict__ rval,
                                                              float *__restrict__ c_v2, unsigned long long *__restrict__ best,
                                                              unsigned long long *__restrict__ err, unsigned long long *__restrict__ scratch_err)
{
    const long long g = (long long)blockIdx.x * SRCH_NT + threadIdx.x;
    if (g == 0 && scratch_err) {
        const unsigned long long x = *scratch_err;
        if (x) { atomicOr(err, x); *scratch_err = 0ull; }
    }
    if (g >= n) return;
    const uint32_t k = kept[g], j0 = koff[g];
    unsigned long long b = 0ull;
    for (uint32_t i = 0; i < k; ++i) {
        const long long j = (long long)j0 + i;
        const uint32_t key = c_key[j];
        const int mover = (c_rows[2 * j].x & TURN_BIT) ? 1 : 0;
        float v2;
        if (key & 0x80000000u) v2 = c_v1[j];
        else {
            // (sum over the doubles + 2 x sum over the other rolls) / 36, each in roll order.  A chain of fmaf with the fp32 weights
            // 1/36 and 2/36 -- which add up to 1 + 2 ulp -- gave V2 = 1.0000002 when every reply was worth exactly 1.0; here equal
            // replies of 1.0 or 0.0 give exactly that, and the average of values in [0, 1] stays inside [0, 1]
            float sd = 0.0f, so = 0.0f;
            const float *r = rval + j * SRCH_ROLLS;
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

// bgamd_env_search_read: candidate rank i < K of game g (zeros past the game's kept count)
__global__ __launch_bounds__(SRCH_NT) void srch_read_kernel(long long n, int K, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ koff,
                                                            const uint4 *__restrict__ c_rows, const float *__restrict__ c_v1,
                                                            const float *__restrict__ c_v2, int32_t *__restrict__ st, float *__restrict__ v1,
                                                            float *__restrict__ v2)
{
    const long long t = (long long)blockIdx.x * SRCH_NT + threadIdx.x;
    if (t >= n * (long long)K) return;
    const long long g = t / K;
    const uint32_t i = (uint32_t)(t % K);
    const bool has = i < kept[g];
    const long long j = (long long)koff[g] + i;
    if (st) {
        int32_t s[28];
        if (has) {
            const uint4 a = c_rows[2 * j], b = c_rows[2 * j + 1];
            const uint32_t p[8] = {a.x & ~TURN_BIT, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            state28_from_planes(p, s);
        } else {
#pragma unroll
            for (int q = 0; q < 28; ++q) s[q] = 0;
        }
#pragma unroll
        for (int q = 0; q < 28; ++q) st[t * 28 + q] = s[q];
    }
    if (v1) v1[t] = has ? c_v1[j] : 0.0f;
    if (v2) v2[t] = has ? c_v2[j] : 0.0f;
}

__global__ __launch_bounds__(SRCH_NT) void srch_kept_kernel(long long n, const uint32_t *__restrict__ kept, int32_t *__restrict__ out)
{
    const long long g = (long long)blockIdx.x * SRCH_NT + threadIdx.x;
    if (g < n) out[g] = (int32_t)kept[g];
}
