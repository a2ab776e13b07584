// bgamd_search3.hip -- the kernels of the 3-ply search step and their launches (bg_search3.h holds the step's plan and the prototypes).
// A translation unit of its own, linked into libbgamd.so behind bgamd.hip: its kernels are a second gfx950 code object, and bgamd.hip's
// -- the greedy step's kernels, their order and addresses -- does not change when one is added here.  It shares with
// bgamd.hip only what both must agree on: the row format (bg_board.h), the search's order and rolls (bg_search_order.h), SRCH_NT.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bg_board.h"
#include "bg_step_plan.h"
#include "bg_search3.h"

using namespace bg;
using bg::s3::DeepList;

namespace {
#include "bg_search_order.h"

// (sum over the 6 doubles + 2 x sum over the 15 other rolls) / 36, each part in roll order: srch_reduce_kernel's expression (that kernel's
// code stays as it is), so equal values of 1.0 or 0.0 give exactly that
__device__ __forceinline__ float s3_roll_mean(const float *__restrict__ r)
{
    float sd = 0.0f, so = 0.0f;
#pragma unroll
    for (int idx = 0, a = 1; a <= 6; ++a)
#pragma unroll
        for (int d = a; d <= 6; ++d, ++idx) {
            if (a == d) sd += r[idx];
            else so += r[idx];
        }
    return (sd + 2.0f * so) * (1.0f / 36.0f);
}

// The deep set of every lane the filtered step searched (kept >= 2): rank r of candidate c = the number of kept candidates that beat it in
// the (V2 for the mover, smaller key) order; d2 = one fp32 subtraction from rank 0's V2 on the mover's side (never negative); c is in L2 iff
// r < k_lim and (r == 0 or d2 <= margin).  d2 does not fall as the rank grows, so L2 is ranks 0 .. |L2| - 1.  O(kept^2) per lane.
template <int NT>
__global__ __launch_bounds__(NT) void s3_deep_select_kernel(long long n, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ koff,
                                                            const uint4 *__restrict__ c_rows, const uint32_t *__restrict__ c_key,
                                                            const float *__restrict__ c_v2, uint32_t k_lim, float margin,
                                                            int32_t *__restrict__ c_d3, uint32_t *__restrict__ dkept)
{
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    if (g >= n) return;
    const uint32_t k = kept[g], j0 = koff[g];
    uint32_t nd = 0;
    if (k >= 2) {
        const int mover = (c_rows[2 * (long long)j0].x & TURN_BIT) ? 1 : 0;
        unsigned long long pb = 0ull;
        float vb = 0.0f;
        for (uint32_t i = 0; i < k; ++i) {
            const long long j = (long long)j0 + i;
            const unsigned long long p = srch_pack(c_v2[j], c_key[j] & 0x7FFFFFFFu, mover);
            if (p > pb) { pb = p; vb = c_v2[j]; }
        }
        for (uint32_t i = 0; i < k; ++i) {
            const long long j = (long long)j0 + i;
            const float v = c_v2[j];
            const unsigned long long pi = srch_pack(v, c_key[j] & 0x7FFFFFFFu, mover);
            uint32_t better = 0;
            for (uint32_t q = 0; q < k; ++q) better += srch_pack(c_v2[(long long)j0 + q], c_key[(long long)j0 + q] & 0x7FFFFFFFu, mover) > pi ? 1u : 0u;
            const float d2 = mover ? v - vb : vb - v;
            const bool keep = better < k_lim && (better == 0 || d2 <= margin);
            c_d3[j] = keep ? (int32_t)better : -1;
            nd += keep ? 1u : 0u;
        }
    } else if (k == 1)
        c_d3[j0] = -1;
    dkept[g] = nd >= 2 ? nd : 0u;
}

// the deep candidates: entry doff[g] + rank of the compact list is candidate j, for the lanes with |L2| >= 2
template <int NT>
__global__ __launch_bounds__(NT) void s3_deep_map_kernel(long long n, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ koff,
                                                         const uint32_t *__restrict__ dkept, const uint32_t *__restrict__ doff,
                                                         const int32_t *__restrict__ c_d3, uint32_t *__restrict__ dmap)
{
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    if (g >= n || dkept[g] < 2) return;
    const uint32_t k = kept[g], j0 = koff[g], d0 = doff[g];
    for (uint32_t i = 0; i < k; ++i) {
        const int32_t r = c_d3[(long long)j0 + i];
        if (r >= 0) dmap[d0 + (uint32_t)r] = j0 + i;
    }
}

// mid lane l of a chunk -> is it live, and its deep candidate j (header: bg_search3.h)
__device__ __forceinline__ bool s3_mid_live(const DeepList &d, long long v, long long &j)
{
    const long long jv = v / SRCH_ROLLS;
    if (jv >= (long long)*d.total) return false;
    j = d.map[jv];
    return !(d.key[j] & 0x80000000u);
}

// Behind flt_select_kernel on the mid env: a live mid lane without rows -- the opponent has no move on a non-doubles roll -- keeps ONE
// reply, the pass (s3_pass_emit_kernel writes it).  A doubles roll without a move has its row already: the position itself.
template <int NT>
__global__ __launch_bounds__(NT) void s3_reply_fix_kernel(long long n, long long v0, DeepList d, const uint32_t *__restrict__ cnt,
                                                          uint32_t *__restrict__ kept)
{
    const long long l = (long long)blockIdx.x * NT + threadIdx.x;
    long long j;
    if (l < n && cnt[l] == 0 && s3_mid_live(d, v0 + l, j)) kept[l] = 1u;
}

// The pass reply of a mid lane without rows, as candidate koff[l]: the deep candidate's position with the OPPONENT's turn bit (the side
// that passes), the smallest key, and v1 = pass_v1[l], the net's value of it that srch_collect_kernel formed from the root pass's
// hidden layer of the mid env.
template <int NT>
__global__ __launch_bounds__(NT) void s3_pass_emit_kernel(long long n, long long v0, DeepList d, const uint32_t *__restrict__ cnt,
                                                          const uint32_t *__restrict__ koff, const float *__restrict__ pass_v1,
                                                          uint4 *__restrict__ c_rows, uint32_t *__restrict__ c_key, float *__restrict__ c_v1)
{
    const long long l = (long long)blockIdx.x * NT + threadIdx.x;
    long long jc;
    if (l >= n || cnt[l] != 0 || !s3_mid_live(d, v0 + l, jc)) return;
    uint4 a = d.rows[2 * jc];
    a.x ^= TURN_BIT;                                       // (the candidate's row carries the mover's)
    const long long j = koff[l];
    c_rows[2 * j] = a;
    c_rows[2 * j + 1] = d.rows[2 * jc + 1];
    c_key[j] = 0u;
    c_v1[j] = pass_v1[l];
}

// Lane per mid lane l = mid root v0 + l: V2 of every kept reply (a terminal reply: its outcome) by s3_roll_mean over its 21 roll values,
// R3 = the best of them for the opponent o (the other side than the deep candidate's mover) into r3[v0 + l].  roots += 21 x the non-terminal replies (one atomic per
// workgroup); the scratch env's error bits into the mid env's.
template <int NT>
__global__ __launch_bounds__(NT) void s3_r3_reduce_kernel(long long n, long long v0, DeepList d, const uint32_t *__restrict__ kept,
                                                          const uint32_t *__restrict__ koff, const uint32_t *__restrict__ c_key,
                                                          const float *__restrict__ c_v1, const float *__restrict__ rval,
                                                          float *__restrict__ c_v2, float *__restrict__ r3, unsigned long long *__restrict__ roots,
                                                          unsigned long long *__restrict__ err, unsigned long long *__restrict__ scratch_err)
{
    __shared__ unsigned int s_roots;
    if (threadIdx.x == 0) s_roots = 0u;
    __syncthreads();
    const long long l = (long long)blockIdx.x * NT + threadIdx.x;
    if (l == 0 && scratch_err) {
        const unsigned long long x = *scratch_err;
        if (x) { atomicOr(err, x); *scratch_err = 0ull; }
    }
    unsigned int mine = 0u;
    long long jc;
    if (l < n && s3_mid_live(d, v0 + l, jc)) {
        const int o = (d.rows[2 * jc].x & TURN_BIT) ? 0 : 1;
        const uint32_t k = kept[l], j0 = koff[l];
        unsigned long long b = 0ull;
        for (uint32_t i = 0; i < k; ++i) {
            const long long j = (long long)j0 + i;
            const uint32_t key = c_key[j];
            const bool term = (key & 0x80000000u) != 0;
            const float v2 = term ? c_v1[j] : s3_roll_mean(rval + j * SRCH_ROLLS);
            c_v2[j] = v2;
            mine += term ? 0u : (unsigned int)SRCH_ROLLS;
            const unsigned long long pk = srch_pack(v2, key & 0x7FFFFFFFu, o);
            b = pk > b ? pk : b;
        }
        const uint32_t vb = (uint32_t)(b >> 32);
        r3[v0 + l] = k ? __uint_as_float(o ? ~vb : vb) : 0.0f;
    }
    if (mine) atomicAdd(&s_roots, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_roots) atomicAdd(roots, (unsigned long long)s_roots);
}

// Lane per game.  A lane searched deeper (|L2| >= 2): V3 of every member of L2 -- a terminal one keeps its outcome -- by s3_roll_mean over
// its 21 mid roots, arg-best for the mover (ties: the smaller key) into best[g] as (ordered value bits, ~key), what apply_kernel decodes.
// Any other lane keeps the best[g] the filtered step's reduce left: its V2 choice, which is rank 0 of the deep order, or its singleton.
// The mid env's error bits into the env's.
template <int NT>
__global__ __launch_bounds__(NT) void s3_v3_reduce_kernel(long long n, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ koff,
                                                          const uint32_t *__restrict__ dkept, const uint32_t *__restrict__ doff,
                                                          const uint4 *__restrict__ c_rows, const uint32_t *__restrict__ c_key,
                                                          const float *__restrict__ c_v1, const int32_t *__restrict__ c_d3,
                                                          const float *__restrict__ r3, float *__restrict__ c_v3,
                                                          unsigned long long *__restrict__ best, unsigned long long *__restrict__ err,
                                                          unsigned long long *__restrict__ mid_err)
{
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    if (g == 0 && mid_err) {
        const unsigned long long x = *mid_err;
        if (x) { atomicOr(err, x); *mid_err = 0ull; }
    }
    if (g >= n || dkept[g] < 2) return;
    const uint32_t k = kept[g], j0 = koff[g], d0 = doff[g];
    const int mover = (c_rows[2 * (long long)j0].x & TURN_BIT) ? 1 : 0;
    unsigned long long b = 0ull;
    for (uint32_t i = 0; i < k; ++i) {
        const long long j = (long long)j0 + i;
        const int32_t r = c_d3[j];
        if (r < 0) continue;
        const uint32_t key = c_key[j];
        const float v3 = (key & 0x80000000u) ? c_v1[j] : s3_roll_mean(r3 + ((long long)d0 + r) * SRCH_ROLLS);
        c_v3[j] = v3;
        const unsigned long long pk = srch_pack(v3, key & 0x7FFFFFFFu, mover);
        b = pk > b ? pk : b;
    }
    best[g] = b;
}

// bgamd_env_search3_read: slot i < K of game g, aligned with srch_read_kernel's.  depth = 0 past the kept count, 1 for a singleton's
// candidate, 3 for a member of the deep set of a lane searched deeper, else 2; v3 = 0 where depth < 3.
template <int NT>
__global__ __launch_bounds__(NT) void s3_read_kernel(long long n, int K, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ koff,
                                                     const uint32_t *__restrict__ dkept, const int32_t *__restrict__ c_d3,
                                                     const float *__restrict__ c_v3, float *__restrict__ v3, int32_t *__restrict__ depth)
{
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t >= n * (long long)K) return;
    const long long g = t / K;
    const uint32_t i = (uint32_t)(t % K), k = kept[g];
    int32_t d = 0;
    float v = 0.0f;
    if (i < k) {
        const long long j = (long long)koff[g] + i;
        d = k < 2 ? 1 : (dkept[g] >= 2 && c_d3[j] >= 0) ? 3 : 2;
        if (d == 3) v = c_v3[j];
    }
    if (v3) v3[t] = v;
    if (depth) depth[t] = d;
}

// bgamd_env_search3_info.  One workgroup; integer sums.  out[0] lanes with a kept candidate, [1] lanes searched at 2 plies (kept >= 2),
// [2] lanes searched at 3 plies (|L2| >= 2), [3] their deep candidates, [4] mid lanes = 21 x the non-terminal ones of those, [5] the level-3
// virtual roots the mid level scored (summed by s3_r3_reduce_kernel).
template <int NT>
__global__ __launch_bounds__(NT) void s3_info_kernel(long long n, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ koff,
                                                     const uint32_t *__restrict__ dkept, const uint32_t *__restrict__ c_key,
                                                     const int32_t *__restrict__ c_d3, const unsigned long long *__restrict__ roots,
                                                     unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long s_sum[5];
    if (threadIdx.x < 5) s_sum[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long v[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    for (long long g = threadIdx.x; g < n; g += NT) {
        const uint32_t k = kept[g], j0 = koff[g], nd = dkept[g];
        if (k == 0) continue;
        v[0] += 1ull;
        if (k < 2) continue;
        v[1] += 1ull;
        if (nd < 2) continue;
        v[2] += 1ull;
        v[3] += nd;
        for (uint32_t i = 0; i < k; ++i) {
            const long long j = (long long)j0 + i;
            v[4] += (c_d3[j] >= 0 && !(c_key[j] & 0x80000000u)) ? (unsigned long long)SRCH_ROLLS : 0ull;
        }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q)
        if (v[q]) atomicAdd(&s_sum[q], v[q]);
    __syncthreads();
    if (threadIdx.x < 5) out[threadIdx.x] = s_sum[threadIdx.x];
    if (threadIdx.x == 5) out[5] = *roots;
}

}  // namespace

// ---- the launches (bg_search3.h) ------------------------------------------------------------------------------------------------------
namespace bg {
namespace s3 {
static dim3 grid1(long long n, int bs) { return dim3((unsigned)((n + bs - 1) / bs)); }
#define S3_LAUNCH(kernel, threads, count, ...) hipLaunchKernelGGL(kernel<threads>, grid1(count, threads), dim3(threads), 0, s, __VA_ARGS__)

void deep_select(hipStream_t s, long long n, const uint32_t *kept, const uint32_t *koff, const uint4 *c_rows, const uint32_t *c_key,
                 const float *c_v2, uint32_t k_lim, float margin, int32_t *c_d3, uint32_t *dkept)
{
    S3_LAUNCH(s3_deep_select_kernel, SRCH_NT, n, n, kept, koff, c_rows, c_key, c_v2, k_lim, margin, c_d3, dkept);
}
void deep_map(hipStream_t s, long long n, const uint32_t *kept, const uint32_t *koff, const uint32_t *dkept, const uint32_t *doff,
              const int32_t *c_d3, uint32_t *dmap)
{
    S3_LAUNCH(s3_deep_map_kernel, SRCH_NT, n, n, kept, koff, dkept, doff, c_d3, dmap);
}
void reply_fix(hipStream_t s, long long n, long long v0, DeepList deep, const uint32_t *cnt, uint32_t *kept)
{
    S3_LAUNCH(s3_reply_fix_kernel, SRCH_NT, n, n, v0, deep, cnt, kept);
}
void pass_emit(hipStream_t s, long long n, long long v0, DeepList deep, const uint32_t *cnt, const uint32_t *koff, const float *pass_v1,
               uint4 *c_rows, uint32_t *c_key, float *c_v1)
{
    S3_LAUNCH(s3_pass_emit_kernel, SRCH_NT, n, n, v0, deep, cnt, koff, pass_v1, c_rows, c_key, c_v1);
}
void r3_reduce(hipStream_t s, long long n, long long v0, DeepList deep, const uint32_t *kept, const uint32_t *koff, const uint32_t *c_key,
               const float *c_v1, const float *rval, float *c_v2, float *r3, unsigned long long *roots, unsigned long long *err,
               unsigned long long *scratch_err)
{
    S3_LAUNCH(s3_r3_reduce_kernel, SRCH_NT, n, n, v0, deep, kept, koff, c_key, c_v1, rval, c_v2, r3, roots, err, scratch_err);
}
void v3_reduce(hipStream_t s, long long n, const uint32_t *kept, const uint32_t *koff, const uint32_t *dkept, const uint32_t *doff,
               const uint4 *c_rows, const uint32_t *c_key, const float *c_v1, const int32_t *c_d3, const float *r3, float *c_v3,
               unsigned long long *best, unsigned long long *err, unsigned long long *mid_err)
{
    S3_LAUNCH(s3_v3_reduce_kernel, SRCH_NT, n, n, kept, koff, dkept, doff, c_rows, c_key, c_v1, c_d3, r3, c_v3, best, err, mid_err);
}
void read(hipStream_t s, long long n, int K, const uint32_t *kept, const uint32_t *koff, const uint32_t *dkept, const int32_t *c_d3,
          const float *c_v3, float *v3, int32_t *depth)
{
    S3_LAUNCH(s3_read_kernel, SRCH_NT, n * K, n, K, kept, koff, dkept, c_d3, c_v3, v3, depth);
}
void info(hipStream_t s, long long n, const uint32_t *kept, const uint32_t *koff, const uint32_t *dkept, const uint32_t *c_key,
          const int32_t *c_d3, const unsigned long long *roots, unsigned long long *out)
{
    hipLaunchKernelGGL(s3_info_kernel<1024>, dim3(1), dim3(1024), 0, s, n, kept, koff, dkept, c_key, c_d3, roots, out);
}
#undef S3_LAUNCH
}  // namespace s3
}  // namespace bg
