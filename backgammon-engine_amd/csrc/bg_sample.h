// bg_sample.h -- the temperature-sampled step (bgamd_env_step_sampled, include/bgamd.h): two small passes over the rows the value net
// has just evaluated, between the value net and the apply / boundary launch of a greedy step.  Included by bgamd.hip inside an anonymous
// namespace just ahead of its KERNEL_ORDER list, and both kernels are TEMPLATES (on their workgroup size): a plain kernel's code
// is emitted ahead of every kernel template's, where it would move boundary_kernel and the learner's kernels to other addresses (that
// alone cost the greedy step 0.5 %); a template's code is emitted where that list names it, behind the earlier ones.
//
//   pass A  sample_score_kernel : per row  s = d / T + g  (d = mover-side value - the lane's best, g = Gumbel noise of the row's planes),
//                                 kept in score[row]; 64-bit atomicMax of (ordered score bits, ~key) into pick[lane], the maximum first
//                                 taken over each run of equal lanes inside the wave (bg_eval.h, best_atomic_max)
//   pass B  sample_pick_kernel  : the row whose (score, ~key) is its lane's maximum writes sv.best[lane] in the greedy step's format
//                                 (ordered bits of its OWN value, ~key) -- the one writer of that word -- and counts the lane
//
// Integer atomics only: a maximum and two counts, none of which depends on the order of arrival.  sv.best is read by pass A alone and
// written by pass B alone; pass B reads the scores pass A stored, so both see the same bits.
#pragma once

// u in (0, 1) of a row: a counter-based function of (seed, game id, ply, the eight plane words) and nothing else -- not of the key, the
// row's place in the arenas, the lane count or the launch.  Two rows of one lane that hold the same afterstate under two keys draw the same u.
//   A = P(counter = p[0..3], key = seed)     B = P(counter = p[4..7] ^ A, key = seed)
//   C = P(counter = (gid_lo, gid_hi, ply, STREAM_SAMPLE), key = (B.x, B.y))
//   u = (2 (C.x >> 9) + 1) 2^-24   -- 23 random bits and a half: every u is an fp32 number, 2^-24 <= u <= 1 - 2^-24
__device__ __forceinline__ float sample_uniform(unsigned long long seed, unsigned long long gid, uint32_t ply, const uint32_t (&p)[8])
{
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const U4 a = philox4x32_10(p[0], p[1], p[2], p[3], k0, k1);
    const U4 b = philox4x32_10(p[4] ^ a.x, p[5] ^ a.y, p[6] ^ a.z, p[7] ^ a.w, k0, k1);
    const U4 c = philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), ply, STREAM_SAMPLE, b.x, b.y);
    return (float)(2u * (c.x >> 9) + 1u) * (1.0f / 16777216.0f);
}

// s = d / T + g in fp32, in exactly this order: q = d / T (IEEE division), L1 = logf(u), L2 = logf(-L1), s = q - L2.
// d <= 0 and T > 0: q is 0 for the lane's best row and -inf at worst; L2 is finite (-L1 lies in [6e-8, 16.7]); no NaN can arise.
__device__ __forceinline__ float sample_score(float d, float temperature, float u)
{
#pragma clang fp contract(off)
    const float q = __fdiv_rn(d, temperature);
    return q - logf(-logf(u));
}

// order-preserving bits of a float that may be negative or -inf (best_atomic_max's shortcut holds for values >= 0 only)
__device__ __forceinline__ uint32_t sample_ordered(float s)
{
    const uint32_t b = __float_as_uint(s);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

struct SampleView {
    unsigned long long *pick;              // [n] (ordered score bits << 32) | ~key; 0 = no row (cleared by the caller before pass A)
    unsigned long long *count;             // [2] lanes that had a move, lanes whose sampled value is not their best value
    float *score;                          // [cap_rows] by arena row
};

template <int NT>
__global__ __launch_bounds__(NT) void sample_score_kernel(EnvView e, const unsigned long long *__restrict__ tops, long long bb, long long cap_rows,
                                                          const uint4 *__restrict__ rows, const uint2 *__restrict__ info,
                                                          const float *__restrict__ values, const unsigned long long *__restrict__ best,
                                                          float temperature, SampleView sm)
{
    const SrchRows R = srch_rows(tops, bb, cap_rows);
    const int lane = threadIdx.x & 63;
    // whole waves go round together (the shuffles below need all 64 lanes): i0 is the wave's first row of this round
    for (long long i0 = (long long)blockIdx.x * NT + (threadIdx.x & ~63); i0 < R.total; i0 += (long long)gridDim.x * NT) {
        const long long i = i0 + lane;
        bool valid = i < R.total;
        uint32_t g = 0xFFFFFFFFu;
        unsigned long long pack = 0ull;
        if (valid) {
            const long long row = srch_row_at(R, i);
            const uint2 inf = info[row];
            valid = (long long)inf.x < e.n;
            if (valid) {
                g = inf.x;
                const uint4 a = rows[2 * row], b = rows[2 * row + 1];
                const uint32_t p[8] = {a.x & ~TURN_BIT, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                const bool p2 = (inf.y >> 31) != 0;
                const uint32_t vb = (uint32_t)(best[g] >> 32);
                const float v = values[row], v_best = __uint_as_float(p2 ? ~vb : vb);
                const float d = (p2 ? -v : v) - (p2 ? -v_best : v_best);
                const unsigned long long gid = e.lane_offset + (unsigned long long)g + (unsigned long long)e.episode[g] * e.lane_stride;
                const float s = sample_score(d, temperature, sample_uniform(e.seed, gid, e.ply[g], p));
                sm.score[row] = s;
                pack = ((unsigned long long)sample_ordered(s) << 32) | (uint32_t)~(inf.y & 0x7FFFFFFFu);
            }
        }
#pragma unroll
        for (int dd = 1; dd < 64; dd <<= 1) {
            const uint32_t og = __shfl_down(g, dd, 64);
            const unsigned long long op = __shfl_down(pack, dd, 64);
            if (lane + dd < 64 && og == g && op > pack) pack = op;
        }
        const uint32_t pg = __shfl_up(g, 1, 64);
        if (valid && (lane == 0 || pg != g)) atomicMax(&sm.pick[g], pack);
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void sample_pick_kernel(long long n, const unsigned long long *__restrict__ tops, long long bb, long long cap_rows,
                                                         const uint2 *__restrict__ info, const float *__restrict__ values,
                                                         unsigned long long *__restrict__ best, SampleView sm)
{
    const SrchRows R = srch_rows(tops, bb, cap_rows);
    uint32_t moved = 0, left = 0;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < R.total; i += (long long)gridDim.x * NT) {
        const long long row = srch_row_at(R, i);
        const uint2 inf = info[row];
        if ((long long)inf.x >= n) continue;
        const uint32_t nkey = (uint32_t)~(inf.y & 0x7FFFFFFFu);
        if ((((unsigned long long)sample_ordered(sm.score[row]) << 32) | nkey) != sm.pick[inf.x]) continue;
        uint32_t bits = __float_as_uint(values[row]);
        bits = (inf.y >> 31) ? ~bits : bits;
        moved += 1;
        left += (uint32_t)(best[inf.x] >> 32) != bits ? 1u : 0u;
        best[inf.x] = ((unsigned long long)bits << 32) | nkey;
    }
    // wave sums -> one LDS word each -> one global atomic per workgroup and counter (finish_turn's scheme: same-address global atomics
    // are served one after the other)
    __shared__ unsigned int s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long m = wave_sum_u32(moved), l = wave_sum_u32(left);
    if ((threadIdx.x & 63) == 0) {
        if (m) atomicAdd(&s_cnt[0], (unsigned int)m);
        if (l) atomicAdd(&s_cnt[1], (unsigned int)l);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&sm.count[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}
