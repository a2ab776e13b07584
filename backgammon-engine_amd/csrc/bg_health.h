// bg_health.h -- two measuring instruments for a training loop (include/bgamd.h: bgamd_net_health, bgamd_env_choice_spread).
//
// net health: is a weight table still one the value net can play with, and does its hidden layer still tell rows apart?
//   health_weights_kernel : one workgroup over the 25 601 weights -- non-finite count, largest finite |w| per tensor, and the acceptance
//                           test of bgamd_weights_check (w1_fits_f16_split, bg_root_resident.h: the same function the host check calls)
//   health_rows_kernel    : the 128 pre-activations a = fc1.weight x + fc1.bias of every 32-byte row on v_mfma_f32_32x32x2_f32 -- the dense
//                           evaluator's exact fp32 FMA chain over ALL 99 k-steps, W1 staged from the raw table (no 16-bit plane: this is
//                           the instrument the f16 paths are judged by) -- then |a| > threshold per (row, unit), the sigmoids and the
//                           second layer.  Counts stay in registers over a wave's tiles, are summed per workgroup in LDS and reach the
//                           result with one integer atomic per unit and workgroup
//   health_finish_kernel  : saturated = sum of the per-unit counts, dead_units = units saturated on every row
// choice spread: a segmented min / max / count over the rows of the last greedy step by game id (spread_* kernels; the rows are walked
//   as bgamd_env_unique_rows_read walks them: srch_rows / srch_row_at, bg_search.h).
// Every output is an integer count or a min / max: integer atomics and atomicMax / atomicMin on the bits of non-negative floats, so no
// result depends on the order of arrival and two calls give the same bits.
// Included by bgamd.hip inside its anonymous namespace, after bg_search.h.
#pragma once

constexpr int HEALTH_W_THREADS = 1024;
constexpr int HEALTH_THREADS = 512;                                   // 8 waves, 2 per SIMD: one workgroup per CU (101 KB of W1)
constexpr int HEALTH_LDS_TOTAL = EVAL_LDS_BYTES + (HEALTH_THREADS / 64) * EVAL_RED_FLOATS * 4;

// the device image of bgamd_net_health_t (include/bgamd.h; the offsets are asserted in bgamd.hip)
struct HealthOut {
    long long nonfinite, rows, saturated, dead_units;
    float max_abs[4], max_abs_preact, v_min, v_max;
    int fits_f16_split;
    int unit_saturated[N_HID];
};

__device__ __forceinline__ bool health_finite(float w) { return w - w == 0.0f; }

__global__ __launch_bounds__(HEALTH_W_THREADS) void health_weights_kernel(const float *__restrict__ theta, long long n_rows,
                                                                          HealthOut *__restrict__ out)
{
    __shared__ unsigned int s_bad, s_unfit, s_max[4];
    if (threadIdx.x < 4) s_max[threadIdx.x] = 0;
    if (threadIdx.x == 4) s_bad = 0;
    if (threadIdx.x == 5) s_unfit = 0;
    __syncthreads();
    unsigned int bad = 0, unfit = 0, mx[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < N_PARAMS; i += HEALTH_W_THREADS) {
        const float w = theta[i];
        const int tensor = i < N_HID * N_IN ? 0 : (i < N_HID * N_IN + N_HID ? 1 : (i < N_HID * N_IN + 2 * N_HID ? 2 : 3));
        if (!health_finite(w)) { ++bad; ++unfit; continue; }
        const unsigned int a = __float_as_uint(w) & 0x7FFFFFFFu;      // |w|: the bits of non-negative floats order like the floats
        mx[tensor] = a > mx[tensor] ? a : mx[tensor];
        if (tensor == 0) {
            _Float16 hi, lo;
            const int f = i % N_IN;
            if (!w1_fits_f16_split(f >= 196 ? w / 15.0f : w, hi, lo)) ++unfit;
        }
    }
    if (bad) atomicAdd(&s_bad, bad);
    if (unfit) atomicAdd(&s_unfit, unfit);
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (mx[t]) atomicMax(&s_max[t], mx[t]);
    __syncthreads();
    if (threadIdx.x < N_HID) out->unit_saturated[threadIdx.x] = 0;
    if (threadIdx.x < 4) out->max_abs[threadIdx.x] = __uint_as_float(s_max[threadIdx.x]);
    if (threadIdx.x == 0) {
        out->nonfinite = (long long)s_bad;
        out->rows = n_rows;
        out->saturated = 0;
        out->dead_units = 0;
        out->max_abs_preact = 0.0f;
        out->v_min = n_rows > 0 ? __uint_as_float(0x7F800000u) : 0.0f;          // the rows pass takes the minimum into it
        out->v_max = 0.0f;
        out->fits_f16_split = s_unfit == 0 ? 1 : 0;
    }
}

__global__ __launch_bounds__(HEALTH_THREADS) void health_rows_kernel(const float *__restrict__ theta, const uint4 *__restrict__ rows,
                                                                     long long n_rows, float threshold, HealthOut *__restrict__ out)
{
    extern __shared__ float4 sHW[];
    float *sRed = reinterpret_cast<float *>(sHW + K_STEPS * 64) + (threadIdx.x >> 6) * EVAL_RED_FLOATS;
    __shared__ unsigned int s_unit[N_HID], s_amax, s_vmin, s_vmax;
    // W1 in the f32 MFMA's B layout (relayout_w1_f32): sHW[s][l].c = W1[32c + (l & 31)][2s + (l >> 5)], straight from the raw table
    for (int i = threadIdx.x; i < K_STEPS * 64; i += HEALTH_THREADS) {
        const int s = i >> 6, l = i & 63;
        const float *w = theta + (l & 31) * N_IN + 2 * s + (l >> 5);
        sHW[i] = make_float4(w[0], w[32 * N_IN], w[64 * N_IN], w[96 * N_IN]);
    }
    if (threadIdx.x < N_HID) s_unit[threadIdx.x] = 0;
    if (threadIdx.x == 0) { s_amax = 0; s_vmin = 0x7F800000u; s_vmax = 0; }
    __syncthreads();

    const long long n_tiles = (n_rows + 31) >> 5;
    const int lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const long long wave = (long long)blockIdx.x * (HEALTH_THREADS / 64) + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * (HEALTH_THREADS / 64);
    const float *b1 = theta + N_HID * N_IN, *w2 = b1 + N_HID;
    float b1v[4], w2v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { b1v[c] = b1[32 * c + r]; w2v[c] = w2[32 * c + r]; }
    const float b2 = w2[N_HID];

    unsigned int sat[4] = {0, 0, 0, 0};                   // this lane's units 32c + r, over the rows of its half
    float amax = 0.0f;
    unsigned int vmin = 0x7F800000u, vmax = 0;

    for (long long tile = wave; tile < n_tiles; tile += n_waves) {
        uint4 u0 = make_uint4(0, 0, 0, 0), u1 = make_uint4(0, 0, 0, 0);
        if (tile * 32 + r < n_rows) { u0 = rows[2 * (tile * 32 + r)]; u1 = rows[2 * (tile * 32 + r) + 1]; }
        const uint32_t p[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
        RowDecode rd;
        decode_setup(p, h, rd);
        floatx16 acc0 = {0}, acc1 = {0}, acc2 = {0}, acc3 = {0};
#define BG_HEALTH_MFMA4(aval, WV)                                                    \
    {                                                                                \
        const float4 wv_ = (WV);                                                     \
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32((aval), wv_.x, acc0, 0, 0, 0);     \
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32((aval), wv_.y, acc1, 0, 0, 0);     \
        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32((aval), wv_.z, acc2, 0, 0, 0);     \
        acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32((aval), wv_.w, acc3, 0, 0, 0);     \
    }
        const float4 *wp = sHW + lane;
        for (int i = 0; i < 24; ++i) {                    // k-steps 4i .. 4i + 3: point i, side 0 even / odd, side 1 even / odd
            BG_HEALTH_MFMA4(decode_even(rd, 0, i), wp[(4 * i + 0) * 64]);
            BG_HEALTH_MFMA4(decode_odd(rd, 0, i), wp[(4 * i + 1) * 64]);
            BG_HEALTH_MFMA4(decode_even(rd, 1, i), wp[(4 * i + 2) * 64]);
            BG_HEALTH_MFMA4(decode_odd(rd, 1, i), wp[(4 * i + 3) * 64]);
        }
        BG_HEALTH_MFMA4(rd.tail[0], wp[96 * 64]);
        BG_HEALTH_MFMA4(rd.tail[1], wp[97 * 64]);
        BG_HEALTH_MFMA4(rd.tail[2], wp[98 * 64]);
#undef BG_HEALTH_MFMA4

        float part[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool vrow = tile * 32 + (j & 3) + 8 * (j >> 2) + 4 * h < n_rows;
            const float a[4] = {acc0[j] + b1v[0], acc1[j] + b1v[1], acc2[j] + b1v[2], acc3[j] + b1v[3]};
            float sum = 0.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float aa = __builtin_fabsf(a[c]);
                if (vrow) {
                    sat[c] += aa > threshold ? 1u : 0u;
                    amax = __builtin_fmaxf(amax, aa);
                }
                sum += w2v[c] * fast_sigmoid(a[c]);
            }
            part[j] = sum;
        }
        // the sum over the 32 columns through the per-wave LDS transpose of eval_rows_f32_kernel
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) sRed[r * EVAL_RED_STRIDE + 8 * q + 4 * h + j] = part[4 * q + j];
        __builtin_amdgcn_wave_barrier();
        float sum = 0.0f;
#pragma unroll
        for (int c = 0; c < 16; ++c) sum += sRed[(16 * h + c) * EVAL_RED_STRIDE + r];
        sum += __shfl_xor(sum, 32, 64);
        __builtin_amdgcn_wave_barrier();
        if (h == 0 && tile * 32 + r < n_rows) {
            const unsigned int vb = __float_as_uint(fast_sigmoid(sum + b2));       // in [0, 1] for finite weights: bits order like values
            vmin = vb < vmin ? vb : vmin;
            vmax = vb > vmax ? vb : vmax;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (sat[c]) atomicAdd(&s_unit[32 * c + r], sat[c]);
    atomicMax(&s_amax, __float_as_uint(amax));
    atomicMin(&s_vmin, vmin);
    atomicMax(&s_vmax, vmax);
    __syncthreads();
    if (threadIdx.x < N_HID && s_unit[threadIdx.x]) atomicAdd(&out->unit_saturated[threadIdx.x], (int)s_unit[threadIdx.x]);
    if (threadIdx.x == 0) {
        atomicMax(reinterpret_cast<unsigned int *>(&out->max_abs_preact), s_amax);
        atomicMin(reinterpret_cast<unsigned int *>(&out->v_min), s_vmin);
        atomicMax(reinterpret_cast<unsigned int *>(&out->v_max), s_vmax);
    }
}

__global__ __launch_bounds__(N_HID) void health_finish_kernel(HealthOut *__restrict__ out)
{
    __shared__ unsigned long long s_sat;
    __shared__ unsigned int s_dead;
    if (threadIdx.x == 0) { s_sat = 0; s_dead = 0; }
    __syncthreads();
    const long long c = out->unit_saturated[threadIdx.x];
    atomicAdd(&s_sat, (unsigned long long)c);
    if (c == out->rows) atomicAdd(&s_dead, 1u);
    __syncthreads();
    if (threadIdx.x == 0) { out->saturated = (long long)s_sat; out->dead_units = (long long)s_dead; }
}

// ---- choice spread ---------------------------------------------------------------------------------------------------------------
// per lane: [0] rows, [1] largest / [2] smallest "ordered" value (the bits of the stored value, complemented for PLAYER2: larger =
// better for the mover, best_atomic_max's order), [3] rows bit-equal to the best, [4] the mover.  Cleared by the caller: 0, 0, ~0, 0, 0.
struct SpreadView {
    uint32_t *cnt, *hi, *lo, *tied, *mover;
};

__device__ __forceinline__ uint32_t spread_ordered(const uint4 *__restrict__ rows, const float *__restrict__ values, long long row,
                                                   uint32_t &mover)
{
    mover = (rows[2 * row].x & TURN_BIT) ? 1u : 0u;
    const uint32_t bits = __float_as_uint(values[row]);
    return mover ? ~bits : bits;
}

__global__ __launch_bounds__(SRCH_NT) void spread_reduce_kernel(const unsigned long long *__restrict__ tops, long long bb, long long cap_rows,
                                                                const uint4 *__restrict__ rows, const uint2 *__restrict__ info,
                                                                const float *__restrict__ values, long long n, SpreadView sp)
{
    const SrchRows R = srch_rows(tops, bb, cap_rows);
    for (long long i = (long long)blockIdx.x * SRCH_NT + threadIdx.x; i < R.total; i += (long long)gridDim.x * SRCH_NT) {
        const long long row = srch_row_at(R, i);
        const uint32_t g = info[row].x;
        if ((long long)g >= n) continue;
        uint32_t mover;
        const uint32_t ord = spread_ordered(rows, values, row, mover);
        atomicAdd(&sp.cnt[g], 1u);
        atomicMax(&sp.hi[g], ord);
        atomicMin(&sp.lo[g], ord);
        sp.mover[g] = mover;                                  // (every row of a lane carries the same turn bit)
    }
}

__global__ __launch_bounds__(SRCH_NT) void spread_tied_kernel(const unsigned long long *__restrict__ tops, long long bb, long long cap_rows,
                                                              const uint4 *__restrict__ rows, const uint2 *__restrict__ info,
                                                              const float *__restrict__ values, long long n, SpreadView sp)
{
    const SrchRows R = srch_rows(tops, bb, cap_rows);
    for (long long i = (long long)blockIdx.x * SRCH_NT + threadIdx.x; i < R.total; i += (long long)gridDim.x * SRCH_NT) {
        const long long row = srch_row_at(R, i);
        const uint32_t g = info[row].x;
        if ((long long)g >= n) continue;
        uint32_t mover;
        if (spread_ordered(rows, values, row, mover) == sp.hi[g]) atomicAdd(&sp.tied[g], 1u);
    }
}

// summary (cleared by the caller): [0] lanes with >= 2 rows, [1] of those the lanes whose rows all tie, [2] rows, [3] lanes without rows
__global__ __launch_bounds__(SRCH_NT) void spread_finish_kernel(long long n, SpreadView sp, int32_t *__restrict__ count, float *__restrict__ best,
                                                                float *__restrict__ worst, int32_t *__restrict__ tied,
                                                                unsigned long long *__restrict__ summary)
{
    const long long g = (long long)blockIdx.x * SRCH_NT + threadIdx.x;
    if (g >= n) return;
    const uint32_t c = sp.cnt[g], t = sp.tied[g], flip = sp.mover[g] ? 0xFFFFFFFFu : 0u;
    if (count) count[g] = (int32_t)c;
    if (best) best[g] = c ? __uint_as_float(sp.hi[g] ^ flip) : 0.0f;
    if (worst) worst[g] = c ? __uint_as_float(sp.lo[g] ^ flip) : 0.0f;
    if (tied) tied[g] = (int32_t)t;
    if (summary) {
        if (c >= 2) atomicAdd(&summary[0], 1ull);
        if (c >= 2 && t == c) atomicAdd(&summary[1], 1ull);
        if (c) atomicAdd(&summary[2], (unsigned long long)c);
        if (c == 0) atomicAdd(&summary[3], 1ull);
    }
}
