// bg_fit.h -- one SUPERVISED step of the value net (include/bgamd.h: bgamd_td_fit_step): n packed 32-byte rows with n fp32 targets
// y_i (P(PLAYER1 wins): rollout means, search values), and, in the closed form of bg_learner.h,
//
//   h = σ(W1 x + b1), v = σ(W2·h + b2), g = v(1-v);  ∇b2 = g, ∇W2 = g h, ∇b1 = db1 = g W2 ⊙ h ⊙ (1-h), ∇W1 = db1 ⊗ x
//   δ_i = y_i - v_i (fp32), coef_i = fp32((double) alpha · (double) δ_i), update = Σ_i coef_i ∇V(x_i)
//
// -- the TD learner's update of a game's terminal step with e = ∇ (train.py:165-170 with a real-valued z): the squared-error
// gradient step.  No traces: the W1 part of the sum is the matrix product dW1ᵀ[198][128] = Xᵀ D with D[i] = coef_i · db1_i, and nothing
// per row ever reaches HBM.  A row whose target is not finite adds nothing and is counted as skipped.
//
// fit_step_kernel: a workgroup of four waves walks 32-row tiles b, b + G, b + 2 G, ... of a chunk (G = workgroups of the launch).
// Per tile:
//   decode        the tile's rows -> sX[32][198 (+ zero columns up to 224)] fp32 in LDS: the encoder's features exactly (cnt / 15
//                 is no 16-bit number), td_feature_value of bg_learner.h
//   forward       W1 x on v_mfma_f32_32x32x2_f32, 99 k-steps: A = sX (row = lane & 31, feature 2 s + (lane >> 5)), B = the wave's 32
//                 hidden units of W1ᵀ, held in 99 registers per lane for the whole launch; + b1, σ; w2·h through LDS, the W2 dot
//                 by 8 threads per row in a fixed order (td_forward_mfma_kernel's), + b2, σ, δ, coef, g per row
//   factors       D[row][unit] = coef · db1 -> LDS; Σ coef · db1 (b1) and Σ coef · g h (W2) per lane on the VALUs over the lane's 16
//                 rows; Σ coef · g (b2), Σ δ² (float64) and the row counts per row slot, on the thread that formed the row's δ
//   gradient      dW1ᵀ += Xᵀ D on the same instruction, K = the tile's 32 rows = 16 k-steps: A = sX (feature 32 f + (lane & 31),
//                 row 2 s + (lane >> 5)) for the seven feature tiles f, B = D (the wave's 32 units); 7 x 16 accumulators per lane
//                 stay in registers over ALL tiles of the workgroup
// and at its end the workgroup writes ONE row of the learner's `partial` buffer (internal order: [feature][unit] | b1 | W2 | b2).
// fit_reduce_kernel sums the G rows in td_reduce_kernel's order, adds the chunks before it, and on the last chunk hands the update
// out or applies it: θ, w1t and the bf16 planes wl3 refreshed exactly as td_reduce_kernel does.
//
// Chunks: a call walks its rows in chunks of FIT_CHUNK_ROWS (BGAMD_FIT_CHUNK at bgamd_td_create; a multiple of 32), a kernel pair per
// chunk; n is bounded by nothing else.
//
// Reduction order (deterministic: no floating-point atomics; the same call gives the same bits).  For a chunk of m rows:
// tiles = ceil(m / 32), G = min(tiles, 256) (BGAMD_FIT_GROUPS at bgamd_td_create: another cap), a workgroup takes at most
// tpw = ceil(tiles / G) tiles.  The fp32 additions that reach one parameter:
//   in the workgroup   one fused multiply-add per row, in row order: a chain of 32 · tpw (W1: the MFMA's k-ordered chain over the
//                      tiles; b1 | W2: two chains of 16 · tpw, then one addition; b2: a chain of tpw per row slot, then the 32
//                      slots pairwise, 5 levels)
//   over workgroups    thread gl of 16 adds rows gl, gl + 16, ... : ceil(G / 16), then the 16 sums in order: 16
//   over chunks        one addition per chunk after the first
// so the longest chain into one parameter is
//   C(n) = max over the chunks of (32 · tpw + ceil(G / 16) + 16) + (chunks - 1)
// = 304 for one full chunk of 65 536 rows (tpw = 8, G = 256), 49 for n <= 32.  (tests/fit_ref.py computes its rounding term from this.)
//
// Per row, from the shapes: forward 2 · 198 · 128 + gradient 2 · 198 · 128 (224 columns issued) + second layer ~ 4 · 128 flop
// = 101 888 flop; 32 B of row + 4 B of target read; written per launch: G x 102 656 B of partial sums, independent of n.
#pragma once
#include "bg_learner.h"

namespace bg {

constexpr int FIT_THREADS = 256;             // four waves: wave c owns hidden units 32 c .. 32 c + 31
constexpr int FIT_FT = 7;                    // feature tiles of 32: 198 -> 224 columns, the last 26 zero
constexpr int FIT_XLD = 225;                 // row stride of sX (odd: the forward's A operand, one row per lane, meets no bank twice)
constexpr int FIT_HLD = N_HID + 1;

struct FitView {
    const uint4 *rows;                       // [m] x 2 uint4: the chunk's rows
    const float *target;                     // [m]
    long long m;
    int tiles;
    const float *theta, *w1t;
    float *partial;                          // [TD_MAX_GROUPS][TD_LD]: the learner's (free between replays)
    double *part_sq;                         // [TD_MAX_GROUPS] Σ δ² of the workgroup's rows
    long long *part_cnt;                     // [TD_MAX_GROUPS][2] rows that counted | rows skipped
};

__global__ __launch_bounds__(FIT_THREADS) void fit_step_kernel(FitView f, double alpha)
{
    __shared__ float sX[FIT_TILE][FIT_XLD];
    __shared__ float sH[FIT_TILE][FIT_HLD];               // w2 · h of the tile, then D = coef · db1
    __shared__ uint32_t sRow[FIT_TILE][8];
    __shared__ float sCoef[FIT_TILE], sG[FIT_TILE];
    __shared__ double sSq[FIT_TILE];                      // the 32 row slots' sums, met once at the workgroup's end
    __shared__ long long sCnt[FIT_TILE][2];
    const int tid = threadIdx.x, lane = tid & 63, c = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int n = 32 * c + r;                             // this lane's hidden unit (B operand and accumulator column)
    float w[N_IN / 2];                                    // W1[n][2 s + hh]: the lane's B operand of forward k-step s
#pragma unroll
    for (int s = 0; s < N_IN / 2; ++s) w[s] = f.w1t[(2 * s + hh) * N_HID + n];
    const float bb = f.theta[TD_OFF_B1 + n], w2n = f.theta[TD_OFF_W2 + n], b2 = f.theta[TD_OFF_B2];
    floatx16 gacc[FIT_FT];
#pragma unroll
    for (int ft = 0; ft < FIT_FT; ++ft) gacc[ft] = (floatx16){0};
    float accb1 = 0.0f, accw2 = 0.0f, accb2 = 0.0f;
    double sq = 0.0;
    long long cnt = 0, skipped = 0;
    for (int q = tid; q < FIT_TILE * (FIT_XLD - N_IN); q += FIT_THREADS) sX[q / (FIT_XLD - N_IN)][N_IN + q % (FIT_XLD - N_IN)] = 0.0f;

    for (int tile = blockIdx.x; tile < f.tiles; tile += gridDim.x) {
        const long long r0 = (long long)tile * FIT_TILE;
        // the target of row tid >> 3 (the thread that forms its δ below): requested before anything waits
        float y = 0.0f;
        if ((tid & 7) == 0 && r0 + (tid >> 3) < f.m) y = f.target[r0 + (tid >> 3)];
        __syncthreads();                                  // the last tile's gradient product has read sX and sH
        if (tid < 2 * FIT_TILE) {
            const long long i = r0 + (tid >> 1);
            uint4 u = make_uint4(0, 0, 0, 0);
            if (i < f.m) u = f.rows[2 * i + (tid & 1)];
            uint32_t *d = &sRow[tid >> 1][4 * (tid & 1)];
            d[0] = u.x; d[1] = u.y; d[2] = u.z; d[3] = u.w;
        }
        __syncthreads();
        for (int q = tid; q < FIT_TILE * N_IN; q += FIT_THREADS) {
            const int row = q / N_IN, j = q - row * N_IN;
            sX[row][j] = r0 + row < f.m ? td_feature_value(sRow[row], j) : 0.0f;
        }
        __syncthreads();
        // ---- forward: [32 rows x 198] · [198 x 32 units] per wave ----
        floatx16 acc = {0};
#pragma unroll
        for (int s = 0; s < N_IN / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sX[r][2 * s + hh], w[s], acc, 0, 0, 0);
        // accumulator j of this lane = tile row (j & 3) + 8 (j >> 2) + 4 hh, hidden unit n
        float hv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            hv[j] = td_sigmoid(acc[j] + bb);
            sH[(j & 3) + 8 * (j >> 2) + 4 * hh][n] = w2n * hv[j];
        }
        __syncthreads();
        {   // output unit: thread = (row, eighth of the hidden layer); δ, coef, g of the row
            const int row = tid >> 3, e8 = tid & 7;
            float sum = 0.0f;
#pragma unroll
            for (int k = 0; k < N_HID / 8; ++k) sum += sH[row][e8 * (N_HID / 8) + k];
            sum += __shfl_xor(sum, 1, 64); sum += __shfl_xor(sum, 2, 64); sum += __shfl_xor(sum, 4, 64);
            if (e8 == 0) {
                const float val = td_sigmoid(sum + b2);
                float coef = 0.0f, g = 0.0f, delta = 0.0f;
                int flag = 0;
                if (r0 + row < f.m) {
                    if (isfinite(y)) {
                        delta = y - val;
                        coef = (float)(alpha * (double)delta);
                        g = val * (1.0f - val);
                        flag = 1;
                    } else flag = 2;
                }
                sCoef[row] = coef; sG[row] = g;
                // b2, Σ δ² and the counts: this thread keeps the sums of row slot `row` over the workgroup's tiles
                accb2 = fmaf(coef, g, accb2);
                sq += (double)delta * (double)delta;
                cnt += flag == 1 ? 1 : 0;
                skipped += flag == 2 ? 1 : 0;
            }
        }
        __syncthreads();
        // ---- factors: D = coef · db1 (the gradient product's B operand), the b1 | W2 sums of this lane's 16 rows ----
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int row = (j & 3) + 8 * (j >> 2) + 4 * hh;
            const float cf = sCoef[row], gg = sG[row], hx = hv[j];
            const float db1 = (gg * w2n) * (1.0f - hx) * hx;
            sH[row][n] = cf * db1;
            accb1 = fmaf(cf, db1, accb1);
            accw2 = fmaf(cf, gg * hx, accw2);
        }
        __syncthreads();
        // ---- gradient: [32 features x 32 rows] · [32 rows x 32 units] for the seven feature tiles ----
#pragma unroll
        for (int s = 0; s < FIT_TILE / 2; ++s) {
            const float b = sH[2 * s + hh][n];
#pragma unroll
            for (int ft = 0; ft < FIT_FT; ++ft) gacc[ft] = __builtin_amdgcn_mfma_f32_32x32x2f32(sX[2 * s + hh][32 * ft + r], b, gacc[ft], 0, 0, 0);
        }
    }
    // ---- the workgroup's row of partial sums, internal order: accumulator j of tile ft = feature 32 ft + (j & 3) + 8 (j >> 2) + 4 hh, unit n ----
    float *pr = f.partial + (long long)blockIdx.x * TD_LD;
#pragma unroll
    for (int ft = 0; ft < FIT_FT; ++ft)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int feat = 32 * ft + (j & 3) + 8 * (j >> 2) + 4 * hh;
            if (feat < N_IN) pr[feat * N_HID + n] = gacc[ft][j];
        }
    accb1 += __shfl_xor(accb1, 32, 64);
    accw2 += __shfl_xor(accw2, 32, 64);
    if (hh == 0) { pr[TD_OFF_B1 + n] = accb1; pr[TD_OFF_W2 + n] = accw2; }
    // the 32 row slots (threads 0, 8, ..., 248) meet in LDS: pairwise in a fixed order, five levels (sCoef is free: every thread is
    // past the barrier behind the last tile's factors)
    if ((tid & 7) == 0) { sCoef[tid >> 3] = accb2; sSq[tid >> 3] = sq; sCnt[tid >> 3][0] = cnt; sCnt[tid >> 3][1] = skipped; }
    __syncthreads();
    if (tid == 0) {
        for (int st = 1; st < FIT_TILE; st *= 2)
            for (int i = 0; i < FIT_TILE; i += 2 * st) {
                sCoef[i] += sCoef[i + st]; sSq[i] += sSq[i + st];
                sCnt[i][0] += sCnt[i + st][0]; sCnt[i][1] += sCnt[i + st][1];
            }
        pr[TD_OFF_B2] = sCoef[0];
        f.part_sq[blockIdx.x] = sSq[0];
        f.part_cnt[2 * blockIdx.x] = sCnt[0][0];
        f.part_cnt[2 * blockIdx.x + 1] = sCnt[0][1];
    }
}

// td_reduce_kernel's sum over the n_groups partial rows, in its order, plus the chunks before this one (`run`, internal order).  The
// last chunk hands the update out (upd, parameter order) or applies it with the refresh of w1t and wl3; block 0 adds the chunk's Σ δ²
// and row counts to the running statistics (stat_sq[0], stat_cnt[0 .. 1]) on one thread, in workgroup order.
__global__ __launch_bounds__(256) void fit_reduce_kernel(TdView v, int n_groups, float *run, int first, int last, float *upd, int apply,
                                                         const double *part_sq, const long long *part_cnt, double *stat_sq, long long *stat_cnt)
{
    __shared__ td_f32x4 red[16][16];
    const int p4 = threadIdx.x & 15, gl = threadIdx.x >> 4;
    const int q0 = blockIdx.x * 64 + p4 * 4;
    td_f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int g = gl; g < n_groups; g += 16) s += *reinterpret_cast<const td_f32x4 *>(v.partial + (long long)g * TD_LD + q0);
    red[gl][p4] = s;
    __syncthreads();
    if (threadIdx.x < 64) {
        const int q = blockIdx.x * 64 + threadIdx.x;
        const int f4 = threadIdx.x >> 2, e = threadIdx.x & 3;
        float u = 0.0f;
#pragma unroll
        for (int g = 0; g < 16; ++g) u += red[g][f4][e];
        if (q < TD_P) {
            if (!first) u = run[q] + u;
            if (!last) run[q] = u;
            else {
                const int p = td_param_of_internal(q);
                if (upd) upd[p] = u;
                if (apply) {
                    const float th = v.theta[p] + u;
                    v.theta[p] = th;
                    if (q < TD_OFF_B1) {
                        v.w1t[q] = th;
                        root3_store_weight(v.wl3, q & (N_HID - 1), q >> 7, th);
                    }
                }
            }
        }
    } else if (blockIdx.x == 0 && threadIdx.x == 64) {
        double sq = 0.0;
        long long cnt = 0, skipped = 0;
        for (int g = 0; g < n_groups; ++g) { sq += part_sq[g]; cnt += part_cnt[2 * g]; skipped += part_cnt[2 * g + 1]; }
        stat_sq[0] += sq;
        stat_cnt[0] += cnt;
        stat_cnt[1] += skipped;
    }
}

}  // namespace bg
