// bg_vr.h -- kernels of the 1-ply pre-roll evaluation (bgamd_env_evaluate_preroll) and of the luck-adjusted rollouts
// (BGAMD_ROLLOUT_VR, include/bgamd.h).  Included by bgamd.hip inside its anonymous namespace, after the rollout's kernels.
//
//   pre-roll  per chunk of virtual lanes of the search's scratch env: pre_fanout writes (position, roll) roots -- the positions are
//             rows, or the lanes of the env that plays a rollout's trials --, the greedy step's roots / expansion / value net score
//             them there (GreedyRun, no apply), srch_collect writes f[position][roll]; pre_reduce (lane per position): finished
//             positions, the fp64 mean
//   rollout   ro_vr_init (per trial)  : every trial's luck total before its first turn on a lane (0, or its rotated turn 0's luck)
//             before every turn of a run: the pre-roll pass on the trial env's lanes, then ro_vr_luck (lane per trial lane) adds
//             f[roll] - mean of the dice the turn is played with to the lane's trial
//   read      ro_vr_reduce (wave per position) : adjusted mean and stderr in ro_reduce's fixed order; per-trial luck totals
#pragma once

// index of the unordered roll of dice (d1, d2) in srch_roll's order
__device__ __forceinline__ int pre_roll_index(int d1, int d2)
{
    const int a = d1 < d2 ? d1 : d2, b = d1 < d2 ? d2 : d1;
    return 6 * (a - 1) - (a - 1) * (a - 2) / 2 + (b - a);
}

// mean(s) = sum over the 21 rolls in order of w_r (double) f(s, r), w_r = 1/36 for a double, 2/36 otherwise: a rounded fp64 product
// and a rounded fp64 sum per roll (no fused multiply-add), as a host replays it
__device__ __forceinline__ double pre_mean(const float *__restrict__ f)
{
    double s = 0.0;
#pragma unroll
    for (int idx = 0, a = 1; a <= 6; ++a)
#pragma unroll
        for (int d = a; d <= 6; ++d, ++idx) s = __dadd_rn(s, __dmul_rn(a == d ? 1.0 / 36.0 : 2.0 / 36.0, (double)f[idx]));
    return s;
}

// virtual lane l of a chunk = v = v0 + l = (position q = v / 21, roll v % 21): the position with the side to roll's turn bit and the
// roll's dice.  Positions: rows[q], q < n (LANES false), or lane q of the env src (LANES true: n = src.n; a finished lane is no
// position).  Past the list, on a finished lane or on a position that is over: a frozen lane (no roots, no rows).
template <bool LANES>
__global__ __launch_bounds__(SRCH_NT) void pre_fanout_kernel(EnvView e, long long v0, long long n, const uint4 *__restrict__ rows, EnvView src)
{
    const long long l = (long long)blockIdx.x * SRCH_NT + threadIdx.x;
    if (l >= e.n) return;
    const long long v = v0 + l, q = v / SRCH_ROLLS;
    uint32_t p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t meta = META_FINISHED;
    if (q < n) {
        int turn;
        bool live = true;
        if (LANES) {
            const uint32_t m = src.meta[q];
            live = !(m & META_FINISHED);
            turn = (int)(m & 1u);
            load_planes(src, q, p);
        } else {
            turn = ro_unrow(rows + 2 * q, p);
        }
        if (live && !over_code(p)) {
            int d1, d2;
            srch_roll((int)(v % SRCH_ROLLS), d1, d2);
            meta = meta_pack(turn, d1, d2, false);
        }
    }
    store_planes(e, l, p);
    e.meta[l] = meta; e.ply[l] = 0; e.episode[l] = 0; e.flags[l] = 0;
}

// lane per position: a position that is over gets its outcome for every roll (into f), then mean; the 21 values and the mean go to
// o_f / o_mean when given
__global__ __launch_bounds__(SRCH_NT) void pre_reduce_kernel(long long n, const uint4 *__restrict__ rows, float *__restrict__ f,
                                                             float *__restrict__ o_f, double *__restrict__ o_mean)
{
    const long long q = (long long)blockIdx.x * SRCH_NT + threadIdx.x;
    if (q >= n) return;
    uint32_t p[8];
    ro_unrow(rows + 2 * q, p);
    float *fq = f + q * SRCH_ROLLS;
    const int oc = over_code(p);
    if (oc)
        for (int k = 0; k < SRCH_ROLLS; ++k) fq[k] = oc == 1 ? 1.0f : 0.0f;
    if (o_f)
        for (int k = 0; k < SRCH_ROLLS; ++k) o_f[q * SRCH_ROLLS + k] = fq[k];
    if (o_mean) o_mean[q] = pre_mean(fq);
}

// every trial jl = p T + i: its luck total before a lane plays a turn of it.  0.0, or -- rotation, a position that is not over -- the
// luck of turn 0, played with ordered pair i % 36: f0 / mean0 are the pre-roll evaluation of the P positions
__global__ __launch_bounds__(RO_NT) void ro_vr_init_kernel(RoView r, const float *__restrict__ f0, const double *__restrict__ mean0,
                                                           double *__restrict__ t_luck)
{
    for (long long jl = (long long)blockIdx.x * RO_NT + threadIdx.x; jl < r.N; jl += (long long)gridDim.x * RO_NT) {
        double L = 0.0;
        if (r.rotate) {
            const long long pi = jl / r.T, k = (jl % r.T) % 36;
            uint32_t p[8];
            ro_unrow(r.pos_rows + 2 * pi, p);
            if (!over_code(p)) L = L + ((double)f0[pi * SRCH_ROLLS + pre_roll_index(1 + (int)(k / 6), 1 + (int)(k % 6))] - mean0[pi]);
        }
        t_luck[jl] = L;
    }
}

// after the pre-roll pass of a turn (f[g][21] of every live lane g of the trial env): a live lane -- its trial's next turn is about to
// be played with the dice in its meta -- adds luck = (double) f[roll] - mean to that trial's total
__global__ __launch_bounds__(RO_NT) void ro_vr_luck_kernel(EnvView e, const uint32_t *__restrict__ lane_trial, const float *__restrict__ f,
                                                           double *__restrict__ t_luck)
{
    const long long g = (long long)blockIdx.x * RO_NT + threadIdx.x;
    if (g >= e.n) return;
    const uint32_t meta = e.meta[g];
    const uint32_t j = lane_trial[g];
    if ((meta & META_FINISHED) || j == RO_NONE) return;
    const float *fg = f + g * SRCH_ROLLS;
    const int k = pre_roll_index((int)((meta >> 4) & 7u), (int)((meta >> 8) & 7u));
    t_luck[j] += (double)fg[k] - pre_mean(fg);
}

// wave per position, ro_reduce's order: y_i = (double) x_i - L_i, vr_mean = (1/T) sum y_i, vr_stderr = sqrt(sum (y_i - vr_mean)^2 /
// (T (T - 1))) (0 for T = 1); the luck totals to o_luck[P][T] when given
__global__ __launch_bounds__(64) void ro_vr_reduce_kernel(long long T, const float *__restrict__ t_val, const double *__restrict__ t_luck,
                                                          double *__restrict__ mean, double *__restrict__ serr, double *__restrict__ o_luck)
{
    const long long p = blockIdx.x, base = p * T;
    const int lane = threadIdx.x;
    double s = 0.0;
    for (long long i = lane; i < T; i += 64) {
        const double L = t_luck[base + i];
        s += (double)t_val[base + i] - L;
        if (o_luck) o_luck[base + i] = L;
    }
    const double m = ro_wave_sum(s) / (double)T;
    double q = 0.0;
    for (long long i = lane; i < T; i += 64) {
        const double d = ((double)t_val[base + i] - t_luck[base + i]) - m;
        q += d * d;
    }
    q = ro_wave_sum(q);
    if (lane == 0) {
        if (mean) mean[p] = m;
        if (serr) serr[p] = T > 1 ? sqrt(q / ((double)T * (double)(T - 1))) : 0.0;
    }
}
