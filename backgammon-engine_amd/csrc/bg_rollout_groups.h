// bg_rollout_groups.h -- kernels of the grouped rollout (bgamd_env_rollout_grouped, bgamd_env_rollout_paired_read, include/bgamd.h).
// Included by bgamd.hip inside an anonymous namespace just ahead of its KERNEL_ORDER list: both are templates whose entries stand
// at that list's end, so that no other kernel of the code object moves.
//
//   intake    ro_group_intake (thread per position) : the caller's group table into the env's copy; a negative group, or one whose
//             last trial's id (group + 1) T - 1 would not fit below 2^31, sets ERRF_RO_GROUP in the intake word
//   loop      ro_refill_kernel (bg_rollout.h) reads the copy through RoView::group: the dice id of a trial is no longer its slot
//   read      ro_pair_reduce (wave per position) : paired differences against a reference position of the same group, in
//             ro_reduce_kernel's order
#pragma once

template <int NT>
__global__ __launch_bounds__(NT) void ro_group_intake_kernel(const int32_t *__restrict__ src, long long P, long long T,
                                                             int32_t *__restrict__ dst, unsigned long long *err)
{
    const long long p = (long long)blockIdx.x * NT + threadIdx.x;
    if (p >= P) return;
    const int32_t g = src[p];
    if (g < 0 || ((long long)g + 1) * T >= (1ll << 31)) atomicOr(err, (unsigned long long)ERRF_RO_GROUP);
    dst[p] = g;
}

// the per-trial quantity `which` of trial slot j: 0 the value x, 1 the luck-adjusted y = x - L, 2 the equity in points
// (ro_outcome_reduce_kernel's: the points of a trial scored from a board, 2 x - 1 of a truncated one)
__device__ __forceinline__ double ro_pair_q(int which, long long j, const float *__restrict__ t_val, const uint32_t *__restrict__ t_turns,
                                            const double *__restrict__ t_luck)
{
    const double x = (double)t_val[j];
    if (which == 1) return x - t_luck[j];
    if (which == 2) {
        const int w = ro_word_points(t_turns[j]);
        return w ? (double)w : 2.0 * x - 1.0;
    }
    return x;
}

// Wave per position p, reference r = ref[p]: d_i = q_i(p) - q_i(r) over the T trials, lane k takes trials k, k + 64, ...; then
// ro_wave_sum's butterfly; lane 0 writes.  group NULL: the identity table (an ungrouped rollout).  r outside [0, P) or in another
// group: NaN, NaN -- nothing of r is read.
template <int NT>
__global__ __launch_bounds__(NT) void ro_pair_reduce_kernel(long long P, long long T, int which, const int32_t *__restrict__ ref,
                                                            const int32_t *__restrict__ group, const float *__restrict__ t_val,
                                                            const uint32_t *__restrict__ t_turns, const double *__restrict__ t_luck,
                                                            double *__restrict__ diff_mean, double *__restrict__ diff_serr)
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
    for (long long i = lane; i < T; i += 64)
        s += ro_pair_q(which, bp + i, t_val, t_turns, t_luck) - ro_pair_q(which, br + i, t_val, t_turns, t_luck);
    const double m = ro_wave_sum(s) / (double)T;
    double q = 0.0;
    for (long long i = lane; i < T; i += 64) {
        const double d = (ro_pair_q(which, bp + i, t_val, t_turns, t_luck) - ro_pair_q(which, br + i, t_val, t_turns, t_luck)) - m;
        q += d * d;
    }
    q = ro_wave_sum(q);
    if (lane == 0) {
        if (diff_mean) diff_mean[p] = m;
        if (diff_serr) diff_serr[p] = T > 1 ? sqrt(q / ((double)T * (double)(T - 1))) : 0.0;
    }
}
