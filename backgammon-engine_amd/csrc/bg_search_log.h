// bg_search_log.h -- the search log's pass (bgamd_env_set_search_log, include/bgamd.h): what a 2-ply search step of either kind decided,
// turn by turn, as (pre-move row, played afterstate, V2 of the played candidate, its v1).  Included by bgamd.hip inside an anonymous
// namespace just ahead of its KERNEL_ORDER list, which places the kernel behind the earlier ones.
//
//   srch_log (lane per game) : between stage D's reduce (sv.best[g] holds the winner, c_v2 every kept candidate's V2) and apply_kernel,
//                              which moves the lane -- so the lane's meta / ply and sv.root_rows are still those of the step's start
// Launched only while a log is set: a search step without one issues the launches it always issued.  The kernel is a template: its code
// is emitted behind the other kernels', whose addresses stay where they were.
#pragma once

// Per lane: live and taking part exactly as lane_begin decides it (not past the env, not finished, not left out by BGAMD_ONLY_P1/P2), ply
// below the log's length.  Such a lane writes entry ply * n + g; every other lane writes nothing.
//   rows   sv.root_rows[g]: the row the greedy step's trajectory log would hold for this turn (stage A wrote it for every lane)
//   after  the played candidate's row with the turn bit of the side that did NOT move (c_rows holds the mover's); without a move the
//          lane's own board with that bit
//   target V2 of the played candidate where the lane was searched (kept >= min_searched: 1 after a plain step, 2 after a filtered one),
//          else a quiet NaN
//   v1     the played candidate's 1-ply value (a terminal candidate: its exact outcome); without a move a quiet NaN
// The played candidate is the one of the lane's <= K kept candidates whose key is the winner's (best[g] = (ordered V2 bits, ~key); the keys
// of a lane's distinct rows differ).  Plain vector stores: 2 x uint4 per row, one dword per float; a NULL buffer is skipped.
template <int NT>
__global__ __launch_bounds__(NT) void srch_log_kernel(EnvView e, int flags, const uint4 *__restrict__ root_rows,
                                                      const unsigned long long *__restrict__ best, const uint32_t *__restrict__ kept,
                                                      const uint32_t *__restrict__ koff, const uint4 *__restrict__ c_rows,
                                                      const uint32_t *__restrict__ c_key, const float *__restrict__ c_v1,
                                                      const float *__restrict__ c_v2, uint32_t min_searched, SearchLog lg)
{
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    if (g >= e.n) return;
    const uint32_t meta = e.meta[g];
    if (meta & META_FINISHED) return;
    const int turn = meta & 1;
    if (((flags & BGAMD_ONLY_P1) && turn != 0) || ((flags & BGAMD_ONLY_P2) && turn != 1)) return;
    const long long ply = (long long)e.ply[g];
    if (ply >= lg.plies) return;
    const long long t = ply * e.n + g;

    const uint4 r0 = root_rows[2 * g], r1 = root_rows[2 * g + 1];
    const unsigned long long pack = best[g];
    const uint32_t k = kept[g];
    long long played = -1;                                 // the played candidate's place in the list; -1: the lane had no move
    if (pack != 0ull) {
        const uint32_t key = ~(uint32_t)pack & 0x7FFFFFFFu, j0 = koff[g];
        for (uint32_t i = 0; i < k && played < 0; ++i)
            if ((c_key[(long long)j0 + i] & 0x7FFFFFFFu) == key) played = (long long)j0 + i;
    }
    const bool has = played >= 0;
    uint32_t p[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};         // (words, not uint4s: a uint4 assigned under a branch
    float v1 = __uint_as_float(0x7FC00000u), target = __uint_as_float(0x7FC00000u);   //  was kept in memory by the compiler)
    if (has) {
        const uint4 c0 = c_rows[2 * played], c1 = c_rows[2 * played + 1];
        p[0] = c0.x; p[1] = c0.y; p[2] = c0.z; p[3] = c0.w; p[4] = c1.x; p[5] = c1.y; p[6] = c1.z; p[7] = c1.w;
        v1 = c_v1[played];
        if (k >= min_searched) target = c_v2[played];
    }
    p[0] = (p[0] & ~TURN_BIT) | (turn ? 0u : TURN_BIT);
    lg.rows[2 * t] = r0;
    lg.rows[2 * t + 1] = r1;
    if (lg.after) { lg.after[2 * t] = make_uint4(p[0], p[1], p[2], p[3]); lg.after[2 * t + 1] = make_uint4(p[4], p[5], p[6], p[7]); }
    if (lg.target) lg.target[t] = target;
    if (lg.v1) lg.v1[t] = v1;
}
