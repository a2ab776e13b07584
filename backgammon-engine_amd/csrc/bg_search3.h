// bg_search3.h -- the launches of the 3-ply search step (bgamd_env_step_search3, include/bgamd.h): the filtered 2-ply step of bg_filter.h,
// whose best candidates by V2 (the deep set L2) are searched one ply deeper -- the opponent answers every roll with a SEARCHED reply.
// The kernels live in bgamd_search3.hip, a translation unit and so a gfx950 code object of their own inside libbgamd.so: the code object
// of bgamd.hip -- every kernel of the greedy step, its order and its addresses -- is what it was before this step existed.
// bgamd.hip's host code (search_stages, search3_deep) calls the functions below; each is one launch on the stream.
//
//   plies 1, 2  the filtered step's stages A-D on the env's own lanes, launch for launch: kept lists, v1, V2, best[g] by V2
//   deep set    deep_select (lane per game)    : L1 ranked by (V2 for the mover, smaller key), kept by (deep_k, deep_margin): c_d3[j] = the
//                                                rank in L2 or -1, dkept[g] = |L2| when the lane is searched deeper (|L2| >= 2), else 0
//               srch_scan, deep_map            : the deep candidates as one list, entry doff[g] + rank -> candidate j
//   mid level   one MID lane per (deep candidate, opponent roll) = mid root v, on the internal mid env, a chunk of its lanes at a time.
//               Mid lane l of a chunk is mid root v0 + l = (entry v / 21 of the deep list, roll v % 21); it is LIVE when the entry exists
//               and its candidate is not terminal.
//               flt_fanout over the deep list  : position c, the opponent o to move, the roll's dice (else: a finished lane)
//               the filtered step's stages A, B on the mid env with reply_fix behind flt_select -- a live mid lane WITHOUT rows (o has no
//                                                move on a non-doubles roll) keeps one reply, the pass -- and pass_emit behind srch_emit,
//                                                which writes that reply: c with o's turn bit, key 0, v1 = the value srch_collect forms
//                                                from the root pass's hidden layer
//               the search's stage C           : EVERY kept reply, a single one too, is searched: (reply, m's roll) virtual roots, srch_fanout
//                                                over the whole reply list, scored on the scratch env, srch_collect
//               r3_reduce (lane per mid lane)  : V2 of every kept reply, the best for o into r3[v]
//   choice      v3_reduce (lane per game)      : V3 of the members of L2, arg-best for the mover into best[g] -> apply_kernel; a lane that is
//                                                not searched deeper keeps the filtered step's best[g]
//   reads       read, info
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bg {
namespace s3 {

// the deep list as a mid level reads it: *total entries, entry -> candidate (rows with the MOVER's turn bit, key | terminal << 31)
struct DeepList {
    const uint32_t *total, *map;
    const uint4 *rows;
    const uint32_t *key;
};

void deep_select(hipStream_t s, long long n, const uint32_t *kept, const uint32_t *koff, const uint4 *c_rows, const uint32_t *c_key,
                 const float *c_v2, uint32_t k_lim, float margin, int32_t *c_d3, uint32_t *dkept);
void deep_map(hipStream_t s, long long n, const uint32_t *kept, const uint32_t *koff, const uint32_t *dkept, const uint32_t *doff,
              const int32_t *c_d3, uint32_t *dmap);
// the three below: n = the mid env's lanes, v0 = the chunk's first mid root, cnt / kept / koff and c_* = the MID env's search state
void reply_fix(hipStream_t s, long long n, long long v0, DeepList deep, const uint32_t *cnt, uint32_t *kept);
void pass_emit(hipStream_t s, long long n, long long v0, DeepList deep, const uint32_t *cnt, const uint32_t *koff, const float *pass_v1,
               uint4 *c_rows, uint32_t *c_key, float *c_v1);
void r3_reduce(hipStream_t s, long long n, long long v0, DeepList deep, const uint32_t *kept, const uint32_t *koff, const uint32_t *c_key,
               const float *c_v1, const float *rval, float *c_v2, float *r3, unsigned long long *roots, unsigned long long *err,
               unsigned long long *scratch_err);
void v3_reduce(hipStream_t s, long long n, const uint32_t *kept, const uint32_t *koff, const uint32_t *dkept, const uint32_t *doff,
               const uint4 *c_rows, const uint32_t *c_key, const float *c_v1, const int32_t *c_d3, const float *r3, float *c_v3,
               unsigned long long *best, unsigned long long *err, unsigned long long *mid_err);
void read(hipStream_t s, long long n, int K, const uint32_t *kept, const uint32_t *koff, const uint32_t *dkept, const int32_t *c_d3,
          const float *c_v3, float *v3, int32_t *depth);
void info(hipStream_t s, long long n, const uint32_t *kept, const uint32_t *koff, const uint32_t *dkept, const uint32_t *c_key,
          const int32_t *c_d3, const unsigned long long *roots, unsigned long long *out);

}  // namespace s3
}  // namespace bg
