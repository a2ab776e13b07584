// bg_cube.h -- the doubling cube as an overlay on the rollout's trials (bgamd_env_rollout_cube, include/bgamd.h): the per-trial record, the
// rule, and the launches.  The kernels live in bgamd_cube.hip, a translation unit and so a gfx950 code object of their own inside
// libbgamd.so, behind bgamd_search3.hip: the code object of bgamd.hip -- every kernel of the greedy step, its order and its addresses
//  -- is what it was before the cube existed.  bgamd.hip's host code (bgamd_env_rollout_grouped and the read calls) calls the
// functions below; each is one launch on the stream.  Everything is passed as raw pointers: nothing here knows EnvView or RoView.
//
//   intake   intake (thread per position)  : the caller's start tables into the env's copy; a value that is no power of two in
//                                            1 .. 2^30 or an owner outside 0 .. 2 sets err_bit in the intake word
//   start    init (thread per trial)       : the record's start from the copy, and -- rotation, a position that is not over -- the
//                                            decision before the rotated turn 0, on the position's own pre-roll mean (none under
//                                            BGAMD_CUBE_HOLD_TURN0, here and in `turn` at ply 0)
//   loop     turn (thread per trial lane)  : right after ro_vr_luck_kernel, on the same f[lane][21]: a live lane's trial gets the decision
//                                            before the turn at hand (turn index = the lane's ply); counts lane-turns and those after a drop
//   read     reduce (wave per position)    : per-trial cubeful equity (kept in an env buffer for `paired`), cube, drop; mean and stderr in
//                                            ro_reduce_kernel's fixed order; the four counts
//            paired (wave per position)    : bgamd_env_rollout_paired_read's which = 3 on that buffer, ro_pair_reduce_kernel's rule
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bg {
namespace cube {

// One trial's record, 16 bytes, read and written as one uint4 by the one lane that plays the trial.
//   value    the cube, a power of two
//   dropped  the turn index of the drop, or -1
//   info     bits 0..1 the owner (0 centre, 1 PLAYER1, 2 PLAYER2), bits 2..3 the side that passed (0 none, 1 PLAYER1, 2 PLAYER2),
//            bits 8..31 the times the cube was turned in the trial
struct Trial {
    uint32_t value;
    int32_t dropped;
    uint32_t info;
    uint32_t spare;
};
static_assert(sizeof(Trial) == 16, "one 16-byte record per trial");
constexpr uint32_t INFO_OWNER = 3u, INFO_PASSED_SHIFT = 2, INFO_TURNS_SHIFT = 8;

// the thresholds of a call (bgamd_env_rollout_cube)
struct Rule {
    double double_at, pass_at, too_good_at;
    uint32_t max_cube;
    int jacoby;
    int hold_turn0;                                    // BGAMD_CUBE_HOLD_TURN0: no decision before turn 0 of a trial
};

// What the kernels must agree on with bg_rollout.h and bgamd.hip, restated here because those live inside bgamd.hip's anonymous
// namespace; bgamd.hip static_asserts every one against its own.
constexpr uint32_t LANE_FINISHED = 1u << 12;           // META_FINISHED
constexpr uint32_t LANE_NONE = 0xFFFFFFFFu;            // RO_NONE
constexpr uint32_t WORD_TRUNC = 1u << 30;              // RO_TRUNC
constexpr int WORD_PTS_SHIFT = 17;                     // RO_PTS_SHIFT
constexpr int ROLLS = 21;                              // SRCH_ROLLS
enum { CTR_TURNS = 0, CTR_AFTER_DROP = 1, CTR_WORDS = 2 };   // the two lane-turn counters (bgamd_env_rollout_cube_info)

void intake(hipStream_t s, long long P, const int32_t *d_value, const int32_t *d_owner, uint32_t *start, unsigned long long *err_word,
            unsigned long long err_bit);
// start [2 P], the env's copy of the tables: start[p] = the value, start[P + p] = the owner
void init(hipStream_t s, long long N, long long T, int rotate, const uint4 *pos_rows, const uint32_t *start, long long P,
          const double *mean0, Rule rule, Trial *trials);
void turn(hipStream_t s, long long L, const uint32_t *meta, const uint32_t *ply, const uint32_t *lane_trial, const float *f, Rule rule,
          Trial *trials, unsigned long long *ctr);
void reduce(hipStream_t s, long long P, long long T, const float *t_val, const uint32_t *t_turns, const Trial *trials, Rule rule,
            double *t_eq, double *mean, double *serr, int64_t *counts, double *o_eq, int32_t *o_cube, int32_t *o_dropped);
void paired(hipStream_t s, long long P, long long T, const int32_t *ref, const int32_t *group, const double *t_eq, double *diff_mean,
            double *diff_serr);

}  // namespace cube
}  // namespace bg
