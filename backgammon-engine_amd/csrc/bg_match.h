// bg_match.h -- match play on the cubeful rollouts (bgamd_env_rollout_match, include/bgamd.h): the cube overlay of bg_cube.h with the
// thresholds of a match score, and a trial's worth as a match-winning chance (MWC).  The kernels live in bgamd_cube.hip beside the
// cube's, in the library's third code object; the cube's five kernels keep their code.  bg_match_plan.h (plain C++) holds the setting's
// validation, the threshold table and the sizes.  Everything is passed as raw pointers.
//
// THE RULE, restated (include/bgamd.h states it).  fp64, every operation rounded on its own.
//   after(a1, a2, state), the MWC of the side needing a1 against the side needing a2 when the next game starts, first case that applies:
//     a1 <= 0: 1.0;  a2 <= 0: 0.0;  state != 0 and a2 == 1: met_pc[a1-1];  state != 0 and a1 == 1: 1.0 - met_pc[a2-1];  else met[a1-1][a2-1].
//   A cube decision before turn k: the cube record's conditions, and not the Crawford game (state 1), and c < the roller's away (else
//   the cube is dead: the trial is marked in its record's spare word, bit 0).  Then double_at and pass_at are the table's entry for
//   (state, c, the roller's away a, the opponent's away b), computed on the host from the ROLLER's row of the table:
//     W(k) = after(a - k, b, state), L(k) = after(a, b - k, state); W1 = W(c), L1 = L(c), W2 = W(2c), L2 = L(2c);
//     pass_at = (W1 - L2) / (W2 - L2);  open = (L1 - L2) / ((L1 - L2) + (W2 - W1));  double_at = open + window_share (pass_at - open);
//     a denominator <= 0 or a result that is not finite: double_at = +inf, no decision.
//   The roller doubles iff double_at <= w <= too_good_at, the opponent passes iff w > pass_at, as in bg_cube.h.
//   Payoff (PLAYER1's MWC, PLAYER1's row): r = +-c of a drop (c before the double) or c x points of a finished trial,
//     mwc = after(a1 - max(r, 0), a2 - max(-r, 0), state) in 64-bit integers; truncated with fp32 value x:
//     mwc = dadd(dmul(x, after(a1 - c, a2, state)), dmul(dsub(1, x), after(a1, a2 - c, state))).
//
//   intake   intake (thread per position)  : away1 | away2 << 8 | state << 16 into the env's copy; a bad entry sets err_bit
//   start    init (thread per trial)       : cube::init with the match's conditions and the table's thresholds
//   loop     turn (thread per trial lane)  : cube::turn likewise, launched in its place; the same record, one writer, the same two counters
//   read     reduce (wave per position)    : per-trial MWC (kept in an env buffer: the paired read's which = 4, by cube::paired), mean and
//                                            stderr in ro_reduce_kernel's fixed order, three counts
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bg_cube.h"

namespace bg {
namespace match {

constexpr uint32_t TRIAL_DEAD = 1u;                    // Trial::spare bit 0: some decision of the trial was withheld by a dead cube
constexpr unsigned long long ERRF_RO_MATCH = 1024;     // intake word, beside ERRF_RO_CUBE (512): a bad entry of the match's score tables

// the uploaded block of a setting (bg_match_plan.h, Layout), as device pointers
struct Table {
    const double *met, *met_pc;                        // [M][M], [M]
    const double2 *thr;                                // [2][levels][M][M]: {double_at, pass_at}
    int M, levels;
};

void intake(hipStream_t s, long long P, int M, const int32_t *d_away1, const int32_t *d_away2, const int32_t *d_state, uint32_t *words,
            unsigned long long *err_word, unsigned long long err_bit);
void init(hipStream_t s, long long N, long long T, int rotate, const uint4 *pos_rows, const uint32_t *start, long long P, const double *mean0,
          cube::Rule rule, Table tab, const uint32_t *words, cube::Trial *trials);
void turn(hipStream_t s, long long L, long long T, const uint32_t *meta, const uint32_t *ply, const uint32_t *lane_trial, const float *f,
          cube::Rule rule, Table tab, const uint32_t *words, cube::Trial *trials, unsigned long long *ctr);
// counts [P][3]: trials that ended the match for PLAYER1, for PLAYER2, trials with a decision withheld by a dead cube
void reduce(hipStream_t s, long long P, long long T, const float *t_val, const uint32_t *t_turns, const cube::Trial *trials, Table tab,
            const uint32_t *words, double *t_mwc, double *mean, double *serr, int64_t *counts, double *o_mwc);

}  // namespace match
}  // namespace bg
