/* bgamd.h -- C ABI of the MI355X-native batched backgammon env step (libbgamd.so).
 *
 * This is the drop-in boundary for ONE hot path of romanoshiliarhopoulos/Backgammon-Engine:
 * the self-play env step.  Each entry point names the reference interface it replaces
 * (paths relative to the reference root).  The reference crosses Python<->C++ through the
 * pybind11 module `backgammon_env` (cppsrc/backgammon_bindings.cpp:41-94); a maintainer binds
 * these symbols instead (ctypes stub in INTEGRATION.md, shipped as
 * backgammon-engine_amd/backgammon_env/).
 *
 * Conventions
 *   - plain C, no torch types.  Every `d_*` pointer is a DEVICE pointer owned by the caller
 *     (e.g. torch.Tensor.data_ptr()); `h_*` pointers are host pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  All work is
 *     stream-ordered; nothing synchronises unless stated.
 *   - return value: 0 = ok, negative = BGAMD_E_* (bgamd_error_string()).
 *   - a state is int32[28] = [board24 (+P1/-P2), bar1, bar2, off1, off2]   (game.hpp:16-28);
 *     |count| <= 15.  turn: 0 = PLAYER1, 1 = PLAYER2 (player.hpp:14-18).
 *   - one host thread drives one env; one env lives on one device.
 *   - history rule: the outputs of a call are a function of its arguments and of the env's documented state -- lanes (boards, side
 *     to move), dice, ply and episode, seed, the weights of both slots, the settings in force (logs, rollout policy, cube, kernel
 *     timing) and the counters.  They do not depend on which calls came before, at which sizes, or whether those calls succeeded:
 *     the internal envs and the buffers an env grows on first use are kept between calls, and nothing may be read from them that
 *     the call at hand did not write.  A read call (`*_read`, `*_info`, bgamd_env_last_choice) either returns what its own call
 *     left, bit for bit, however many other calls came in between, or is refused with its documented code.
 */
#ifndef BGAMD_H
#define BGAMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bgamd_env bgamd_env;

enum {
    BGAMD_OK = 0,
    BGAMD_E_INVALID = -1,     /* bad argument                                         */
    BGAMD_E_HIP = -2,         /* a HIP runtime call failed (see bgamd_last_hip_error) */
    BGAMD_E_NODEVICE = -3,    /* no usable gfx950 device                              */
    BGAMD_E_ARENA = -4,       /* candidate arena overflow (raise arena_rows)          */
    BGAMD_E_STATE = -5,       /* a state had |count| > 15                             */
    BGAMD_E_NOWEIGHTS = -6,   /* greedy step / evaluate before bgamd_env_load_weights */
    BGAMD_E_DELTA = -7,       /* an afterstate differed from its root position in more features than a legal turn
                                 can change (incremental value net): the rows handed to it are not afterstates  */
    BGAMD_E_WEIGHTS = -8      /* a weight is not finite, or an fc1 weight does not fit the f16 hi + lo planes of the value
                                 net's root pass (|w| >= 65 504): nothing was loaded                            */
};

/* step flags */
enum {
    BGAMD_ROLL = 1,           /* draw this turn's dice from the Philox stream (Game::rollDice,
                                 game.cpp:665-670); without it the dice set by
                                 bgamd_env_set_dice are used (Game::setDice, game.cpp:9-12)     */
    BGAMD_AUTO_RESET = 2,     /* a finished game restarts (new episode, opening roll);
                                 without it a finished game stays finished and is skipped      */
    BGAMD_NO_FLIP = 4,        /* do not flip the turn / advance ply (make_move semantics,
                                 model.py:180-222, for the scalar Game surface)                */
    BGAMD_WANT_INDEX = 8,     /* greedy step: also report the chosen move's index into the
                                 reference-order list and the list length (walks the whole list
                                 per lane: parity/debug use, not the throughput path)           */
    BGAMD_ONLY_P1 = 16,       /* only lanes with PLAYER1 / PLAYER2 to move take part in this call  */
    BGAMD_ONLY_P2 = 32,       /*   (head-to-head play of two policies, train.py:262-277)           */
    BGAMD_WEIGHTS_SLOT1 = 64, /* greedy step evaluates with weight slot 1 instead of slot 0        */
    BGAMD_ROLLOUT_ROTATE = 128, /* bgamd_env_rollout: trial i's first turn uses ordered dice pair i mod 36 */
    BGAMD_ROLLOUT_VR = 256    /* bgamd_env_rollout: also compute luck-adjusted results, read with bgamd_env_rollout_vr_read */
};

/* value-net arithmetic.  F32: fp32-grade values (inside the 1e-5 parity bound, measured 1.8e-7).  In a greedy step the
 * hidden layer is evaluated INCREMENTALLY: one dense pass per game for the root position (W1 split exactly into three
 * bf16 terms on v_mfma_f32_32x32x16_bf16, fp32 accumulation; BGAMD_ROOT_F32=1 at env creation: the f32 MFMA chain
 * v_mfma_f32_32x32x2_f32 instead), then  a_row = a_root + Σ Δx_f · W1[:, f]  in fp32 FMAs over the few features an
 * afterstate changes (same real sum as the dense chain, different association, values agree to ~1e-7).
 * BGAMD_MFMA_DELTA=1 at env creation: that sum on v_mfma_f32_32x32x16_f16 over a K-compacted fixed-point W table
 * instead (csrc/bg_eval_mfma.h: exact sums, values within 1.4e-6; measured slower, opt-in).  F32_DENSE: the dense MFMA chain over every afterstate (what bgamd_evaluate always uses).  F16X2: W1 split into f16 hi + lo
 * (22 mantissa bits), exact products, fp32 accumulation on v_mfma_f32_32x32x16_f16 -- fp32-grade values (inside
 * the 1e-5 parity bound) on the fast matrix pipe.  BF16: single bf16 weights, speed mode outside the bound. */
enum { BGAMD_F32 = 0, BGAMD_BF16 = 1, BGAMD_F16X2 = 2, BGAMD_F32_DENSE = 3 };

int bgamd_version(void);
/* hex digest of the sources (csrc + this header) the library was compiled from: the Python binding compares it with
 * the sources on disk and refuses a stale build; bench.py prints it */
const char *bgamd_source_hash(void);
const char *bgamd_error_string(int code);
const char *bgamd_last_hip_error(void);
int bgamd_device_count(void);

/* ---- env lifetime ---------------------------------------------------------------------
 * Replaces: Game::Game(int) game.cpp:44-56 for n_games boards at once.
 * Lane g plays game_id = lane_offset + g + episode * lane_stride; dice/choice words are
 * Philox4x32-10(key = seed, counter = (game_id, ply, stream)) so a shard's games do not
 * depend on how many shards there are.  arena_rows = capacity of the candidate arena
 * (0 = default 256 rows per game, min 65 536).  The greedy step with the incremental value net (BGAMD_F32) uses it as four
 * arenas of arena_rows / 4 (non-doubles / doubles turn x no blot hit / hit): BGAMD_E_ARENA is raised when ONE of them runs
 * over in a step -- the distinct afterstates of a step average 17 per game over all four, 64 per game and arena are the default. */
int bgamd_env_create(bgamd_env **out, int64_t n_games, int device, uint64_t seed,
                     uint64_t lane_offset, uint64_t lane_stride, int64_t arena_rows);
int bgamd_env_destroy(bgamd_env *env);
int64_t bgamd_env_num_games(const bgamd_env *env);

/* All lanes: episode 0, ply 0, start position (Game::populateBoard game.cpp:240-252), turn from
 * the opening roll protocol of play_game (train.py:89-97) on the OPENING stream. */
int bgamd_env_reset(bgamd_env *env, void *stream);
/* The same for episode `episode` of every lane (game_id = lane_offset + lane + episode * lane_stride): a training
 * loop that plays one game per lane and round gives every round fresh dice this way -- play_game draws new dice for
 * every game (train.py:64-121, 527-547).  Counters are kept. */
int bgamd_env_reset_episode(bgamd_env *env, uint32_t episode, void *stream);
/* Gives an existing env the dice streams a freshly created one would have (seed, lane_offset, lane_stride as in
 * bgamd_env_create; lane_stride 0 = n_games) and resets it to episode 0.  Pooled one-lane envs of the scalar Game surface
 * (the reference constructs a Game per candidate, game.cpp:68-77) are re-seeded with it, so set_seed() decides the dice of
 * every Game created afterwards whether its env is new or comes from the pool. */
int bgamd_env_reseed(bgamd_env *env, uint64_t seed, uint64_t lane_offset, uint64_t lane_stride, void *stream);
/* Only the lanes with d_mask[g] != 0 restart, as the next episode of that lane (start position, opening roll of
 * the next global game id) -- what BGAMD_AUTO_RESET does for a finished game, on demand. */
int bgamd_env_reset_lanes(bgamd_env *env, const int32_t *d_mask /*[n]*/, void *stream);

/* ---- state access (getGameBoard/getJailedCount/getBornOffCount/getTurn/setGameBoard/
 *      setBorneOffPieces/setTurn, bindings.cpp:64-85) ------------------------------------- */
int bgamd_env_set_states(bgamd_env *env, const int32_t *d_states28, const int32_t *d_turn, void *stream);
int bgamd_env_get_states(bgamd_env *env, int32_t *d_states28, int32_t *d_turn, void *stream);
/* is_game_over (bindings.cpp:11-16) on the current boards: bit0 = over, bit1 = winner (0/1),
 * bit2 = lane frozen (finished without AUTO_RESET); bits4-5 = over/winner flags of the last step
 * (set even when the lane was auto-reset). d_states28 may be NULL in set_states (turn only). */
int bgamd_env_get_flags(bgamd_env *env, int32_t *d_flags, void *stream);
/* everything the scalar getters of bindings.cpp:64-93 read, in ONE launch: d_out[n][32] = state28 | turn | die1 | die2 |
 * flags (as bgamd_env_get_flags) */
int bgamd_env_snapshot(bgamd_env *env, int32_t *d_out, void *stream);
int bgamd_env_set_dice(bgamd_env *env, const int32_t *d_dice /*[n,2]*/, void *stream);   /* setDice      */
int bgamd_env_get_dice(bgamd_env *env, int32_t *d_dice /*[n,2]*/, void *stream);         /* get_last_dice */
/* roll_dice: dice of (game_id, ply) on the TURN stream; advance_ply != 0 post-increments ply so that
 * repeated calls draw fresh dice (the scalar Game surface), 0 leaves ply to the step functions. */
int bgamd_env_roll(bgamd_env *env, int advance_ply, void *stream);

/* ---- the scalar Game surface with HOST arguments, for ONE-LANE envs (n_games == 1): what a compiled binding of the
 * reference's module calls per method of bindings.cpp:62-93 (backgammon-engine_amd/pybind/backgammon_env_pybind.cpp is that
 * binding; the Python package's Game uses the same entry points).  Plain ints and host pointers in and out; each call
 * stages its arguments on the device, runs the same kernels as the vectorised entry points and synchronises.
 *   snapshot   : h_out[32] = state28 | turn | die1 | die2 | flags (as bgamd_env_get_flags)  -- getGameBoard, getTurn,
 *                getJailedCount, getBornOffCount, get_last_dice, is_game_over
 *   set_state  : h_state28 (or NULL = keep the board) and turn (-1 = keep)                    -- setGameBoard, setBorneOffPieces, setTurn
 *   set_dice / roll (roll draws the lane's next Philox dice and returns them)                -- setDice, roll_dice
 *   legal_moves: returns the number of (origin, dest) pairs written to h_pairs[26][2]         -- legalMoves (game.cpp:80-105)
 *   try_move   : returns 0 = moved, 1..7 = the reference's message in source order            -- tryMove (game.cpp:573-663)
 *   enumerate  : returns the number C of sequences of legalTurnSequences / evaluateTurnSequences (game.cpp:134-222) in
 *                reference order and fills the first min(C, cap) rows of h_states28[.][28], h_seq[.][4][2], h_len[.]
 *                (any may be NULL); call with cap = 0 for the count alone */
int bgamd_game_snapshot(bgamd_env *env, int32_t h_out[32]);
int bgamd_game_set_state(bgamd_env *env, const int32_t *h_state28, int turn);
int bgamd_game_set_dice(bgamd_env *env, int d1, int d2);
int bgamd_game_roll(bgamd_env *env, int32_t h_dice[2]);
int bgamd_game_legal_moves(bgamd_env *env, int player, int die, int8_t *h_pairs);
int bgamd_game_try_move(bgamd_env *env, int player, int dice, int origin, int dest);
int64_t bgamd_game_enumerate(bgamd_env *env, int player, int d1, int d2, int32_t *h_states28, int8_t *h_seq, int32_t *h_len,
                             int64_t cap);

/* ---- enumeration: Game::evaluateTurnSequences for every lane (game.cpp:193-222) -----------
 * Fills the env's candidate arena in REFERENCE ORDER (duplicates kept) for the lanes' current
 * turn and dice, or for the explicit (player, d1, d2) arguments of the reference call.  Afterwards:
 *   bgamd_env_candidates_info : d_offsets[n] (first row of lane g), d_counts[n]; returns total rows
 *                               (synchronises the stream)
 *   bgamd_env_candidates_read : rows [first, first+n_rows) unpacked to int32 states [n_rows,28] and
 *                               int8 sequences [n_rows,4,2] ((origin,dest), -1 padded), lengths. */
int bgamd_env_enumerate(bgamd_env *env, const int32_t *d_player /*[n] or NULL*/, const int32_t *d_dice /*[n,2] or NULL*/,
                        void *stream);
int64_t bgamd_env_candidates_info(bgamd_env *env, int64_t *d_offsets, int32_t *d_counts, void *stream);
int bgamd_env_candidates_read(bgamd_env *env, int64_t first, int64_t n_rows, int32_t *d_states28,
                              int8_t *d_seq, int32_t *d_seq_len, void *stream);

/* ---- the env step ---------------------------------------------------------------------------
 * One turn of every live lane: (roll) -> enumerate -> choose -> apply -> terminal check ->
 * (auto-reset | flip turn), i.e. the body of play_game's loop (train.py:103-121).
 *   random: uniform over the reference-order list, k = (u32 * C) >> 32 with u32 from d_choice_u32
 *           (per lane) or, when NULL, from the Philox TURN stream         (benchmark.py:54-61)
 *   greedy: TDLGammonModel.make_move (model.py:180-222): value net on every afterstate with the
 *           MOVER's turn bit, argmax (P1) / argmin (P2), first index wins ties; epsilon > 0 draws
 *           the exploration test and index from the TURN stream.  precision BGAMD_F32 | BGAMD_BF16.
 * Per-lane results of the last step: chosen reference-order index (-1 = no move), sequence, candidate
 * count, value of the chosen afterstate.  The greedy step reports index and count exactly only with
 * BGAMD_WANT_INDEX; without it index is 0 and count 1 when a move was made (-1 / 0 when none was). */
int bgamd_env_step_random(bgamd_env *env, int flags, const uint32_t *d_choice_u32, void *stream);
/* same result through the one-lane-per-game walk of the whole sequence tree (slow tail; cross-check) */
int bgamd_env_step_random_walk(bgamd_env *env, int flags, const uint32_t *d_choice_u32, void *stream);
int bgamd_env_load_weights(bgamd_env *env, const float *h_weights /* 25601: W1[128][198] b1 W2 b2 */);   /* slot 0 */
int bgamd_env_load_weights_slot(bgamd_env *env, int slot /* 0 | 1 */, const float *h_weights);
/* host only (no device needed): would bgamd_env_load_weights accept these 25 601 floats?  BGAMD_OK | BGAMD_E_WEIGHTS.  The reference's
 * model takes any fp32 state_dict (model.py:36-37); the value net's root pass here multiplies fc1.weight as f16 hi + f16 lo planes, exact
 * for 22 mantissa bits up to |w| < 65 504 -- a table beyond that (a diverged run) is refused loudly instead of evaluated as NaN. */
int bgamd_weights_check(const float *h_weights);
int bgamd_env_step_greedy(bgamd_env *env, int flags, float epsilon, int precision, void *stream);
/* n_steps greedy steps back to back (the loop body of play_game, train.py:103-121, n_steps times for every lane),
 * identical in effect to n_steps calls of bgamd_env_step_greedy; between two steps of a run the apply of one and the
 * roots of the next share a launch. */
int bgamd_env_run_greedy(bgamd_env *env, int flags, float epsilon, int precision, int64_t n_steps, void *stream);
int bgamd_env_last_choice(bgamd_env *env, int32_t *d_chosen, int32_t *d_count, int8_t *d_seq /*[n,4,2]*/,
                          int32_t *d_seq_len, float *d_value, void *stream);

/* ---- the temperature-sampled step: a move drawn with probability ~ exp(value / T) over the afterstates the net has scored ---------------
 * A greedy step in which a lane with a move, mover m, plays a SAMPLED afterstate instead of its best one.  The rule, for temperature T > 0:
 *   - candidates: the rows the value net evaluated for the lane (what bgamd_env_unique_rows_info / _read list).  Two rows that hold the
 *     same afterstate under two keys (about 3 % of the rows) count as ONE candidate;
 *   - mover-side value: a_i = v_i for PLAYER1, -v_i for PLAYER2, of the stored fp32 value v_i; a_best the same of the lane's best row (the
 *     greedy step's choice); d_i = a_i - a_best <= 0, one fp32 subtraction;
 *   - the draw is Gumbel-max: row i gets u_i in (0, 1) and the score  s_i = d_i / T + g_i,  g_i = -log(-log(u_i)),  formed in fp32 as
 *     q = d_i / T (IEEE division), L1 = logf(u_i), L2 = logf(-L1), s_i = q - L2.  The lane plays the row with the largest score; on
 *     bit-equal scores the smallest key (the earliest reference-order index), the greedy step's tie rule.  Because d / T is used and not
 *     a / T, every finite T > 0 is safe: the best row scores 0 + g, the others go to -inf at worst, no NaN arises.  As T -> 0 the step
 *     becomes the greedy step (up to the choice among rows whose values are bit-equal to the best);
 *   - u_i is a counter-based function of (env seed, game id, ply, the row's eight 32-bit plane words with the turn bit cleared) and of
 *     nothing else -- not of the key, the row's place, the lane count or the launch.  With P = Philox4x32-10 and key = (seed_lo, seed_hi)
 *     unless stated:  A = P(counter = row[0..3]);  B = P(counter = row[4..7] ^ A);  C = P(counter = (gid_lo, gid_hi, ply, 2), key = (B.x,
 *     B.y)) -- 2 is the SAMPLE stream, beside TURN = 0 and OPENING = 1 --;  u = (2 (C.x >> 9) + 1) 2^-24.  (23 random bits and a half, so
 *     that every u is an fp32 number: 2^-24 <= u <= 1 - 2^-24.)  Rows holding the same afterstate therefore draw the same u, score
 *     bit-equal and fall to the tie rule: the distribution is exactly softmax(a / T) over the DISTINCT afterstates;
 *   - T = 0 is the greedy step itself: the same launches, bit-identical results.  T < 0, NaN or +inf: BGAMD_E_INVALID.  There is no
 *     epsilon: the sampled entry points do not explore uniformly;
 *   - everything else is the greedy step: a lane without a move, a lane that does not take part and a finished lane keep what they keep
 *     there; bgamd_env_last_choice reports the SAMPLED row's sequence and value; every flag, both weight slots, every precision, the
 *     trajectory log and ring and bgamd_env_stats work unchanged.
 * Two small passes over the evaluated rows run between the value net and the apply (csrc/bg_sample.h); their scratch is allocated by the
 * first sampled step.  The 2-ply search, the rollouts and the analysis never sample. */
int bgamd_env_step_sampled(bgamd_env *env, int flags, float temperature, int precision, void *stream);
/* n_steps sampled steps back to back, as bgamd_env_run_greedy: the same games as n_steps calls of bgamd_env_step_sampled */
int bgamd_env_run_sampled(bgamd_env *env, int flags, float temperature, int precision, int64_t n_steps, void *stream);
/* Host values of the last call of either with T > 0 (summed over a run's steps; SYNCHRONISES that call's stream): h_out[0] lanes that had
 * a move, h_out[1] of those the lanes that left the arg-max: the value of the row they played is not bit-equal to their best value.
 * BGAMD_E_INVALID before the first such call. */
int bgamd_env_sample_info(bgamd_env *env, int64_t h_out[2]);

/* ---- 2-ply expectimax move search (TD-Gammon's 2-ply) -------------------------------------------------------------------------
 * One searched turn for every live lane that takes part (flags: BGAMD_ROLL, BGAMD_AUTO_RESET, BGAMD_NO_FLIP, BGAMD_WANT_INDEX,
 * BGAMD_ONLY_P1/P2 and BGAMD_WEIGHTS_SLOT1 mean what they mean for the greedy step; no epsilon; the F32 incremental value net only):
 *   1. roll and enumerate exactly as the greedy step does (same Philox stream, mover, weight slot);
 *   2. v1(c) of every distinct afterstate c: the greedy step's value, bit for bit (mover's turn bit) -- except a TERMINAL c (the
 *      mover has borne off the 15th checker), which scores its outcome exactly: 1.0 if PLAYER1 won, 0.0 if PLAYER2 won;
 *   3. keep the top_k best by v1 for the mover (copies of one afterstate count once; ties: the smaller key = the earlier
 *      reference-order index, the greedy step's rule); top_k = 0 keeps every distinct afterstate;
 *   4. V2(c) = v1(c) for a terminal c; otherwise  V2(c) = sum over the 21 unordered opponent rolls r = (1,1), (1,2), ..., (6,6), in that
 *      order, of w_r R(c, r), w_r = 1/36 for a double and 2/36 otherwise, where R(c, r) is the value of the reply the greedy step
 *      would choose from c (the opponent's turn bit, arg-min for PLAYER2 / arg-max for PLAYER1, no special case for terminal
 *      replies) -- or, when the opponent has no legal move, the net's value of c with the OPPONENT's turn bit.  In fp32 the sum is formed
 *      as (sum over the 6 doubles + 2 x sum over the 15 other rolls) / 36, each part in roll order: replies that are all exactly 1.0 (or
 *      0.0) give exactly 1.0 (0.0), and V2 never leaves [0, 1];
 *   5. choose the kept c with the best V2 for the mover (ties: the smaller key), then apply / terminal check / flip or auto-reset
 *      exactly as the greedy step does;
 *   6. bgamd_env_last_choice: the chosen sequence, index and count (exact with BGAMD_WANT_INDEX), value = V2 of the choice.
 * Stream-ordered; with top_k > 0 the host never waits (n * top_k * 21 virtual roots are bounded up front, slots past a lane's kept
 * count are skipped on the device); top_k = 0 reads the number of kept candidates back once.  The (candidate, roll) pairs are
 * scored by the greedy step's own roots / expansion / value-net kernels on an internal scratch env (created on first use, grown up to
 * a fixed chunk of lanes, freed by bgamd_env_destroy; it uses this env's weight tables).  A search step writes neither the
 * trajectory log nor the ring log: with either set it returns BGAMD_E_INVALID.  Arena overflow, missing weights and delta errors
 * surface as they do for the greedy step. */
int bgamd_env_step_search(bgamd_env *env, int flags, int top_k, void *stream);
/* The last search step's kept candidates, best v1 first: d_states28 [n,K,28], d_v1 [n,K], d_v2 [n,K] (zero past a lane's count),
 * d_kept [n].  K = the last call's top_k; with top_k = 0 the largest kept count.  Any pointer may be NULL.  BGAMD_E_INVALID before
 * the first search step. */
int bgamd_env_search_read(bgamd_env *env, int32_t *d_states28, float *d_v1, float *d_v2, int32_t *d_kept, void *stream);

/* ---- the filtered search step (GNU Backgammon's move filter) -------------------------------------------------------------------------
 * bgamd_env_step_search (items 1-6 above, the same flags, refusals and errors) with these differences:
 *   - margin: with d(c) = v1(rank 0) - v1(c) for mover PLAYER1 and v1(c) - v1(rank 0) for mover PLAYER2 -- ONE fp32 subtraction, never
 *     negative -- a distinct afterstate is kept iff its rank in the (v1 for the mover, smaller key) order is below top_k (0 = no limit)
 *     AND d(c) <= margin.  Rank 0 is always kept.  Terminal candidates take part with their exact outcome, as they do in item 2.  margin
 *     is >= 0 and may be +inf; NaN or a negative margin: BGAMD_E_INVALID.  The kept list stays "best v1 first";
 *   - singletons: a lane with ONE kept candidate -- a forced move, or a lane the filter cut to one -- is not searched.  It contributes no
 *     virtual root, its candidate is played, bgamd_env_last_choice reports its v1 as the value and bgamd_env_search_read v2 = v1 for it.
 *     With margin = +inf the step therefore equals bgamd_env_step_search except for the reported value and v2 of such lanes: their
 *     choice and every board are the same;
 *   - list length: the step reads the real lengths of the candidate list and of the searched candidates back once (it SYNCHRONISES the
 *     stream once, as top_k = 0 does for bgamd_env_step_search) and launches only the scoring passes the searched list needs;
 *   - V2 of a kept candidate of a searched lane depends on the candidate and the weights alone -- not on top_k, the margin, the other
 *     lanes or the chunking.
 * bgamd_env_search_read works after either kind of step. */
int bgamd_env_step_search_filtered(bgamd_env *env, int flags, int top_k, float margin, void *stream);
/* Host values of the last search step of either kind (BGAMD_E_INVALID before the first, and after an analysis, as bgamd_env_search_read):
 *   h_out[0] lanes that had a move (kept >= 1);
 *   h_out[1] lanes searched: kept >= 2 after a filtered step; after bgamd_env_step_search every lane that had a move (= h_out[0]: it
 *            searches its singletons too);
 *   h_out[2] kept candidates;
 *   h_out[3] virtual roots scored = 21 x the non-terminal kept candidates of the searched lanes (the virtual lanes under a terminal
 *            candidate, and bgamd_env_step_search's slots past a lane's kept count, are finished lanes and are not counted).
 * The counts are taken when asked for (one small launch on the step's stream, which is SYNCHRONISED; further calls return the same
 * values without a launch): a search step launches nothing for them. */
int bgamd_env_search_info(bgamd_env *env, int64_t h_out[4]);

/* ---- the 3-ply search step: the opponent's replies chosen by 2-ply search -----------------------------------------------------------
 * The filtered step, whose best candidates by V2 are searched one ply deeper.  Flags are the filtered step's, with the same meaning; the
 * F32 incremental value net only; the weight slot by BGAMD_WEIGHTS_SLOT1.  For every live lane that takes part, mover m, opponent o:
 *   1. plies 1 and 2 are bgamd_env_step_search_filtered(top_k, margin), launch for launch: roll, enumerate, v1 of every distinct afterstate,
 *      the kept list L1, V2 of every candidate of a lane that kept >= 2; terminal candidates at their exact outcome, rank 0 always kept.  A
 *      lane that keeps one candidate plays it unsearched, value = v1;
 *   2. the deep set L2 of a searched lane: L1 ranked by (V2 for the mover, smaller key); d2(c) = ONE fp32 subtraction of V2(c) from
 *      V2(rank 0) on the mover's side, never negative; c is kept iff its rank < deep_k (0 = no limit) AND d2(c) <= deep_margin; rank 0 is
 *      always in.  A lane whose L2 has one member plays it -- it is the filtered step's choice --, its value is its V2, and no deeper root
 *      is spent on it;
 *   3. V3(c) for c in L2 when |L2| >= 2: a terminal c keeps its exact outcome; otherwise V3(c) = (sum over the 6 doubles of R3(c, r) + 2 x
 *      sum over the 15 other rolls) / 36 in fp32, each part in roll order -- item 4's expression of the 2-ply search, so equal replies of
 *      1.0 or 0.0 give exactly that;
 *   4. R3(c, r), the opponent's SEARCHED reply from c with roll r:
 *      - the replies are the distinct afterstates of (c, o to move, dice r); when o has no legal move the one reply is c itself (the pass),
 *        which a doubles roll without a move yields as a row everywhere and this step adds for the other rolls;
 *      - v1 of a reply d: the greedy step's value with o's turn bit, the exact outcome if o has borne off its 15th checker; for the pass
 *        reply the net's value of c with o's turn bit;
 *      - kept replies: the filter's rule with o as the mover -- rank in the (v1 for o, smaller key) order < reply_top_k (0 = all) and
 *        within reply_margin of rank 0;
 *      - EVERY kept reply, a single one too, gets V2(d) as item 4 of the 2-ply search defines it with the roles swapped: m's 21 rolls,
 *        m's greedy reply or m's no-move value, the same fp32 sum; a terminal d takes its outcome;
 *      - R3(c, r) = the best V2(d) for o over the kept replies: max for PLAYER1, min for PLAYER2;
 *      - R3 depends on (c, r), the weights, reply_top_k and reply_margin alone: not on the lane, the other lanes, the other parameters or
 *        the chunking;
 *   5. choose the member of L2 with the best V3 for the mover (ties: the smaller key); apply, terminal check, flip or auto-reset by the
 *      greedy step's own apply; bgamd_env_last_choice reports the chosen sequence and its deepest value: V3, or V2 / v1 for the lanes of
 *      items 2 / 1;
 *   6. bgamd_env_search_read and bgamd_env_search_info work after this step exactly as after the filtered step with the same (top_k,
 *      margin): the 2-ply part is bit-identical to it.
 * BGAMD_E_INVALID: a negative top_k, deep_k or reply_top_k; a NaN or negative margin of the three (+inf is allowed); a trajectory or ring
 * log set (the search step's refusal); a SEARCH LOG set -- 3-ply targets are not logged, and the step refuses rather than write them
 * half-right.  BGAMD_E_NOWEIGHTS, arena and delta errors surface as for the search step; error bits raised on the internal envs reach
 * this env's.
 * Synchronisation: the step SYNCHRONISES the stream 2 + C times: once as the filtered step does, once for the length of the deep list, and
 * once in each of the C chunks of the mid level (below) for the length of its reply list; a step in which no lane is searched deeper
 * synchronises twice.
 * Device memory: the mid level -- one lane per (deep candidate, opponent roll) -- lives on an internal mid env of at most 65 536 lanes
 * (~1.8 GB with its search buffers at that size; a smaller step creates a smaller one), created by the first 3-ply step and freed by
 * bgamd_env_destroy; C = ceil(21 x deep candidates / its lanes).  Its (reply, roll) virtual roots are scored on the scratch env of the
 * 2-ply search, which the step shares.  Per kept candidate the step adds 96 bytes (V3, the rank in L2, the deep list, 21 R3 values).
 * Out of scope: bgamd_env_analyze_moves judges by 2 plies; bgamd_env_rollout_policy(plies = 3) stays refused; nothing samples; the
 * search log is refused (above). */
int bgamd_env_step_search3(bgamd_env *env, int flags, int top_k, float margin, int deep_k, float deep_margin, int reply_top_k,
                           float reply_margin, void *stream);
/* Aligned with bgamd_env_search_read's slots after a 3-ply step: d_depth [n,K] = the deepest value the candidate received -- 1 (a
 * singleton's candidate), 2, or 3 (a member of L2 of a lane with |L2| >= 2) -- and 0 past a lane's kept count; d_v3 [n,K] = V3 where
 * depth = 3, else 0.  Either pointer may be NULL.  BGAMD_E_INVALID before the first 3-ply step, and after a later search step of another
 * kind or an analysis has overwritten the search state. */
int bgamd_env_search3_read(bgamd_env *env, float *d_v3 /*[n,K]*/, int32_t *d_depth /*[n,K]*/, void *stream);
/* Host values of the last 3-ply step (refused as bgamd_env_search3_read is; taken when asked for, as bgamd_env_search_info: one small
 * launch on the step's stream, which is SYNCHRONISED):
 *   h_out[0] lanes that had a move;   h_out[1] lanes searched at 2 plies (kept >= 2);   h_out[2] lanes searched at 3 plies (|L2| >= 2);
 *   h_out[3] deep candidates = the members of L2 of the lanes of h_out[2];
 *   h_out[4] mid lanes = 21 x the non-terminal ones of those;
 *   h_out[5] level-3 virtual roots scored = 21 x the non-terminal kept replies of all mid lanes. */
int bgamd_env_search3_info(bgamd_env *env, int64_t h_out[6]);

/* ---- search log: the search steps' turns for the learner (TD replay of searched games, fitting the net to its own search) ------------
 * d_rows and d_after are [max_plies][n] x 32 B rows (16-byte aligned) in the trajectory log's format (8 planes, turn in plane 0 bit 31);
 * d_target and d_v1 are [max_plies][n] floats.  d_rows == NULL disables the log; with d_rows set any of the other three may be NULL (that
 * part is not written); max_plies <= 0 with d_rows set: BGAMD_E_INVALID.  The setting sticks to the env and is separate from
 * bgamd_env_set_trajectory and the ring log: a search step still refuses to run while either of those is set.
 * While the log is set, every bgamd_env_step_search and bgamd_env_step_search_filtered writes one entry for each lane that is live and
 * takes part (not finished or frozen, not left out by BGAMD_ONLY_P1/P2), at index ply * n + lane, ply = the lane's ply when the step
 * begins -- the trajectory log's rule.  Plies >= max_plies are dropped: nothing is written past the buffers.  The entry:
 *   rows    the pre-move row: the lane's board and the mover's turn bit, bit-identical to what a greedy step would put into the
 *           trajectory log for that turn;
 *   after   the afterstate that is played, with the turn bit of the side that is NOT the mover -- a terminal afterstate too, and with
 *           BGAMD_NO_FLIP too.  A lane without a move logs its own board with that bit;
 *   target  V2 of the played candidate, bit-equal to the value bgamd_env_last_choice reports and to bgamd_env_search_read's v2 of it,
 *           for every lane whose candidates were searched: after bgamd_env_step_search every lane with a move, after the filtered step
 *           every lane that kept >= 2 candidates (a terminal candidate's V2 is its exact outcome).  A lane that was not searched -- the
 *           filtered step's singleton, a lane without a move -- gets a quiet NaN: bgamd_td_fit_step skips and counts such a row, so no
 *           mask is needed downstream.  For a non-terminal played candidate the target is a function of the logged `after` row and the
 *           weights alone: V2 is the 1-ply pre-roll lookahead of that position (bgamd_env_evaluate_preroll's roll values, item 4's sum);
 *   v1      the 1-ply value of the played candidate (a terminal candidate: its exact outcome); a lane without a move: a quiet NaN.
 * Lanes that take no part write nothing: their slots keep what the caller put there.  One pass of a thread per lane between the V2
 * reduction and the apply (csrc/bg_search_log.h), launched only while the log is set.
 * Refusals while the log is set (BGAMD_E_INVALID): a search step with BGAMD_AUTO_RESET (a lane's next game would write over its last
 * one); bgamd_env_step_greedy / run_greedy / step_sampled / run_sampled / step_random / step_random_walk (a turn played by them would be
 * a hole in the log).  bgamd_env_analyze_moves, bgamd_env_rollout and bgamd_env_evaluate_preroll ignore the log: they apply nothing to
 * the env, and the rollout's trial env never has one. */
int bgamd_env_set_search_log(bgamd_env *env, void *d_rows, void *d_after, float *d_target, float *d_v1, int64_t max_plies);

/* ---- move analysis: a played move scored against the 2-ply search (GNU Backgammon's "analyse game") ----------------------------------
 * Every lane's decision is its current board, side to move and dice as they stand (bgamd_env_set_states / bgamd_env_set_dice);
 * d_played28[g] is the afterstate that was played from lane g (reference layout; the mover's turn bit is implied).  flags: only
 * BGAMD_ONLY_P1, BGAMD_ONLY_P2 and BGAMD_WEIGHTS_SLOT1, with the greedy step's meaning.
 *   1. stage A is the search's items 1-2 without the roll: the same roots, expansion and F32 incremental value net with the mover's turn
 *      bit; v1(c) is the greedy step's value, bit for bit, a TERMINAL c scores its exact outcome; "distinct afterstates" and "smaller key"
 *      mean what they mean there;
 *   2. the distinct afterstates are ranked by (v1 for the mover, smaller key); kept are the top_k best (0 = all) AND the played afterstate,
 *      wherever it ranks.  The kept list stays "best v1 first": a played candidate whose rank is >= top_k is its last entry.  The list is
 *      bounded by n (top_k + 1) candidates up front: with top_k > 0 the host never waits (top_k = 0 reads the list's length back once);
 *   3. V2 of every kept candidate exactly as the search's item 4: the same scoring passes on the search's scratch env and the same fp32
 *      sum (doubles + 2 x others) / 36 in roll order.  A candidate's V2 depends on the candidate and the weights alone -- not on top_k,
 *      the other lanes or the chunking;
 *   4. nothing is applied: the lanes' boards, turns, dice, ply, episode and flags, bgamd_env_last_choice, the trajectory / ring logs and
 *      the win / finished / steps counters are untouched.  candidates_raw, rows_evaluated and the node counters of bgamd_env_stats DO
 *      advance, as stage A's launches advance them for any step.  The last search step's results are invalidated
 *      (bgamd_env_search_read: BGAMD_E_INVALID until the next search step); the env's arenas are scratch, as for
 *      bgamd_evaluate_incremental.
 * Per lane (bgamd_env_analysis_read; any pointer may be NULL):
 *   status    0 = analysed; 1 = the lane took no part (finished / frozen, or filtered out by BGAMD_ONLY_P1/P2); 2 = the mover has no legal
 *             move (nothing to judge); 3 = `played` is not one of the lane's afterstates -- an illegal move, or a state with |count| > 15
 *             or one that cannot be packed: it matches nothing and raises no error code.  (A doubles roll without a legal move is ONE
 *             empty sequence, as everywhere: its only afterstate is the board itself, distinct = 1, and the board played is status 0.)
 *   distinct  the number of distinct afterstates (status 0, 2, 3)
 *   rank1     the number of distinct afterstates that beat the played one in the (v1, key) order: 0 = the played move is the 1-ply choice
 *   v1_played / v1_best   v1 of the played afterstate / of rank 0
 *   v2_played / v2_best   V2 of the played afterstate / the best V2 for the mover over the kept set (ties: the smaller key)
 *   best28    the afterstate with v2_best
 *   rank2     the number of kept candidates that beat the played one in the (V2 for the mover, smaller key) order
 *   error     one fp32 subtraction, never negative: mover PLAYER1 v2_best - v2_played, mover PLAYER2 v2_played - v2_best; exactly 0.0 iff
 *             the bits tie
 * Status 3: the best side (distinct, v1_best, v2_best over the top_k, best28) is filled, every played-side field and error are 0 and
 * rank1 = rank2 = -1.  Status 1 or 2: everything but status (and, for 2, distinct) is 0.
 * d_summary[12] (doubles, the counts exact): for movers PLAYER1 [0..4] and PLAYER2 [5..9] the decisions analysed (status 0), the unforced
 * ones (distinct >= 2), the mistakes (error > 0), the sum of (double) error, the largest error; [10] = lanes with status 2, [11] = with
 * status 3.  Reduced in a fixed order without floating-point atomics: bit-identical from call to call, and each side's five numbers are
 * the same whether the sides are analysed together or in BGAMD_ONLY_P1 and BGAMD_ONLY_P2 calls.
 * Errors: BGAMD_E_INVALID for a NULL env or d_played28, top_k < 0, any other flag, a trajectory or ring log set (the search step's
 * refusal), and for bgamd_env_analysis_read before the first analysis or after one that failed; BGAMD_E_NOWEIGHTS for an empty slot;
 * arena and delta errors surface as they do for the search step.  Both calls are stream-ordered. */
int bgamd_env_analyze_moves(bgamd_env *env, int flags, int top_k, const int32_t *d_played28 /*[n][28]*/, void *stream);
int bgamd_env_analysis_read(bgamd_env *env, int32_t *d_status, int32_t *d_distinct, int32_t *d_rank1, int32_t *d_rank2,
                            float *d_v1_played, float *d_v1_best, float *d_v2_played, float *d_v2_best, float *d_error,
                            int32_t *d_best28 /*[n][28]*/, double *d_summary /*[12]*/, void *stream);

/* ---- Monte Carlo rollouts (TD-Gammon / GNU Backgammon rollouts; points: see bgamd_env_rollout_outcomes_read) -----------------------
 * Plays T = trials games ("trials") from each of the P positions d_states28[P] / d_turn[P] (turn = side to move; d_turn NULL = PLAYER1)
 * with the greedy policy and reports how often PLAYER1 wins.  Trial i of position p is one game:
 *   - id and dice: j = (position_offset + p) * T + i; the dice of the trial's turn k (k = 0, 1, ...) are the TURN-stream dice of a lane with
 *     game id j at ply k: Philox4x32-10(key = seed, counter = (j_lo, j_hi, k, STREAM_TURN)) through die_from_u32;
 *   - BGAMD_ROLLOUT_ROTATE in flags: turn 0 uses ordered pair number i mod 36 instead, d1 = 1 + (i mod 36) / 6, d2 = 1 + (i mod 36) % 6
 *     (T a multiple of 36: every first roll occurs exactly T / 36 times); turns k >= 1 as above;
 *   - play: both sides as bgamd_env_step_greedy with BGAMD_ROLL (fp32 incremental value net, weight slot by BGAMD_WEIGHTS_SLOT1, the
 *     mover's turn bit, arg-max for PLAYER1 / arg-min for PLAYER2, first index on ties, no special case for terminal afterstates); a pass
 *     is a turn;
 *   - outcome: a game that ends scores 1.0 if PLAYER1 won, else 0.0; a position that is already over scores its winner at 0 turns;
 *   - max_plies = M > 0: a trial still running after its M-th turn stops there and scores the fp32 net's value (same slot) of the board
 *     reached with the turn bit of the side now to move -- bit-identical to bgamd_evaluate_slot(..., BGAMD_F32) of that state and turn.
 *     M = 0 plays every trial to its end (BGAMD_E_INVALID if a trial is still running after 100 000 turns).
 * Per position (any pointer may be NULL): d_mean[P] = (1/T) sum x_i;  d_stderr[P] = sqrt(sum (x_i - mean)^2 / (T (T - 1))), 0 for T = 1 --
 * with rotation this is the plain, conservative estimate (the stratification by first roll is not credited);  d_turns[P] (int64) = total
 * turns played;  d_truncated[P] = trials scored by the net.  Per trial (optional): d_trial_value[P][T], d_trial_turns[P][T].
 * Results depend only on (positions, position_offset, T, M, flags, seed, weights): bit for bit the same for any `lanes` (the internal lane
 * count, 0 = default: min(65 536, P T rounded up to 256)) and from call to call; the statistics are reduced in a fixed order.  Splitting the
 * positions over calls (or ranks) with position_offset gives the same trials.
 * No side effect on this env: its lanes, dice, ply / episode, counters, last_choice and search results are untouched.  The trials run on
 * an internal scratch env of `lanes` lanes (created on first use, re-created when the lane count changes, freed by bgamd_env_destroy;
 * ~1.7 GB at 65 536 lanes) that uses this env's weight tables; buffers of O(P T) bytes are kept between calls.
 * Errors: P < 1, T < 1, M < 0, lanes < 0, position_offset < 0, P T >= 2^31 or flags other than BGAMD_ROLLOUT_ROTATE | BGAMD_WEIGHTS_SLOT1 |
 * BGAMD_ROLLOUT_VR (below): BGAMD_E_INVALID; a bad state: BGAMD_E_STATE; an empty weight slot: BGAMD_E_NOWEIGHTS; arena overflow and delta errors of the greedy
 * kernels: BGAMD_E_ARENA / BGAMD_E_DELTA.
 * SYNCHRONISES the stream before it returns (it must know when the last trial has ended; the host reads a trials-done counter about every
 * 16 turns). */
int bgamd_env_rollout(bgamd_env *env, int flags, const int32_t *d_states28, const int32_t *d_turn, int64_t n_positions,
                      int64_t position_offset, int64_t trials, int64_t max_plies, uint64_t seed, int64_t lanes,
                      double *d_mean, double *d_stderr, int64_t *d_turns, int32_t *d_truncated,
                      float *d_trial_value, int32_t *d_trial_turns, void *stream);
/* Diagnostics of the last rollout (host values): h_out = [lanes, env steps issued (rotation steps included), lane-steps that played a
 * turn of a live trial, turns per run between refill points].  Idle share = 1 - h_out[2] / (h_out[0] h_out[1]). */
int bgamd_env_rollout_info(bgamd_env *env, int64_t h_out[4]);
/* Who plays the turns of bgamd_env_rollout's trials.  The setting sticks to the env.  plies = 1 (the default): the greedy step, as described
 * above -- launches and outputs are what they are on an env that never called this.  plies = 2: every turn of every trial, the rotated
 * first turn included, is chosen by bgamd_env_step_search_filtered with (top_k, margin) and the rollout's weight slot.  Everything else in
 * the rollout's contract stays: trial ids and TURN-stream dice (a 2-ply rollout shares its dice with the 1-ply rollout of the same
 * positions, T and seed), the rotation pairs, a pass is a turn, the outcome scoring, truncation at max_plies by the fp32 net value of the
 * board reached, the fixed reduction order, independence of `lanes`, of the call order and of position_offset splits, no side effect on
 * the env.  Each search turn is a step of its own with a refill after it: bgamd_env_rollout_info reports 1 turn per run.
 * bgamd_env_rollout_outcomes_read works as before.  BGAMD_ROLLOUT_VR is allowed: a turn's luck keeps its definition (the 1-ply f and mean
 * of bgamd_env_evaluate_preroll; E[luck | history] = 0 whatever the policy, so the adjusted value stays unbiased) and the plain outputs
 * are bit-identical with and without the flag.
 * The virtual roots are scored on THIS env's search scratch env (shared with the luck pass; at most 131 072 lanes, ~3.4 GB); the trial
 * env's own search buffers add ~0.2 GB at 65 536 lanes and top_k 5.
 * plies other than 1 or 2, top_k < 0, a negative or NaN margin: BGAMD_E_INVALID (the setting is unchanged). */
int bgamd_env_rollout_policy(bgamd_env *env, int plies /* 1 | 2 */, int top_k, float margin);

/* ---- rollouts on shared dice: dice groups and paired differences -------------------------------------------------------------------------
 * bgamd_env_rollout in every respect but the dice id.  d_group[P] assigns each position to a dice group (any non-negative numbers: sparse,
 * unordered, repeated).  Trial i of position p rolls the TURN-stream dice of game id j = (group_offset + d_group[p]) * T + i -- trial i of
 * every position of a group plays the same dice at every ply ("common random numbers": the candidates of one decision meet the same
 * luck, so their difference is known far more tightly than either mean).  With BGAMD_ROLLOUT_ROTATE turn 0 uses ordered pair i mod 36, as
 * there.  The trial's RESULT slot stays p * T + i: every output ([P], [P][T]) is indexed by position as before, and so is everything the
 * read calls return.  Unchanged: the policy (bgamd_env_rollout_policy), BGAMD_ROLLOUT_VR, bgamd_env_rollout_outcomes_read, truncation,
 * the fixed reduction order, bit-identical results for any `lanes`, from call to call and when the groups are split over calls with
 * group_offset, and no side effect on the env.  Position p of this call computes, bit for bit, what the single-position call
 * bgamd_env_rollout(position p alone, position_offset = group_offset + d_group[p]) computes.
 * d_group NULL: every position is its own group p -- this IS bgamd_env_rollout with position_offset = group_offset (the same launches,
 * the same bits; bgamd_env_rollout is implemented as this call).
 * Errors, beside bgamd_env_rollout's: a negative group, (max group + 1) * T >= 2^31 or group_offset < 0: BGAMD_E_INVALID.  The table is
 * checked in the pass that refuses bad states, before anything is played.
 * The env keeps a device copy of the table (4 P bytes) for bgamd_env_rollout_paired_read. */
int bgamd_env_rollout_grouped(bgamd_env *env, int flags, const int32_t *d_states28, const int32_t *d_turn, const int32_t *d_group /*[P]*/,
                              int64_t n_positions, int64_t group_offset, int64_t trials, int64_t max_plies, uint64_t seed, int64_t lanes,
                              double *d_mean, double *d_stderr, int64_t *d_turns, int32_t *d_truncated,
                              float *d_trial_value, int32_t *d_trial_turns, void *stream);
/* Paired differences of the last rollout of either kind (P and T of that call; BGAMD_E_INVALID before the first or after one that failed).
 * `which` selects the per-trial quantity q: 0 the value x_i; 1 the luck-adjusted y_i = (double) x_i - L_i (BGAMD_E_INVALID unless that
 * rollout had BGAMD_ROLLOUT_VR); 2 the equity e_i in points as bgamd_env_rollout_outcomes_read defines it; 3 the cubeful
 * equity of bgamd_env_rollout_cube_read (BGAMD_E_INVALID unless that rollout ran with the cube on); 4 the match-winning chance of
 * bgamd_env_rollout_match_results (BGAMD_E_INVALID unless that rollout ran under a match).  Other values: BGAMD_E_INVALID.
 * For each position p with its reference r = d_ref[p], in fp64:
 *   d_i = q_i(p) - q_i(r);  d_diff_mean[p] = (1/T) sum d_i;  d_diff_stderr[p] = sqrt(sum (d_i - diff_mean)^2 / (T (T - 1))), 0 for T = 1,
 * reduced in the fixed order of the plain statistics (one wave per position, lane k takes trials k, k + 64, ..., then the same butterfly).
 * A reference outside [0, P), or in another dice group than p (after an ungrouped rollout: any r != p) pairs nothing: both outputs are
 * NaN for that p, the other positions are unaffected.  r = p gives exactly 0 and 0.  Either output may be NULL; d_ref may not.
 * Stream-ordered, does not synchronise; the rollout's own outputs and the other reads are what they were without this call. */
int bgamd_env_rollout_paired_read(bgamd_env *env, const int32_t *d_ref /*[P]*/, int which, double *d_diff_mean /*[P]*/,
                                  double *d_diff_stderr /*[P]*/, void *stream);

/* ---- 1-ply pre-roll evaluation (GNU Backgammon's "evaluation before the roll") ------------------------------------------------------
 * For each of the n positions s = d_states28[n] with the side to roll m = d_turn[n] (NULL = PLAYER1), what the roller can expect from
 * each of the 21 unordered rolls r = (1,1), (1,2), ..., (1,6), (2,2), ..., (6,6), in that order (the search's roll order):
 *   - f(s, r) is exactly the R(c, r) of the search's item 4 with s in the place of c and the roller in the opponent's role: when the
 *     roller has a move, the value of the afterstate the greedy step would choose (F32 incremental value net, the roller's turn bit,
 *     arg-max for PLAYER1 / arg-min for PLAYER2, no special case for terminal afterstates); when the roller has no move, the net's value
 *     of s with the roller's turn bit; a position that is already over (15 off for either side) gives its outcome, 1.0 if PLAYER1 has
 *     won, else 0.0, for every roll;
 *   - mean(s) = sum over the 21 rolls in order of w_r * (double) f(s, r) in fp64, w_r = 1.0/36.0 for a double and 2.0/36.0 otherwise
 *     (a rounded product and a rounded sum per roll, no fused multiply-add).
 * Out (either may be NULL): d_roll_values[n][21] (fp32), d_mean[n] (fp64).  flags: 0 or BGAMD_WEIGHTS_SLOT1 (the weight slot).  A
 * position's values depend on nothing else in the call (not on the other positions, n or the chunking).
 * No side effect on this env: its lanes, dice, ply / episode, counters, last_choice, search results and rollout results are untouched.
 * The n x 21 (position, roll) pairs are scored by the greedy step's own kernels on the search's internal scratch env.
 * Errors: n < 1 or other flags: BGAMD_E_INVALID; a bad state: BGAMD_E_STATE; an empty weight slot: BGAMD_E_NOWEIGHTS; arena overflow and
 * delta errors of the greedy kernels: BGAMD_E_ARENA / BGAMD_E_DELTA.  SYNCHRONISES the stream (a bad state is refused before anything is
 * scored; the scratch env's error bits are read at the end). */
int bgamd_env_evaluate_preroll(bgamd_env *env, int flags, const int32_t *d_states28, const int32_t *d_turn, int64_t n,
                               float *d_roll_values, double *d_mean, void *stream);

/* ---- luck-adjusted rollouts (BGAMD_ROLLOUT_VR; GNU Backgammon's variance reduction) ------------------------------------------------
 * With BGAMD_ROLLOUT_VR in its flags, bgamd_env_rollout also charges every trial with the luck of its rolls:
 *   - the played trials are unchanged: every output of the call (mean, stderr, turns, truncated, per-trial value and turns) and
 *     bgamd_env_rollout_info are bit-identical to the same call without the flag;
 *   - luck of a turn: trial i plays turns k = 0 ... K_i - 1; before turn k its board is s_k with m_k to roll, the turn is played with
 *     dice (a, b) and r_k is their unordered roll.  luck_k = (double) f(s_k, r_k) - mean(s_k), with f and mean bit-identical to what
 *     bgamd_env_evaluate_preroll returns for (s_k, m_k) with the rollout's weight slot.  A pass is a turn with a luck like any other;
 *     the last turn of a game counts too;
 *   - rotation: turn 0 of trial i is played with ordered pair i mod 36, and its luck uses the pre-roll evaluation of the position
 *     itself (evaluated once per call).  Over a multiple of 36 trials the turn-0 lucks cancel (up to rounding): the adjusted stderr
 *     credits the stratification by first roll that the plain one does not;
 *   - truncation (max_plies = M > 0): turns 0 ... M - 1 count; the trial's value x_i is the plain one.  A position that is already over
 *     has L = 0;
 *   - per trial: L_i = sum of luck_k in fp64, in turn order, from 0.0; the adjusted value is y_i = (double) x_i - L_i;
 *   - per position: vr_mean = (1/T) sum y_i;  vr_stderr = sqrt(sum (y_i - vr_mean)^2 / (T (T - 1))), 0 for T = 1; both reduced in the
 *     fixed order of the plain statistics.  Like them, bit for bit the same for any `lanes`, from call to call and over position_offset
 *     splits.
 * Why it is unbiased: E[luck_k | history] = 0 because r_k is drawn from the same 1/36 and 2/36 distribution the mean uses
 * (die_from_u32 is uniform to within 2^-32 per die), so E[y_i] = E[x_i].
 * Cost: before every turn of every trial the 21 rolls of its position are scored (21 virtual roots on the search's scratch env). */
/* The luck-adjusted results of the last bgamd_env_rollout, which must have had BGAMD_ROLLOUT_VR (else BGAMD_E_INVALID): d_vr_mean[P],
 * d_vr_stderr[P], d_trial_luck[P][T] = L_i (fp64, any may be NULL; P and T of that call).  Stream-ordered. */
int bgamd_env_rollout_vr_read(bgamd_env *env, double *d_vr_mean, double *d_vr_stderr, double *d_trial_luck, void *stream);

/* ---- gammons and backgammons: a finished game in points ------------------------------------------------------------------------------
 * Backgammon is scored in points.  The reference knows wins only (over(), cppsrc/game.cpp:388-407), so the standard rules apply.  The
 * winner is the side over() names (PLAYER1 is checked first: 15 off on both sides is PLAYER1's).  With the loser being the other side:
 *   - single game (1 point): the loser has borne off at least one checker;
 *   - backgammon (3 points): the loser has borne off none and has a checker on its bar or in the winner's home board (PLAYER1 won: a
 *     PLAYER2 checker on points 19-24 or on PLAYER2's bar; PLAYER2 won: a PLAYER1 checker on points 1-6 or on PLAYER1's bar);
 *   - gammon (2 points): everything else.
 * Points are from PLAYER1's side: 0 = the game is not over, +1 / +2 / +3 = PLAYER1 won a single game / a gammon / a backgammon,
 * -1 / -2 / -3 = PLAYER2 did.
 * OUT OF SCOPE: games that are auto-reset inside a greedy step (BGAMD_AUTO_RESET, continuous self-play).  Their final boards are gone
 * when the step returns; counting their gammons would mean changing the step's boundary launch.  The env's counters stay win / loss. */
#define BGAMD_OUTCOME_BAD INT32_MIN
/* points of each state from PLAYER1's side (0 = not over); a state with |count| > 15 gives BGAMD_OUTCOME_BAD (INT32_MIN).
 * Stateless, stream-ordered, nothing synchronises.  n < 1 or a NULL pointer: BGAMD_E_INVALID. */
int bgamd_outcomes(const int32_t *d_states28, int64_t n, int32_t *d_points, void *stream);
/* the same for the CURRENT board of every lane of an env (d_points[n_games]): a frozen lane (finished without BGAMD_AUTO_RESET) keeps its
 * final board, so this is the result of its game; a lane that is still playing, or was auto-reset, gives 0.  The env is not changed.
 * Stream-ordered.  A NULL pointer: BGAMD_E_INVALID. */
int bgamd_env_outcomes(bgamd_env *env, int32_t *d_points, void *stream);

/* Outcomes of the last bgamd_env_rollout (any flags; BGAMD_E_INVALID before the first, or after one that failed; P and T of that call).
 * Every trial that bgamd_env_rollout scores from a board -- a game that ended on its lane, a position that was already over, a rotated
 * first turn that ended the game -- also records that board's points; a truncated trial (max_plies) records 0.  Any pointer may be NULL.
 *   d_counts[P][6]     int64: trials that ended as PLAYER1 single, gammon, backgammon, PLAYER2 single, gammon, backgammon (truncated trials are
 *                      in none of the six: the six sum to T - truncated[p]);
 *   d_trial_points[P][T] int8: +-1, +-2, +-3, or 0 for a trial scored by the net;
 *   equity of trial i, fp64, PLAYER1's cubeless money equity in points: (double) points_i for a finished trial; 2.0 * (double) x_i - 1.0 for a
 *   truncated one (x_i = its fp32 net value: the net knows wins only, a truncated trial is credited no gammons);
 *   d_equity[P] = (1/T) sum e_i;  d_equity_stderr[P] = sqrt(sum (e_i - mean)^2 / (T (T - 1))), 0 for T = 1.
 * Reduced in the fixed order of the plain statistics: bit for bit the same for any `lanes`, from call to call and over position_offset
 * splits.  Stream-ordered.  The plain outputs of bgamd_env_rollout, bgamd_env_rollout_info and bgamd_env_rollout_vr_read are what they
 * were without this call.
 * The luck adjustment stays a WIN-PROBABILITY quantity: vr_mean of bgamd_env_rollout_vr_read is not an equity, because the f and mean
 * that make up a turn's luck come from a one-output net that estimates P(PLAYER1 wins) and knows nothing of gammons. */
int bgamd_env_rollout_outcomes_read(bgamd_env *env, int64_t *d_counts, double *d_equity, double *d_equity_stderr,
                                    int8_t *d_trial_points, void *stream);

/* ---- the doubling cube on the rollout's trials: cubeful money equity ------------------------------------------------------------------
 * The net knows wins only, so the cube never changes which checker move is played: a cubeful rollout is an OVERLAY on the trials as
 * bgamd_env_rollout plays them.  Every trial carries a record -- the cube value c (a power of two), its owner o (0 the centre, 1 PLAYER1,
 * 2 PLAYER2), the turn index of a drop (or -1) with the side that passed, and how often the cube was turned in the trial -- which is
 * advanced before every turn from the pre-roll mean the luck pass (BGAMD_ROLLOUT_VR) computes anyway.  The cubeless and the cubeful
 * results come from the same trials, as GNU Backgammon reports them.
 * THE RULE.  A trial of position p starts with c = d_cube_value[p] and o = d_cube_owner[p] (NULL tables: 1, in the centre).  Before turn
 * k of the trial the board is s_k and m_k is to roll -- turn 0 and a rotated turn 0 included, the latter on the position's own pre-roll
 * mean, evaluated once per call like the turn-0 luck.  A cube decision is made iff the trial has not been dropped, the position is not
 * over, c < max_cube, and o is the centre or m_k.  Then, in fp64:
 *   w = mean(s_k) for PLAYER1 to roll, 1.0 - mean(s_k) for PLAYER2 (one subtraction); mean is bit-identical to what
 *       bgamd_env_evaluate_preroll returns for (s_k, m_k) with the rollout's weight slot;
 *   m_k doubles iff double_at <= w && w <= too_good_at;
 *   the opponent then passes iff w > pass_at: the trial is dropped at turn k and its cubeful result is c, the value BEFORE the double,
 *       won by m_k; else it takes: c <- 2 c, o <- the opponent, one more cube turn.
 * A pass (no legal move) is a turn like any other and the cube is offered before it.  The trial keeps being played after a drop (its
 * lane is not freed: bgamd_env_rollout_cube_info reports what that costs).
 * Cubeful equity of a trial from PLAYER1's side, fp64: dropped: +c if PLAYER2 passed, -c if PLAYER1 did (c at the drop); finished on the
 * board: c_final * points, points = +-1, +-2, +-3 as bgamd_env_rollout_outcomes_read records them; with BGAMD_CUBE_JACOBY a trial whose
 * cube was never turned IN THE TRIAL counts as a single game, c_final * (+-1), whatever cube it started with; truncated at max_plies:
 * c * (2.0 * (double) x_i - 1.0).  No further cube leverage is credited at the horizon (no Janowski-style live-cube equity): out of scope.
 * The defaults suggested for the thresholds -- double_at 0.70, pass_at 0.78, too_good_at 1.0 (never too good: w is a win probability
 * and knows no gammons), max_cube 64 -- are a plain money-play rule of thumb and NO measured optimum.
 *
 * BGAMD_CUBE_HOLD_TURN0: no decision is made before turn 0 of a trial (rotated or not); from turn 1 on the rule is as above.  It is what
 * "no double" means when a cube action is analysed: the roller holds the cube this turn, and both sides handle it by the rule afterwards.
 *
 * bgamd_env_rollout_cube is a sticky setting like bgamd_env_rollout_policy.  cube_flags: 0 switches the cube off (the default: the
 * rollouts' launches and results are what they are on an env that never called this; the other arguments are ignored), or BGAMD_CUBE_ON,
 * alone or with BGAMD_CUBE_JACOBY and / or BGAMD_CUBE_HOLD_TURN0.  d_cube_value / d_cube_owner are DEVICE pointers (either may be NULL), read by the next rollout's
 * intake pass; their length is that call's P, and they must stay valid until that call.  Errors (BGAMD_E_INVALID, the setting
 * unchanged): other flags, a flag without BGAMD_CUBE_ON, a NaN threshold, a threshold outside [0, 1], double_at > too_good_at,
 * max_cube not a power of two in 1 .. 2^30.
 * While the cube is on: a rollout call without BGAMD_ROLLOUT_VR returns BGAMD_E_INVALID before anything is played; a table entry that is
 * no power of two in 1 .. 2^30, or an owner outside 0 .. 2, is refused (BGAMD_E_INVALID) in the pass that refuses bad states.  The plain
 * outputs, bgamd_env_rollout_info, bgamd_env_rollout_vr_read, bgamd_env_rollout_outcomes_read and bgamd_env_rollout_paired_read with
 * which 0 .. 2 are bit for bit what the same call without the cube returns.
 * Out of scope: the cube in live envs, self-play and the arena; cube-aware checker play; freeing a lane at a drop; cubeful rollouts
 * without the luck pass.  (Match play: bgamd_env_rollout_match below.) */
enum { BGAMD_CUBE_ON = 1, BGAMD_CUBE_JACOBY = 2, BGAMD_CUBE_HOLD_TURN0 = 4 };
int bgamd_env_rollout_cube(bgamd_env *env, int cube_flags, double double_at, double pass_at, double too_good_at, int64_t max_cube,
                           const int32_t *d_cube_value /*[P]*/, const int32_t *d_cube_owner /*[P]*/);
/* The cube results of the last rollout, which must have run with the cube on (else BGAMD_E_INVALID); P and T of that call.  Any pointer
 * may be NULL.  d_cubeful[P], d_cubeful_stderr[P] (fp64): mean and standard error of the per-trial cubeful equity, reduced in the fixed
 * order of the plain statistics (one wave per position, lane k takes trials k, k + 64, ..., then the same butterfly), every sum a chain
 * of rounded fp64 additions.  d_counts[P][4] (int64): trials that PLAYER1 passed, trials that PLAYER2 passed, cube turns in all, trials
 * whose final cube is >= max_cube.  d_trial_cubeful[P][T] (fp64), d_trial_cube[P][T] (int32, the final cube), d_trial_dropped[P][T]
 * (int32, the turn of the drop or -1).  Like every rollout result bit for bit independent of `lanes`, of the call order and of
 * position_offset / group_offset splits.  Stream-ordered. */
int bgamd_env_rollout_cube_read(bgamd_env *env, double *d_cubeful, double *d_cubeful_stderr, int64_t *d_counts, double *d_trial_cubeful,
                                int32_t *d_trial_cube, int32_t *d_trial_dropped, void *stream);
/* host values of the last cubeful rollout: h_out = [turns played on the trial env's lanes (a rotated turn 0 is not: it is played once per
 * ordered pair), those of them played after the trial's drop, the turn the drop is made before included].  h_out[1] / h_out[0] is the
 * share of the rollout's work that freeing a lane at a drop would save. */
int bgamd_env_rollout_cube_info(bgamd_env *env, int64_t h_out[2]);

/* ---- match play on the cubeful rollouts: match-winning chance by score ------------------------------------------------------------------
 * At a match score the cube's thresholds stop being constants, some cubes are dead, the Crawford game has no cube, and a trial is worth
 * a match-winning chance (MWC), not points.  A match is a second sticky setting on top of bgamd_env_rollout_cube: the same trials, the
 * same per-trial record with its one writer, the cube's conditions and four of its settings (too_good_at, max_cube, the start tables,
 * BGAMD_CUBE_HOLD_TURN0); the cube setting's double_at and pass_at are IGNORED while a match is set.  All arithmetic is fp64 and every
 * operation is rounded on its own (no fused multiply-add, on the device or on the host), so a Python float model is exact.
 * A SETTING: a table size M, 1 <= M <= 64; met[M][M], met[a-1][b-1] = the chance that a side needing a points beats a side needing b,
 * the 1-away row and column holding the Crawford-game values; met_pc[M], met_pc[k-1] = the post-Crawford chance of a trailer needing k
 * against a leader needing 1 (met_pc[0]: double match point); window_share in [0, 1].  Per position p: away1[p], away2[p] in 1 .. M
 * (PLAYER1's and PLAYER2's points to go) and state[p]: 0 normal, 1 the Crawford game, 2 post-Crawford; 1 and 2 are valid iff
 * min(away1, away2) == 1, 0 iff min(away1, away2) > 1.
 * after(a1, a2, state) is the MWC of the side needing a1 when the next game starts against a side needing a2; the first case that
 * applies:  a1 <= 0: 1.0;  a2 <= 0: 0.0;  state != 0 (the next game is post-Crawford) and a2 == 1: met_pc[a1-1];  state != 0 and
 * a1 == 1: 1.0 - met_pc[a2-1];  otherwise met[a1-1][a2-1].  Points are subtracted in 64-bit integers (c x 3 can exceed 32 bits).
 * THE DECISION before turn k.  The cube record's conditions stay (not dropped, position not over, c < max_cube, access to the cube,
 * BGAMD_CUBE_HOLD_TURN0), and a match adds two: state[p] == 1 (the Crawford game): no decision; c >= the roller's away (a dead cube):
 * no decision, and the trial is counted as one in which a decision was withheld by a dead cube.  Otherwise, with a the roller's points
 * to go, b the opponent's, W(k) = after(a - k, b, state) the roller's MWC after winning k points in this game and
 * L(k) = after(a, b - k, state) after losing k -- the roller reads the table from ITS OWN row, whichever seat it has (for a table with
 * met[a][b] + met[b][a] == 1 that is 1 - PLAYER1's view up to rounding) -- and W1 = W(c), L1 = L(c), W2 = W(2c), L2 = L(2c):
 *   pass_at   = (W1 - L2) / (W2 - L2)                         the opponent's dead-cube take point, in the roller's w;
 *   open      = (L1 - L2) / ((L1 - L2) + (W2 - W1))           where doubling stops losing;
 *   double_at = open + window_share * (pass_at - open).
 * A denominator <= 0, or a result that is not finite: no decision is made at that entry (double_at = +inf).  From there the cube's own
 * rule applies with these two numbers: the roller doubles iff double_at <= w && w <= too_good_at, the opponent passes iff w > pass_at,
 * and otherwise takes.  The thresholds are computed ONCE per setting on the host, for every (state in {0, 2}, cube 2^l < M, a, b), and
 * uploaded with the tables: on the device a decision is a few small loads and one 16-byte load, and no division.
 * The net knows wins only and no gammons, so the thresholds do not either: W(k) and L(k) count single games.  window_share is a rule
 * of thumb (0.5 is the suggested default) and NO measured optimum, like the cube's own thresholds.
 * PAYOFF of a trial, PLAYER1's MWC (PLAYER1's row).  r = the trial's points from PLAYER1's side: a dropped trial +-c, c the cube BEFORE
 * the double; a trial finished on the board c x points; in both cases mwc = after(a1 - max(r, 0), a2 - max(-r, 0), state) -- a gammon
 * with the cube on 2 at 3-away ends the match, points beyond the match length are worth nothing.  A trial truncated at max_plies with
 * fp32 value x: mwc = x * after(a1 - c, a2, state) + (1 - x) * after(a1, a2 - c, state), formed as
 * dadd(dmul(x, .), dmul(dsub(1, x), .)).  Jacoby has no meaning in a match.
 *
 * bgamd_env_rollout_match is sticky.  match_flags: BGAMD_MATCH_ON sets it, 0 clears it (the other arguments are ignored; an env that
 * cleared it behaves as one that never set it).  h_met[M][M] and h_met_pc[M] are HOST pointers, copied at the call together with the
 * threshold table computed from them.  d_away1, d_away2, d_state are DEVICE pointers [P], read by the next rollout's intake pass like
 * the cube's start tables; they must stay valid until that call.  Errors (BGAMD_E_INVALID, the setting unchanged): other flags, M
 * outside 1 .. 64, a NULL table, a table entry outside [0, 1] or not finite, window_share NaN or outside [0, 1].  A call that sets new
 * tables ends the readability of an earlier rollout as a match (bgamd_env_rollout_match_results, which = 4); clearing does not.
 * While a match is set: a rollout call with the cube off, with BGAMD_CUBE_JACOBY set, or without BGAMD_ROLLOUT_VR returns
 * BGAMD_E_INVALID before anything is played; an away outside 1 .. M, a state outside 0 .. 2 or one that does not go with the score is
 * refused (BGAMD_E_INVALID) in the pass that refuses bad states.  Every other output of the call -- the plain ones,
 * bgamd_env_rollout_info, the luck and outcome reads, paired which 0 .. 2 -- is bit for bit what it is without the match;
 * bgamd_env_rollout_cube_read and which = 3 describe, in points, the records the match rule produced.
 * Out of scope: a match in live envs, self-play and the arena; playing a match game after game; gammon-aware or live-cube thresholds;
 * automatic doubles and beavers; freeing a lane at a drop; a shipped published match equity table. */
enum { BGAMD_MATCH_ON = 1 };
int bgamd_env_rollout_match(bgamd_env *env, int match_flags, int64_t M, const double *h_met /*[M][M]*/, const double *h_met_pc /*[M]*/,
                            double window_share, const int32_t *d_away1 /*[P]*/, const int32_t *d_away2 /*[P]*/,
                            const int32_t *d_state /*[P]*/);
/* The match results of the last rollout, which must have run under a match (else BGAMD_E_INVALID); P and T of that call.  Any pointer
 * may be NULL.  d_mwc[P], d_mwc_stderr[P] (fp64): mean and standard error of the per-trial MWC of PLAYER1, in the fixed order of
 * bgamd_env_rollout_cube_read.  d_counts[P][3] (int64): trials that ended the match for PLAYER1, trials that ended it for PLAYER2 (a
 * truncated trial is in neither), trials in which some decision was withheld by a dead cube.  d_trial_mwc[P][T] (fp64).  Bit for bit
 * independent of `lanes`, of the call order and of position_offset / group_offset splits.  Stream-ordered. */
int bgamd_env_rollout_match_results(bgamd_env *env, double *d_mwc, double *d_mwc_stderr, int64_t *d_counts /*[P][3]*/, double *d_trial_mwc,
                                 void *stream);
/* h_out = {double_at, pass_at} of the uploaded threshold table, read back from the device: state 0 or 2, cube a power of two below M,
 * a the roller's and b the opponent's points to go in 1 .. M; +inf, +inf where no decision is made.  BGAMD_E_INVALID for anything else
 * and before the first setting.  Synchronises. */
int bgamd_env_rollout_match_thresholds(bgamd_env *env, int state, int64_t cube, int a, int b, double h_out[2]);

/* (slot 8 below counts the 32-row x 2-feature MFMA steps of the dense f32 net, or the W1 columns added by the
 * incremental one) */
/* counters since create/reset_stats (synchronises): [steps, games_finished, p1_wins, candidates_raw,
 * rows_evaluated, error_flags, leaf_parent_nodes, doubles_inner_nodes, ksteps_executed (fp32 value net:
 * 32-row x 2-feature MFMA steps actually issued, of 99 per tile), reserved] */
int bgamd_env_stats(bgamd_env *env, uint64_t h_out[10]);
int bgamd_env_reset_stats(bgamd_env *env, void *stream);

/* single-checker surface for lane-wise moves: Game::tryMove (game.cpp:573-663) and
 * Game::legalMoves (game.cpp:80-105).  d_err: 0 ok, 1..7 = the reference's messages in source order. */
int bgamd_env_try_move(bgamd_env *env, const int32_t *d_player, const int32_t *d_dice, const int32_t *d_origin,
                       const int32_t *d_dest, int32_t *d_err, void *stream);
int bgamd_env_legal_moves(bgamd_env *env, const int32_t *d_player, const int32_t *d_die,
                          int32_t *d_n, int8_t *d_pairs /*[n,26,2]*/, void *stream);

/* diagnostics: (game, key | turn<<31) of every row the value net evaluated in the last greedy step (after the
 * pruning of commuting move orders: a few per cent of the rows are still copies); returns the row count (synchronises). */
int64_t bgamd_env_unique_rows_info(bgamd_env *env, void *d_info /* uint32[cap][2] */, int64_t cap, void *stream);
/* ... and the rows themselves with the value the net gave each: rows [first, first + n_rows) of that list as int32
 * states [n_rows][28] and float values [n_rows] (either may be NULL).  With BGAMD_F32 these are the outputs of the
 * incremental kernel, row by row -- what the parity tests compare with the reference model.  (Round 4: the step keeps its rows in four
 * arenas by kind of turn and by whether the moves hit a blot; both calls list them one arena after the other, i.e. `first` counts rows
 * of that list.  The order of the rows inside an arena is the order in which the leaf stage's workgroups allocated them: no meaning.) */
int bgamd_env_unique_rows_read(bgamd_env *env, int64_t first, int64_t n_rows, int32_t *d_states28, float *d_values,
                               void *stream);

/* ---- net health: is this weight table still one the value net can play with, and does its hidden layer still tell rows apart? ----------
 * A training loop's own question (the reference's loop never asks it: train.py:519-547 saves whatever the updates left).  Stateless, in
 * the style of bgamd_encode_rows: d_theta = 25 601 device floats (W1[128][198] | b1 | W2 | b2: a learner's table as it stands, no env
 * needed), d_rows = n_rows 32-byte rows (16-byte aligned) in the trajectory log's format (bgamd_pack_rows, bgamd_env_set_trajectory, the
 * ring log), threshold > 0 (15: sigmoid'(15) ~ 3e-7, a unit that far out passes no gradient and tells no two rows apart).
 *   weights : nonfinite = the NaN / +-Inf among the 25 601; max_abs = the largest finite |w| of each tensor, exact; fits_f16_split = 1
 *             iff bgamd_weights_check (and so bgamd_env_load_weights) would accept the table -- the same test, run on the device;
 *   rows    : a = fc1.weight x + fc1.bias of every row and unit in fp32 (the dense evaluator's v_mfma_f32_32x32x2_f32 chain over all 99
 *             k-steps, W1 as it is: no 16-bit table), then the sigmoids and the second layer.  saturated = (row, unit) pairs with
 *             |a| > threshold, unit_saturated[u] = the rows on which unit u is, dead_units = units that are on EVERY row,
 *             max_abs_preact = max |a|, v_min / v_max = the extreme net outputs.
 * n_rows = 0 (d_rows may be NULL): the weight fields, everything else zero.  The rows' fields mean something only when nonfinite == 0;
 * with non-finite weights the call still completes.  Every field is an integer count or a min / max: bit-identical from call to call.
 * threshold <= 0 (or NaN), n_rows < 0 or n_rows >= 2^31: BGAMD_E_INVALID.  Stream-ordered on the current device, nothing synchronises;
 * d_out is DEVICE memory. */
typedef struct {
    int64_t nonfinite;            /* weights that are NaN or +-Inf, of 25 601 */
    int64_t rows;                 /* n_rows */
    int64_t saturated;            /* (row, unit) pairs with |a| > threshold, a = fc1.weight x + fc1.bias in fp32 */
    int64_t dead_units;           /* units saturated on EVERY row (0 when n_rows = 0) */
    float   max_abs[4];           /* largest finite |w| of fc1.weight, fc1.bias, fc2.weight, fc2.bias (0 if none finite) */
    float   max_abs_preact;       /* max |a| over all pairs */
    float   v_min, v_max;         /* smallest / largest net output over the rows */
    int32_t fits_f16_split;       /* 1 iff bgamd_weights_check would accept this table */
    int32_t unit_saturated[128];  /* per hidden unit: rows on which it is saturated */
} bgamd_net_health_t;
int bgamd_net_health(const float *d_theta /*25601*/, const void *d_rows /*n_rows x 32 B*/, int64_t n_rows, float threshold,
                     bgamd_net_health_t *d_out, void *stream);

/* ---- choice spread: do the candidates of a turn still differ? ------------------------------------------------------------------------
 * Per lane, over exactly the rows bgamd_env_unique_rows_info / _read list for the last greedy step (copies still in that list count as
 * rows), without copying a row to the host: d_count[n] = the lane's rows; d_best[n] / d_worst[n] = the extreme values from the MOVER's
 * side, as stored (the mover is the row's turn bit; PLAYER1 plays the maximum, PLAYER2 the minimum -- the greedy step's rule, model.py:
 * 205-213); d_tied[n] = rows whose value is bit-equal to best.  A lane without rows (finished, frozen, left out by BGAMD_ONLY_P1/P2, or
 * without a legal move) reports count 0, best = worst = 0, tied 0.  With epsilon = 0, best is bit-equal to bgamd_env_last_choice's value
 * wherever count >= 1.  d_summary[4] = lanes with count >= 2, of those the lanes with tied == count (the tie rule alone chose the move),
 * total rows, lanes with count == 0.  Any pointer may be NULL.  A segmented reduction over the four arenas by game id; stream-ordered,
 * no side effect on the env (its per-lane scratch words aside).  Before the first greedy step: BGAMD_E_INVALID. */
int bgamd_env_choice_spread(bgamd_env *env, int32_t *d_count, float *d_best, float *d_worst, int32_t *d_tied,
                            int64_t *d_summary /*[4]*/, void *stream);

/* ---- trajectory log for the learner (the list of encodings play_game returns, train.py:105-106,
 * kept as 32-byte rows: 8 bit planes, turn of the side to move in plane 0 bit 31).  When set, every
 * greedy step stores the PRE-move row of each live lane at d_rows[(ply*n + lane)*32 B]; plies >=
 * max_plies are dropped.  NULL disables.  bgamd_env_get_progress copies ply / episode per lane
 * (a finished, frozen lane has ply = T-1).  bgamd_encode_rows: rows -> float[n][198]. */
int bgamd_env_set_trajectory(bgamd_env *env, void *d_rows, int64_t max_plies);
int bgamd_env_get_progress(bgamd_env *env, int32_t *d_ply, int32_t *d_episode, void *stream);

/* ---- ring log of CONTINUOUS self-play ---------------------------------------------------------------------------------
 * play_game (train.py:64-121) plays one game to the end; a round of them (train.py:527-547) on n lanes ends with a long tail of
 * nearly empty steps (mean game 83 turns, longest ~450: a 65 536-game round is ~460 steps for 5.5 M turns).  With BGAMD_AUTO_RESET a
 * lane starts its next game (episode + 1 of the lane: fresh dice, fresh opening roll) the step after the last one ended, every lane
 * is busy at every step, and the log is indexed by the ENV STEP instead of the lane's ply:
 *   d_rows [ring_steps][n] x 32 B : the pre-move row of lane g at env step k (k counted from this call) sits in slot k % ring_steps
 *   d_end  [ring_steps][n] uint16 : 0, or -- when the turn logged in that slot was the LAST of its game -- the game's number of logged
 *                                   turns (<= 32 767) | winner << 15 (0 = PLAYER1).  The game's turns are the `turns` slots ending there.
 * Only greedy steps (bgamd_env_step_greedy / run_greedy) log into the ring; every lane must take part in every step (no
 * BGAMD_ONLY_P1/P2).  Every game is one episode of one lane: the same game bgamd_env_reset_episode + a run to the end plays with the
 * same weights.  A caller that refreshes the weights between runs lets the games in flight go on under the new ones (TD-Gammon's own
 * self-play changes the weights after every move).  NULL disables.  bgamd_env_trajectory_step: env steps logged since the call.
 * Enforced (round 5): with a ring set, a greedy step without BGAMD_AUTO_RESET or with BGAMD_ONLY_P1/P2 returns BGAMD_E_INVALID.
 * bgamd_env_trajectory_step is a HOST counter bumped when a run is ENQUEUED: read the end records on the stream the run was issued on (or
 * after synchronising it) -- ContinuousSelfPlay.finished() does the former. */
int bgamd_env_set_trajectory_ring(bgamd_env *env, void *d_rows, int64_t ring_steps, uint16_t *d_end);
int64_t bgamd_env_trajectory_step(const bgamd_env *env);
int bgamd_encode_rows(const void *d_rows, int64_t n, float *d_out198, void *stream);

/* ---- stateless operators ----------------------------------------------------------------------
 * _encode_states_np (model.py:111-144) and forward (model.py:63-67) on caller-provided states. */
int bgamd_encode(const int32_t *d_states28, const int32_t *d_turn, int64_t n, float *d_out198, void *stream);
int bgamd_evaluate(bgamd_env *env, const int32_t *d_states28, const int32_t *d_turn, int64_t n,
                   int precision, float *d_values, void *stream);                       /* weight slot 0 */
int bgamd_evaluate_slot(bgamd_env *env, int slot, const int32_t *d_states28, const int32_t *d_turn, int64_t n,
                        int precision, float *d_values, void *stream);
/* The same values through the INCREMENTAL fp32 path of the greedy step (make_move's forward over the afterstates of
 * a turn, model.py:209-211): afterstate i is evaluated as its root position's hidden layer (one dense pass per root,
 * root d_root_index[i] of the n_roots given with the MOVER's turn, model.py:209) plus the W1 columns of the features
 * in which it differs from that root.  A row that differs from its root in more features than a legal turn changes
 * raises BGAMD_E_DELTA at the next bgamd_env_stats.  n_roots <= the env's lanes, n <= its arena rows; the env's
 * arenas are used as scratch (do not interleave with a step in flight on another stream). */
int bgamd_evaluate_incremental(bgamd_env *env, int slot, const int32_t *d_root_states28, const int32_t *d_root_turn,
                               int64_t n_roots, const int32_t *d_states28, const int32_t *d_root_index, int64_t n,
                               float *d_values, void *stream);

/* kernel timing hook for bench.py: brackets kernel groups with HIP events on the launch stream;
 * bgamd_env_kernel_times returns accumulated milliseconds and launch counts since the last call
 * (synchronises).  slots: 0 ordered enumerate, 1 value net, 2 apply, 3 random step,
 * 4 roots+expand (plies 1-3), 5 leaf stage, 6 root term of the incremental value net when it is a launch of its own (the first step of a run; every step of an env
 * below 24 576 lanes (experimental build: or with BGAMD_ROOT_IN_BOUNDARY=0) -- otherwise it runs inside the boundary launch, slot 2; the experimental build's BGAMD_OVERLAP=1 forks the launch onto the env's
 * second stream beside the doubles plies, rounds 1-3's default).  enable: 0 = off, 1 = every group, (mask << 8) | (stride << 20) = only the groups
 * whose bit is set in mask, on every stride-th launch of a group (0 = every launch; an event pair costs ~4 us of
 * stream time, so a timed run samples). */
/* "default" or "experimental" (-DBGAMD_EXPERIMENTAL: the kernels that lost their A/B are compiled in and their switches honoured --
 * BGAMD_MFMA_DELTA, BGAMD_F16X2_RESIDENT, BGAMD_ROOT_RESIDENT=0, BGAMD_ROOT_F32, BGAMD_TD_FUSED=0; the default build ignores them).
 * bgamd_env_kernel_choice: what the last greedy step actually launched -- h_out[0] value net: 0 eval_rows_delta_kernel, 1 eval_rows_mdelta_kernel,
 * 2 eval_rows_f32_kernel, 3 eval_rows_f16x2_kernel, 4 eval_rows_d16_kernel, 5 eval_rows_bf16_kernel; h_out[1] root pass: 0 none, 1
 * root_hidden_resident_kernel, 2 root_hidden_bf16x3_kernel, 3 eval_rows_f32_kernel<root>, 4 no launch of its own: it ran inside the
 * boundary launch of the step before (boundary_kernel<true>, every step of a run but the first); h_out[2]: bit 0 = root pass on the env's
 * second stream, bit 1 = the expansion below the roots (doubles plies 2-3 + leaf stage) ran as ONE launch (expand_all_kernel; the default,
 * the experimental build's BGAMD_EXPAND_MERGED=0 brings doubles_kernel + expand_kernel<LEAF> back); h_out[3]: 1 = experimental build.  bench.py labels its kernels
 * from this, not from the environment. */
const char *bgamd_build_flags(void);
int bgamd_env_kernel_choice(bgamd_env *env, int32_t h_out[4]);
int bgamd_env_time_kernels(bgamd_env *env, int enable);
int bgamd_env_kernel_times(bgamd_env *env, double h_ms[8], uint64_t h_launches[8]);
/* The internal envs as they stand: h_out = lanes of the env that scores the virtual roots of the 2-ply search, the move analysis, the
 * pre-roll evaluation and the rollouts' luck pass (kept while it has at least the lanes a call wants), of the rollouts' trial env
 * (exactly the last rollout's lanes) and of the 3-ply step's mid env (kept like the first); 0 where there is none yet.  Host values,
 * nothing is launched.  For tests of the history rule above: no result may depend on these numbers. */
int bgamd_env_scratch_info(bgamd_env *env, int64_t h_out[3]);

/* states (28 ints, reference getGameBoard layout) + turn -> 32-byte rows, the trajectory log's format */
int bgamd_pack_rows(const int32_t *d_states28, const int32_t *d_turn, int64_t n, void *d_rows, void *stream);

/* ---- TD(lambda) learner -----------------------------------------------------------------------------
 * Replaces apply_td_updates (pysrc/TD(λ) model/train.py:124-172) with the eligibility traces of
 * model.py:48-53 (reset per game, train.py:539-540), as a lock-step replay: step t updates EVERY game that has a
 * turn t from the same weights, and the per-game updates  fp32(α δ_g) · e_g  are summed (one game = the
 * reference's own update, step for step; many games = mini-batch TD(λ), the documented deviation).
 * Weights: flat float[25601] = fc1.weight[128][198] | fc1.bias[128] | fc2.weight[128] | fc2.bias[1].
 *
 * begin : d_rows = the env's trajectory log [T][n_lanes] x 32 B; d_order = the n_games lanes to replay, ordered by
 *         DECREASING d_length[lane] (so the games still running at step t are a prefix of the order);
 *         d_length[lane] in 1..T = number of logged turns, d_p1_won[lane] = 1 if PLAYER1 won (the terminal target z,
 *         train.py:165).  The buffers must stay valid until the last step.  Traces start at zero.
 * step  : step t over the first n_active games of the order: forward of s_t and s_{t+1}, δ = V(s_{t+1}) - V(s_t)
 *         (z - V(s_t) on a game's last turn), e <- λ e + ∇V(s_t), update = Σ_g fp32(alpha · δ_g) e_g with alpha·δ
 *         formed in float64 (train.py:147).  d_update == NULL: the update is applied to the weights.  Otherwise it is
 *         written to d_update[25601] and NOT applied: the caller all-reduces it over the ranks (the one collective
 *         of a training step) and calls bgamd_td_apply.
 * replay: steps 0..n_steps-1 with h_n_active[t] games each, applied locally.
 * stats : Σ δ² and the number of (game, step) updates since begin (synchronises). */
typedef struct bgamd_td bgamd_td;
int bgamd_td_create(bgamd_td **out, int64_t max_games, int device);
int bgamd_td_destroy(bgamd_td *td);
int bgamd_td_set_weights(bgamd_td *td, const float *d_theta, void *stream);
int bgamd_td_get_weights(bgamd_td *td, float *d_theta, void *stream);
int bgamd_td_begin(bgamd_td *td, const void *d_rows, int64_t T, int64_t n_lanes, const int32_t *d_order,
                   int64_t n_games, const int32_t *d_length, const uint8_t *d_p1_won, void *stream);
/* Streamed replay of a round (replaces the loop over a round's games of train.py:536-547 for rounds far larger than the
 * reference's): n_slots slots replay the round's games one after another -- slot i plays the games (lanes of the log)
 * d_queue[d_queue_offsets[i] .. d_queue_offsets[i + 1]), a game's step 0 following the terminal step of the game before it in
 * the next training step -- so every training step sums the TD(lambda) updates of n_slots games at DIFFERENT plies, and the
 * round takes max_i (sum of slot i's game lengths) steps instead of (sub-rounds) x (longest game).  A slot's trace restarts
 * with each game (train.py:133 reset_eligibility_traces).  Then bgamd_td_step(t, n_slots, ...) for t = 0, 1, ... (steps past a
 * slot's last game add nothing for it); t is not bounded by T here.  One game per slot == bgamd_td_begin with that order. */
/* Host-only helper (no device needed): the schedule of a streamed replay.  h_length[n_lanes] = logged turns per lane (<= 0: not
 * replayed).  Games are dealt longest first, each to the slot with the fewest turns so far, and every slot plays its share in a fixed
 * pseudo-random order.  -> h_queue[games] lanes in slot-major play order, h_queue_offsets[n_slots + 1], the number of games and the
 * number of training steps (= the largest slot total).  bgamd_td_begin_stream takes these two arrays (copied to the device). */
int bgamd_td_stream_schedule(const int32_t *h_length, int64_t n_lanes, int64_t n_slots, int32_t *h_queue, int32_t *h_queue_offsets,
                             int64_t *h_n_games, int64_t *h_n_steps);
int bgamd_td_begin_stream(bgamd_td *td, const void *d_rows, int64_t T, int64_t n_lanes, const int32_t *d_queue,
                          const int32_t *d_queue_offsets, int64_t n_slots, const int32_t *d_length, const uint8_t *d_p1_won,
                          void *stream);
/* The same over a GAME TABLE and a ring log (continuous self-play, bgamd_env_set_trajectory_ring): queue entries are game ids
 * 0 .. n_games-1; game i sits in column d_game_lane[i] of the log, its first turn in ring slot d_game_start[i], its turn k in slot
 * (d_game_start[i] + k) % ring_steps; d_length / d_p1_won are indexed by game id.  bgamd_td_stream_schedule takes d_length as it is. */
int bgamd_td_begin_stream_games(bgamd_td *td, const void *d_rows, int64_t ring_steps, int64_t n_lanes, const int32_t *d_queue,
                                const int32_t *d_queue_offsets, int64_t n_slots, int64_t n_games, const int32_t *d_game_lane,
                                const int32_t *d_game_start, const int32_t *d_length, const uint8_t *d_p1_won, void *stream);
int bgamd_td_step(bgamd_td *td, int64_t t, int64_t n_active, double alpha, float lambda, float *d_update, void *stream);
int bgamd_td_apply(bgamd_td *td, const float *d_update, void *stream);
int bgamd_td_replay(bgamd_td *td, int64_t n_steps, const int64_t *h_n_active, double alpha, float lambda, void *stream);
/* Delayed update, opt-in (delay = 1; 0 = exact, the default): bgamd_td_replay applies the update of step t one step LATE -- step t + 1 runs on
 * the weights of step t plus the update of step t - 1 -- whenever the replay is a streamed one through a constant number of slots that takes the
 * fused training step with >= 201 workgroups (512 ... 4 096 slots on 256 CUs; anything else replays exactly).  The step's reduction then has a
 * whole step to happen in and a training step is ONE launch instead of two (csrc/bg_learner.h: the reduction of step t - 1 rides on the waves
 * that idle during step t's forward pass).  A documented deviation from train.py:136-170, where every update is applied before the next state
 * is evaluated: with thousands of games summed per step a one-step delay is a perturbation of the step ORDER, not of what is learned (quality:
 * profiles/r04_training_quality.txt) -- but ONE game no longer reproduces the reference's update step for step, so fixtures G6 / G9 hold for
 * delay = 0 only.  bgamd_td_step / bgamd_td_step_allreduce are always exact. */
int bgamd_td_set_delay(bgamd_td *td, int delay);
/* ---- the one collective of a multi-rank training step, issued by the library ("one all-reduce of 25 601 fp32 per
 * training step, RCCL over xGMI, in place, on the compute stream"; train.py:536-547 is the loop it scales).  The learner owns an RCCL
 * communicator: rank 0 calls bgamd_td_comm_unique_id, the 128 bytes reach the other ranks by whatever the launcher has
 * (torch.distributed broadcast, a file), every rank calls bgamd_td_comm_init (collective: returns when all ranks have).  RCCL is
 * resolved at run time (the librccl.so.1 already in the process, else the ROCm install's; BGAMD_RCCL_LIB overrides).
 *   step_allreduce  : bgamd_td_step with the update handed out -> ncclAllReduce(sum, in place) -> bgamd_td_apply, three enqueues on
 *                     `stream`, no host synchronisation; n_active = 0: the rank adds nothing at step t but joins the collective
 *   replay_allreduce: steps 0 .. n_steps-1 (the MAX over the ranks); this rank's own log covers the first n_own_steps of them */
int bgamd_td_comm_unique_id(uint8_t h_id[128]);
int bgamd_td_comm_init(bgamd_td *td, const uint8_t h_id[128], int rank, int world);
int bgamd_td_comm_destroy(bgamd_td *td);
int bgamd_td_step_allreduce(bgamd_td *td, int64_t t, int64_t n_active, double alpha, float lambda, void *stream);
int bgamd_td_replay_allreduce(bgamd_td *td, int64_t n_steps, const int64_t *h_n_active, int64_t n_own_steps, double alpha, float lambda,
                              void *stream);
/* (the readers below wait for the stream the replay was issued on, not for the device: a learner replaying on its own stream beside
 * an env at play does not wait for the env) */
int bgamd_td_stats(bgamd_td *td, double *h_sq_sum, int64_t *h_updates);
/* Traffic report of the column-sparse traces: Σ over the (game, step) updates since begin of the W1 trace columns that
 * were touched (of 198; a column = 128 floats, read + written).  BGAMD_TD_DENSE=1 in the environment at bgamd_td_create
 * keeps every column active (the dense pass: same results bit for bit, 198 columns per update).  Synchronises. */
int bgamd_td_active_columns(bgamd_td *td, uint64_t *h_columns);
/* ... and of the columns that were WRITTEN.  The stored trace is e / c with one scale c = Π λ for all games of the replay
 * (train.py:150-158's e <- λ e + ∇ becomes ê <- ê + ∇ / c), so a column whose feature is zero in s_t is read but not written;
 * c is folded back in by an ordinary pass when it leaves [2^-40, 2^40].  BGAMD_TD_LAZY=0 at bgamd_td_create: every step is an
 * ordinary pass (written = active).  Synchronises. */
int bgamd_td_written_columns(bgamd_td *td, uint64_t *h_columns);
/* Diagnostics: the replay's slots (lock-step: one per game) -> int32 h_out[n][6] = (lane, length, p1_won, start step) of the game
 * a slot holds (length 0: none), the slot's queue cursor (-1 in a lock-step replay), its (game, step) updates so far.  Synchronises. */
int bgamd_td_slots(bgamd_td *td, int32_t *h_out);
/* HIP-event time of the trace kernel since the last call: enable with bgamd_td_time(td, 1).  A step of 512 .. 4 096 slots runs its forward pass
 * INSIDE the trace launch (td_step_fused_kernel): the bracket then holds both, and bytes / time derived from it understate the trace pass
 * (BGAMD_TD_FUSE_STEP=0 at bgamd_td_create separates them again: forward kernel, trace kernel, reduce kernel). */
int bgamd_td_time(bgamd_td *td, int enable);
int bgamd_td_times(bgamd_td *td, double *h_trace_ms, uint64_t *h_launches, uint64_t *h_game_steps);

/* ---- supervised step: fit the value net to real-valued targets (rollout means, search values) --------------------------------
 * d_rows = n rows of 32 B (bgamd_pack_rows; the turn bit is the side to move), d_target = n floats, y_i = P(PLAYER1 wins) of row i.
 *   update = Σ_i fp32(alpha · δ_i) ∇V(x_i), δ_i = y_i - V(x_i) in fp32, alpha·δ formed in float64 (train.py:147)
 * -- bgamd_td_step's update of a terminal step with e = ∇ and a real-valued z: the squared-error gradient step of the reference's own
 * learner.  A row whose target is not finite adds nothing and is counted as skipped.  d_update == NULL: the update is applied to the
 * weights, and every copy of them the TD kernels read is refreshed as after a TD step.  Otherwise it is written to d_update[25601] and
 * NOT applied: the caller all-reduces it and calls bgamd_td_apply, as with bgamd_td_step.  n = 0 is allowed (d_rows and d_target may
 * be NULL): a zero update, so that a rank without rows joins the collective.  n is not bounded by max_games: the rows are walked in
 * chunks of 65 536 (BGAMD_FIT_CHUNK at bgamd_td_create: another multiple of 32).  Stream-ordered, no host wait, no bgamd_td_begin
 * needed.  Deterministic: the same rows, targets, weights and alpha give the same bits (csrc/bg_fit.h states the order of the sums).
 * Call it BETWEEN replays: it leaves traces, slots, queue cursors, bgamd_td_stats and the column counters as they are, but uses the
 * replay's buffer of partial sums, so it must not be enqueued between the steps of a replay with a delayed update pending
 * (bgamd_td_set_delay) or on another stream than a replay still in flight.
 * fit_stats: Σ δ², the rows that counted and the rows skipped since bgamd_td_create or the last call of it; waits for the stream of
 * the last fit step, which must still exist (before any fit step: the null stream).  BGAMD_FIT_CHUNK and BGAMD_FIT_GROUPS (most
 * workgroups per launch, 1 .. 256) are read at bgamd_td_create: test hooks that reach several chunks and several tiles per workgroup
 * with few rows; both change the order of the sums (csrc/bg_fit.h), not what is summed. */
int bgamd_td_fit_step(bgamd_td *td, const void *d_rows, const float *d_target, int64_t n, double alpha, float *d_update, void *stream);
int bgamd_td_fit_stats(bgamd_td *td, double *h_sq_sum, int64_t *h_rows, int64_t *h_skipped);
/* ... with the library's own collective (bgamd_td_comm_init): fit step -> ncclAllReduce(sum, in place) -> bgamd_td_apply, three
 * enqueues on `stream`; n = 0: the rank adds nothing but joins. */
int bgamd_td_fit_step_allreduce(bgamd_td *td, const void *d_rows, const float *d_target, int64_t n, double alpha, void *stream);

#ifdef __cplusplus
}
#endif
#endif
