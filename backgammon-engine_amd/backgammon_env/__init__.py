"""`backgammon_env` -- host-side mirror of the reference's pybind11 module of the same name
(cppsrc/backgammon_bindings.cpp:41-94), running on MI355X through libbgamd.so.

Same names, argument meaning and error behaviour as the reference module:
    PlayerType, Player, Pieces, Game           (scalar surface: one board = a one-lane env)
plus the vectorised surface the batched self-play loop uses:
    VecGame                                    (n boards per device, one board per lane)
and, in `backgammon_env.policy`, the TDLGammonModel operators (encode / forward / make_move).

Everything that computes runs in HIP kernels; there is no CPU fallback.  PyTorch is used only
to own device buffers and streams.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import enum
import os

# The greedy step runs its root pass on a second stream beside the doubles plies; ROCm maps streams onto GPU_MAX_HW_QUEUES (default 4)
# hardware queues, and a process that also holds an RCCL communicator has more streams than that: the env's two then share a queue and
# every step loses the overlap (0.153 -> 0.167 ms at 65 536 lanes).  The variable is read when the HIP runtime starts: this default
# takes effect when the package is imported before the first GPU call (multi-rank launchers: export it).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np
import torch

from . import _capi
from ._capi import (AUTO_RESET, BF16, CUBE_HOLD_TURN0, CUBE_JACOBY, CUBE_ON, F16X2, F32, F32_DENSE, MATCH_ON, NO_FLIP, ONLY_P1,  # noqa: F401
                    ONLY_P2, ROLL, ROLLOUT_ROTATE, ROLLOUT_VR, WANT_INDEX, WEIGHTS_SLOT1, BgamdError)
from .match import Match, MatchTable  # noqa: F401

__all__ = ["PlayerType", "Player", "Pieces", "Game", "VecGame", "Cube", "Match", "MatchTable", "BgamdError", "set_seed", "pack_rows", "outcomes"]


@dataclasses.dataclass
class Cube:
    """The doubling cube of VecGame.rollout(cube=...) (include/bgamd.h, bgamd_env_rollout_cube).  Before a turn the side to roll, with
    access to the cube and w its chance to win by the pre-roll evaluation, doubles iff double_at <= w <= too_good_at; the other side
    passes iff w > pass_at.  The defaults are a plain money-play rule of thumb, no measured optimum.  max_cube: no double at or beyond
    it.  jacoby: a trial whose cube was never turned in the trial counts as a single game.  hold_turn0: no decision before a trial's
    turn 0 (the roller holds the cube this turn: the "no double" line of a cube action).  value / owner: the cube at the start, a
    scalar or one entry per position (a power of two; 0 = the centre, 1 = PLAYER1 owns it, 2 = PLAYER2); None = 1, centred."""
    double_at: float = 0.70
    pass_at: float = 0.78
    too_good_at: float = 1.0
    max_cube: int = 64
    jacoby: bool = False
    hold_turn0: bool = False
    value: object = None
    owner: object = None

ERR_MESSAGES = {                                   # cppsrc/game.cpp:585-642, in source order
    0: "", 1: "Invalid origin", 2: "Origin out of range", 3: "Destination out of range",
    4: "Cannot move in that direction.", 5: "Move does not match dice.", 6: "Invalid destination.",
    7: "Cannot bear off from jail",
}

# the 21 unordered rolls in the order of VecGame.evaluate_preroll's columns (and of the search): (1,1), (1,2), ..., (1,6), (2,2), ..., (6,6)
ROLLS = [(a, b) for a in range(1, 7) for b in range(a, 7)]

_seed = int.from_bytes(os.urandom(8), "little")    # reference: random_device (game.hpp:45)
_next_scalar_id = 0


def set_seed(seed: int):
    """Seeds the dice of scalar Game objects created afterwards (the reference cannot be seeded)."""
    global _seed, _next_scalar_id
    _seed = int(seed) & (2 ** 64 - 1)
    _next_scalar_id = 0                  # (pooled envs are re-seeded when they are handed out: Game.__init__)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def pack_rows(states28, turn, device="cuda"):
    """[..., 28] reference-layout states + turn (scalar or [...]) -> int32 [..., 8] 32-byte rows (the trajectory
    log's format: 8 bit planes, turn of the side to move in plane 0 bit 31)."""
    st = torch.as_tensor(states28, dtype=torch.int32).to(device).contiguous()
    lead = st.shape[:-1]
    n = st.numel() // 28
    t = torch.as_tensor(turn, dtype=torch.int32).to(device).expand(lead).contiguous()
    out = torch.empty((n, 8), dtype=torch.int32, device=st.device)
    _capi.check(_capi.load().bgamd_pack_rows(_ptr(st), _ptr(t), n, _ptr(out), _stream()), "pack_rows")
    return out.reshape(*lead, 8)


def outcomes(states28, device="cuda"):
    """[..., 28] reference-layout states -> int32 [...] points from PLAYER1's side (include/bgamd.h, bgamd_outcomes): 0 = not over,
    +1 / +2 / +3 = PLAYER1 won a single game / a gammon / a backgammon, -1 / -2 / -3 = PLAYER2 did; a state with |count| > 15 gives
    _capi.OUTCOME_BAD."""
    st = torch.as_tensor(states28, dtype=torch.int32).to(device).contiguous()
    lead = st.shape[:-1]
    n = st.numel() // 28
    out = torch.empty((n,), dtype=torch.int32, device=st.device)
    _capi.check(_capi.load().bgamd_outcomes(_ptr(st), n, _ptr(out), _stream()), "outcomes")
    return out.reshape(lead)


class PlayerType(enum.IntEnum):                    # bindings.cpp:46-48 (unscoped enum: equals ints)
    PLAYER1 = 0
    PLAYER2 = 1


PLAYER1, PLAYER2 = PlayerType.PLAYER1, PlayerType.PLAYER2


class Player:                                      # bindings.cpp:51-54, cppsrc/player.hpp:6-27
    def __init__(self, name: str, num: PlayerType):
        if not isinstance(name, str) or not isinstance(num, PlayerType):
            raise TypeError("Player(name: str, num: PlayerType)")
        self._name, self._num = name, int(num)

    def getName(self):
        return self._name

    def getNum(self):
        return self._num


class Pieces:                                      # bindings.cpp:57-59: live view of a Game's counters
    def __init__(self, game: "Game"):
        self._game = game

    def numJailed(self, player):
        return self._game.getJailedCount(player)

    def numFreed(self, player):
        return self._game.getBornOffCount(player)


class VecGame:
    """n concurrent games on one MI355X, one board per lane (include/bgamd.h)."""

    def __init__(self, n_games: int, device: int = 0, seed: int = 20240603, lane_offset: int = 0,
                 lane_stride: int | None = None, arena_rows: int = 0):
        self._lib = _capi.load()
        if not torch.cuda.is_available():
            raise BgamdError("no GPU visible: backgammon_env has no CPU fallback")
        self.n = int(n_games)
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        _capi.check(self._lib.bgamd_env_create(C.byref(h), self.n, device, seed, lane_offset,
                                               lane_stride or 0, arena_rows), "bgamd_env_create")
        self._h = h
        self._has_weights = False
        self._rollout_shape = (0, 0)       # P, T of the last rollout (rollout_outcomes_read)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bgamd_env_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers
    def _buf(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _dev(self, x, dtype, shape):
        t = torch.as_tensor(x, dtype=dtype).to(self.device).contiguous()
        if tuple(t.shape) != tuple(shape):
            t = t.expand(shape).contiguous()
        return t

    # -- state
    def reset(self, mask=None, episode=None):
        """mask=None: every lane back to episode 0 (counters cleared).  mask [n]: only the lanes with mask != 0 restart
        (next episode).  episode=k: every lane starts its episode k -- global game id lane_offset + lane + k * lane_stride,
        i.e. fresh dice and a fresh opening roll for every round of a one-game-per-lane training loop."""
        if episode is not None:
            _capi.check(self._lib.bgamd_env_reset_episode(self._h, int(episode), _stream()), "reset_episode")
            return
        if mask is None:
            _capi.check(self._lib.bgamd_env_reset(self._h, _stream()), "reset")
            return
        m = self._dev(mask, torch.int32, (self.n,))
        _capi.check(self._lib.bgamd_env_reset_lanes(self._h, _ptr(m), _stream()), "reset_lanes")
        torch.cuda.current_stream().synchronize()

    def reseed(self, seed: int, lane_offset: int = 0, lane_stride: int = 0, null_stream: bool = False):
        """The dice streams of a freshly created env with these arguments, on this one (episode 0, start position)."""
        st = None if null_stream else _stream()
        _capi.check(self._lib.bgamd_env_reseed(self._h, int(seed) & (2 ** 64 - 1), int(lane_offset), int(lane_stride), st), "reseed")

    def set_states(self, states28=None, turn=None):
        s = self._dev(states28, torch.int32, (self.n, 28)) if states28 is not None else None
        t = self._dev(turn, torch.int32, (self.n,)) if turn is not None else None
        _capi.check(self._lib.bgamd_env_set_states(self._h, _ptr(s), _ptr(t), _stream()), "set_states")
        torch.cuda.current_stream().synchronize()     # s / t may be temporaries

    def states(self):
        s = self._buf((self.n, 28), torch.int32)
        _capi.check(self._lib.bgamd_env_get_states(self._h, _ptr(s), None, _stream()), "get_states")
        return s

    def turns(self):
        t = self._buf((self.n,), torch.int32)
        _capi.check(self._lib.bgamd_env_get_states(self._h, None, _ptr(t), _stream()), "get_states")
        return t

    def flags(self):
        f = self._buf((self.n,), torch.int32)
        _capi.check(self._lib.bgamd_env_get_flags(self._h, _ptr(f), _stream()), "get_flags")
        return f

    def outcomes(self):
        """int32 [n]: the points of every lane's CURRENT board from PLAYER1's side (bgamd_env_outcomes) -- +-1 single game, +-2 gammon,
        +-3 backgammon for a lane frozen on its final board (finished without auto_reset); 0 for a lane still playing or auto-reset."""
        o = self._buf((self.n,), torch.int32)
        _capi.check(self._lib.bgamd_env_outcomes(self._h, _ptr(o), _stream()), "outcomes")
        return o

    def snapshot(self):
        """int32 [n, 32] = state28 | turn | die1 | die2 | flags: every scalar getter's data in one launch."""
        out = self._buf((self.n, 32), torch.int32)
        _capi.check(self._lib.bgamd_env_snapshot(self._h, _ptr(out), _stream()), "snapshot")
        return out

    def set_dice(self, dice):
        d = self._dev(dice, torch.int32, (self.n, 2))
        _capi.check(self._lib.bgamd_env_set_dice(self._h, _ptr(d), _stream()), "set_dice")
        torch.cuda.current_stream().synchronize()

    def dice(self):
        d = self._buf((self.n, 2), torch.int32)
        _capi.check(self._lib.bgamd_env_get_dice(self._h, _ptr(d), _stream()), "get_dice")
        return d

    def roll(self, advance_ply: bool = False):
        _capi.check(self._lib.bgamd_env_roll(self._h, int(advance_ply), _stream()), "roll")

    # -- enumeration (evaluateTurnSequences for every lane)
    def enumerate(self, player=None, dice=None):
        """-> (offsets int64[n], counts int32[n], states int32[N,28], seq int8[N,4,2], seq_len int32[N]),
        rows of lane g = [offsets[g], offsets[g]+counts[g]), reference order."""
        p = self._dev(player, torch.int32, (self.n,)) if player is not None else None
        d = self._dev(dice, torch.int32, (self.n, 2)) if dice is not None else None
        _capi.check(self._lib.bgamd_env_enumerate(self._h, _ptr(p), _ptr(d), _stream()), "enumerate")
        offs, cnts = self._buf((self.n,), torch.int64), self._buf((self.n,), torch.int32)
        total = _capi.check(self._lib.bgamd_env_candidates_info(self._h, _ptr(offs), _ptr(cnts), _stream()),
                            "candidates_info")
        st = self._buf((total, 28), torch.int32)
        sq = self._buf((total, 4, 2), torch.int8)
        ln = self._buf((total,), torch.int32)
        _capi.check(self._lib.bgamd_env_candidates_read(self._h, 0, total, _ptr(st), _ptr(sq), _ptr(ln), _stream()),
                    "candidates_read")
        return offs, cnts, st, sq, ln

    # -- the env step
    def load_weights(self, weights, slot: int = 0):
        """slot 0 | 1 (head-to-head play keeps one weight set per side).  weights: flat float32[25601] = W1[128,198] | b1[128] | W2[128] | b2[1], or a state_dict with
        fc1.weight / fc1.bias / fc2.weight / fc2.bias (the reference checkpoints, train.py:513-515)."""
        if isinstance(weights, dict):
            weights = np.concatenate([np.asarray(weights[k].detach().cpu().float()).ravel()
                                      for k in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")])
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).ravel())
        if w.size != 25601:
            raise ValueError("expected 25601 weights (198->128->1)")
        _capi.check(self._lib.bgamd_env_load_weights_slot(self._h, int(slot), w.ctypes.data_as(C.c_void_p)), "load_weights")
        self._has_weights = True

    @staticmethod
    def _flags(roll, auto_reset, no_flip=False, only_player=None, slot=0):
        f = (ROLL if roll else 0) | (AUTO_RESET if auto_reset else 0) | (NO_FLIP if no_flip else 0)
        if only_player is not None:
            f |= ONLY_P1 if int(only_player) == 0 else ONLY_P2
        return f | (WEIGHTS_SLOT1 if slot else 0)

    def step_random(self, roll=True, auto_reset=True, choice_u32=None, no_flip=False, only_player=None, walk=False):
        """walk=True: the one-lane-per-game whole-tree walk instead of the bounded task kernels (same result)."""
        c = None
        if choice_u32 is not None:
            c = torch.as_tensor(np.asarray(choice_u32, dtype=np.uint32).view(np.int32)).to(self.device).contiguous()
        fn = self._lib.bgamd_env_step_random_walk if walk else self._lib.bgamd_env_step_random
        _capi.check(fn(self._h, self._flags(roll, auto_reset, no_flip, only_player), _ptr(c), _stream()), "step_random")
        if c is not None:
            torch.cuda.current_stream().synchronize()

    def step_greedy(self, roll=True, auto_reset=True, epsilon=0.0, precision=F32, no_flip=False, want_index=False,
                    only_player=None, slot=0):
        """want_index: also report the chosen reference-order index and the list length (slow path).
        only_player / slot: head-to-head play -- step only the lanes of that side with weight slot `slot`."""
        _capi.check(self._lib.bgamd_env_step_greedy(self._h, self._flags(roll, auto_reset, no_flip, only_player, slot) |
                                                    (WANT_INDEX if want_index else 0), float(epsilon),
                                                    int(precision), _stream()), "step_greedy")

    def run_greedy(self, n_steps, roll=True, auto_reset=True, epsilon=0.0, precision=F32, only_player=None, slot=0):
        """n_steps greedy steps in one call: the same games as n_steps calls of step_greedy, with the apply of one
        step and the roots of the next sharing a launch."""
        _capi.check(self._lib.bgamd_env_run_greedy(self._h, self._flags(roll, auto_reset, False, only_player, slot),
                                                   float(epsilon), int(precision), int(n_steps), _stream()), "run_greedy")

    def step_sampled(self, temperature, roll=True, auto_reset=True, precision=F32, no_flip=False, want_index=False, only_player=None,
                     slot=0):
        """A greedy step in which every lane plays an afterstate drawn with probability ~ exp(value for the mover / temperature) over the
        distinct afterstates the net scored (include/bgamd.h, bgamd_env_step_sampled: Gumbel-max, noise keyed by seed, game id, ply and
        the afterstate).  temperature 0 is step_greedy, bit for bit; negative, NaN or inf raises.  last_choice() reports the sampled
        move and its value; the other arguments mean what they mean for step_greedy."""
        _capi.check(self._lib.bgamd_env_step_sampled(self._h, self._flags(roll, auto_reset, no_flip, only_player, slot) |
                                                     (WANT_INDEX if want_index else 0), float(temperature), int(precision), _stream()),
                    "step_sampled")

    def run_sampled(self, n_steps, temperature, roll=True, auto_reset=True, precision=F32, only_player=None, slot=0):
        """n_steps sampled steps in one call: the same games as n_steps calls of step_sampled (run_greedy's fused step boundary)."""
        _capi.check(self._lib.bgamd_env_run_sampled(self._h, self._flags(roll, auto_reset, False, only_player, slot), float(temperature),
                                                    int(precision), int(n_steps), _stream()), "run_sampled")

    def sample_info(self):
        """Host values of the last step_sampled / run_sampled with temperature > 0 (summed over a run's steps; synchronises): [lanes that
        had a move, lanes whose played value is not their best value].  Raises before the first such call."""
        h = (C.c_int64 * 2)()
        _capi.check(self._lib.bgamd_env_sample_info(self._h, h), "sample_info")
        return list(h)

    def step_search(self, top_k=8, roll=True, auto_reset=True, no_flip=False, want_index=False, only_player=None, slot=0, margin=None,
                    plies=2, deep_k=2, deep_margin=float("inf"), reply_top_k=2, reply_margin=float("inf")):
        """One 2-ply expectimax turn (include/bgamd.h, bgamd_env_step_search): the top_k best afterstates by the net (0 = all
        distinct ones) are re-scored by the average over the opponent's 21 rolls of the opponent's greedy reply, and the best of
        them is played.  last_choice()["value"] is that 2-ply value; search_candidates() lists the kept candidates.
        margin (None = the step above): the filtered step (bgamd_env_step_search_filtered) -- only the candidates whose 1-ply value lies
        within `margin` (>= 0, may be inf) of the best are searched, and a lane that keeps one candidate plays it unsearched (its value
        and v2 are its 1-ply value).  Synchronises once.
        plies = 3 (bgamd_env_step_search3): the filtered step (margin None = inf) whose best candidates by the 2-ply value -- at most
        deep_k (0 = all), within deep_margin of the best -- are searched one ply deeper: the opponent answers each of its 21 rolls with
        the best of its reply_top_k (0 = all) replies within reply_margin by THEIR 2-ply value.  last_choice()["value"] is the deepest value
        the chosen move received; search_candidates() adds v3 and depth, search3_info() counts the work.  Synchronises twice and once per
        chunk of the mid level.  The deep parameters are ignored at plies = 2."""
        flags = self._flags(roll, auto_reset, no_flip, only_player, slot) | (WANT_INDEX if want_index else 0)
        if plies not in (2, 3):
            raise ValueError("plies must be 2 or 3")
        if plies == 3:
            _capi.check(self._lib.bgamd_env_step_search3(self._h, flags, int(top_k), float("inf") if margin is None else float(margin),
                                                         int(deep_k), float(deep_margin), int(reply_top_k), float(reply_margin), _stream()),
                        "step_search3")
        elif margin is None:
            _capi.check(self._lib.bgamd_env_step_search(self._h, flags, int(top_k), _stream()), "step_search")
        else:
            _capi.check(self._lib.bgamd_env_step_search_filtered(self._h, flags, int(top_k), float(margin), _stream()), "step_search_filtered")
        self._search_k, self._search_plies = int(top_k), int(plies)      # (of the last step that was accepted: a refused one changes no read)

    def search_info(self):
        """Host values of the last search step of either kind (bgamd_env_search_info; synchronises): [lanes that had a move, lanes
        searched, kept candidates, virtual roots scored]."""
        h = (C.c_int64 * 4)()
        _capi.check(self._lib.bgamd_env_search_info(self._h, h), "search_info")
        return list(h)

    def search3_info(self):
        """Host values of the last 3-ply search step (bgamd_env_search3_info; synchronises): [lanes that had a move, lanes searched at 2
        plies, lanes searched at 3 plies, deep candidates, mid lanes, level-3 virtual roots scored].  Raises unless the last search step
        was a 3-ply one."""
        h = (C.c_int64 * 6)()
        _capi.check(self._lib.bgamd_env_search3_info(self._h, h), "search3_info")
        return list(h)

    def search_candidates(self):
        """The last search step's kept candidates, best 1-ply value first: (states[n,K,28], v1[n,K], v2[n,K], kept[n]); K is
        that step's top_k, or (top_k = 0) the largest kept count.  Slots past a lane's count are zero.  After a 3-ply step
        (step_search(plies=3)) two more follow: v3[n,K] (0 where depth < 3) and depth[n,K] int32, the deepest value the candidate
        received: 1, 2 or 3, and 0 past the lane's count."""
        kept = self._buf((self.n,), torch.int32)
        _capi.check(self._lib.bgamd_env_search_read(self._h, None, None, None, _ptr(kept), _stream()), "search_read")
        K = getattr(self, "_search_k", 0)
        if K == 0:
            K = int(kept.max().item()) if self.n else 0
        st = self._buf((self.n, K, 28), torch.int32)
        v1, v2 = self._buf((self.n, K), torch.float32), self._buf((self.n, K), torch.float32)
        if K > 0:
            _capi.check(self._lib.bgamd_env_search_read(self._h, _ptr(st), _ptr(v1), _ptr(v2), None, _stream()), "search_read")
        if getattr(self, "_search_plies", 2) == 3:
            v3, depth = self._buf((self.n, K), torch.float32), self._buf((self.n, K), torch.int32)
            _capi.check(self._lib.bgamd_env_search3_read(self._h, _ptr(v3), _ptr(depth), _stream()), "search3_read")
            return st, v1, v2, kept, v3, depth
        return st, v1, v2, kept

    ANALYSIS_FIELDS = (("status", torch.int32), ("distinct", torch.int32), ("rank1", torch.int32), ("rank2", torch.int32),
                       ("v1_played", torch.float32), ("v1_best", torch.float32), ("v2_played", torch.float32),
                       ("v2_best", torch.float32), ("error", torch.float32))

    def analyze_moves(self, played, top_k=4, only_player=None, slot=0):
        """Move analysis (include/bgamd.h, bgamd_env_analyze_moves): `played` [n, 28] is the afterstate played from each lane's current
        board, side to move and dice; it is judged against a 2-ply search over the top_k best afterstates by the net (0 = all) and
        itself.  Nothing is applied.  -> dict of device tensors [n]: status (0 analysed, 1 idle, 2 no move, 3 not an afterstate), distinct,
        rank1, rank2, v1_played, v1_best, v2_played, v2_best, error, best [n, 28], summary_raw (float64 [12]) -- and summary, the same
        twelve numbers by name: player1 / player2 -> decisions, unforced, mistakes, error_sum, max_error; no_move; not_found
        (synchronises for them)."""
        st = self._dev(played, torch.int32, (self.n, 28))
        _capi.check(self._lib.bgamd_env_analyze_moves(self._h, self._flags(False, False, False, only_player, slot), int(top_k), _ptr(st),
                                                      _stream()), "analyze_moves")
        out = {k: self._buf((self.n,), dt) for k, dt in self.ANALYSIS_FIELDS}
        out["best"] = self._buf((self.n, 28), torch.int32)
        out["summary_raw"] = self._buf((12,), torch.float64)
        _capi.check(self._lib.bgamd_env_analysis_read(self._h, *[_ptr(out[k]) for k, _ in self.ANALYSIS_FIELDS], _ptr(out["best"]),
                                                      _ptr(out["summary_raw"]), _stream()), "analysis_read")
        s = out["summary_raw"].cpu().tolist()             # (synchronises: `st` may be a temporary)
        side = lambda v: {"decisions": int(v[0]), "unforced": int(v[1]), "mistakes": int(v[2]), "error_sum": v[3], "max_error": v[4]}
        out["summary"] = {"player1": side(s[0:5]), "player2": side(s[5:10]), "no_move": int(s[10]), "not_found": int(s[11])}
        return out

    def evaluate_preroll(self, states28, turn, slot=0):
        """1-ply pre-roll evaluation (include/bgamd.h, bgamd_env_evaluate_preroll): for each position with `turn` to roll, the value of the
        greedy step's choice for each of the 21 rolls in ROLLS' order (the net's value of the position when the roll has no move; the
        outcome for a position that is over) and their probability-weighted mean.  -> (roll_values [n, 21] float32, mean [n] float64)"""
        st = torch.as_tensor(states28, dtype=torch.int32).to(self.device).contiguous().reshape(-1, 28)
        n = st.shape[0]
        t = self._dev(turn, torch.int32, (n,))
        f, m = self._buf((n, 21), torch.float32), self._buf((n,), torch.float64)
        _capi.check(self._lib.bgamd_env_evaluate_preroll(self._h, WEIGHTS_SLOT1 if slot else 0, _ptr(st), _ptr(t), n, _ptr(f), _ptr(m),
                                                         _stream()), "evaluate_preroll")
        return f, m

    def rollout(self, states28, turn, trials, max_plies=0, rotate=True, seed=20240603, slot=0, position_offset=0, lanes=0,
                per_trial=False, variance_reduction=False, outcomes=False, plies=1, top_k=4, margin=float("inf"), groups=None,
                group_offset=0, cube=None, match=None):
        """Monte Carlo rollouts (include/bgamd.h, bgamd_env_rollout): `trials` greedy games from each of the P positions (turn = side to
        move), trial i of position p with the TURN-stream dice of game id (position_offset + p) * trials + i; rotate: the first turn of
        trial i uses ordered dice pair i % 36.  max_plies > 0 stops a trial after that many turns and scores it by the fp32 net.  This
        env's weights (slot) are used; its own lanes are untouched.  -> dict of device tensors: mean [P] (float64, the share of PLAYER1
        wins), stderr [P], turns [P] (int64), truncated [P] (int32); per_trial: also trial_value [P, T] (float32), trial_turns [P, T].
        variance_reduction: also the luck-adjusted vr_mean [P] and vr_stderr [P] (float64; BGAMD_ROLLOUT_VR: every turn's luck against
        the pre-roll evaluation is subtracted from the trial's value), with per_trial trial_luck [P, T] (float64); the plain outputs are
        the same as without it.
        outcomes: also the games in points (bgamd_env_rollout_outcomes_read) -- counts [P, 6] (int64: trials that ended as PLAYER1 single
        game, gammon, backgammon, PLAYER2 single game, gammon, backgammon; truncated trials are in none), equity [P] and equity_stderr [P]
        (float64, PLAYER1's cubeless equity in points; a truncated trial counts 2 x - 1 of its net value x), with per_trial trial_points
        [P, T] (int8, 0 = truncated).  The other outputs are the same as without it.
        plies = 2: every turn of every trial is chosen by the filtered 2-ply search with (top_k, margin) instead of the greedy step
        (bgamd_env_rollout_policy, set for this call; 1 is put back afterwards).  Same trials, same dice.
        groups (int sequence or tensor [P]): dice groups (bgamd_env_rollout_grouped) -- trial i of position p rolls the dice of game id
        (group_offset + groups[p]) * trials + i instead, so the positions of a group share their trials' dice; every output stays indexed
        by position, and position p's are those of the single-position call with position_offset = group_offset + groups[p].
        rollout_paired() then reads the differences inside a group.  groups with a non-zero position_offset: ValueError.
        cube (a Cube, or a dict of its fields): the doubling cube on the same trials (bgamd_env_rollout_cube, set for this call and
        switched off afterwards) -- also cubeful [P], cubeful_stderr [P] (float64, PLAYER1's cubeful money equity in points) and
        cube_counts [P, 4] (int64: trials PLAYER1 passed, trials PLAYER2 passed, cube turns, trials that ended at max_cube), with
        per_trial trial_cubeful [P, T] (float64), trial_cube [P, T] (int32, the final cube), trial_dropped [P, T] (int32, the turn of
        the drop or -1).  The other outputs are the same as without it.  The cube decides on the luck pass's pre-roll means: cube
        without variance_reduction is a ValueError.
        match (a backgammon_env.Match; needs cube=, else ValueError): the cube is handled by the thresholds of each position's match
        score and the trials are worth match-winning chances (bgamd_env_rollout_match, set for this call and cleared afterwards;
        the cube's double_at and pass_at are ignored, jacoby is refused) -- also mwc [P], mwc_stderr [P] (float64, PLAYER1's
        match-winning chance) and match_counts [P, 3] (int64: trials that ended the match for PLAYER1, for PLAYER2, trials in which a
        decision was withheld by a dead cube), with per_trial trial_mwc [P, T].  The other outputs are the same as without it;
        cubeful, trial_cube and trial_dropped describe in points the records the match rule produced."""
        if match is not None and cube is None:
            raise ValueError("rollout: a match sets the cube's thresholds; pass cube= with match=")
        if cube is not None and not variance_reduction:
            raise ValueError("rollout: the cube decides on the luck pass's pre-roll means; pass variance_reduction=True with cube")
        if groups is not None and int(position_offset) != 0:
            raise ValueError("rollout: groups set the dice ids; pass group_offset, not position_offset")
        if groups is None and int(group_offset) != 0:
            raise ValueError("rollout: group_offset goes with groups; without them pass position_offset")
        if int(plies) != 1:
            _capi.check(self._lib.bgamd_env_rollout_policy(self._h, int(plies), int(top_k), float(margin)), "rollout_policy")
            try:
                return self.rollout(states28, turn, trials, max_plies, rotate, seed, slot, position_offset, lanes, per_trial,
                                    variance_reduction, outcomes, groups=groups, group_offset=group_offset, cube=cube, match=match)
            finally:
                _capi.check(self._lib.bgamd_env_rollout_policy(self._h, 1, 0, 0.0), "rollout_policy")
        st = torch.as_tensor(states28, dtype=torch.int32).to(self.device).contiguous().reshape(-1, 28)
        P, T = st.shape[0], int(trials)
        t = self._dev(turn, torch.int32, (P,))
        if groups is not None:
            grp = torch.as_tensor(groups).to(torch.int64).reshape(-1)
            if grp.shape[0] != P:
                raise ValueError("rollout: groups has %d entries for %d positions" % (grp.shape[0], P))
            if P and (int(grp.min()) < -(2 ** 31) or int(grp.max()) >= 2 ** 31):
                raise ValueError("rollout: a group does not fit in int32")
            grp = grp.to(torch.int32).to(self.device).contiguous()
        out = {"mean": self._buf((P,), torch.float64), "stderr": self._buf((P,), torch.float64),
               "turns": self._buf((P,), torch.int64), "truncated": self._buf((P,), torch.int32)}
        if per_trial:
            out["trial_value"] = self._buf((P, max(T, 0)), torch.float32)
            out["trial_turns"] = self._buf((P, max(T, 0)), torch.int32)
        flags = (ROLLOUT_ROTATE if rotate else 0) | (WEIGHTS_SLOT1 if slot else 0) | (ROLLOUT_VR if variance_reduction else 0)
        if cube is not None:
            c = cube if isinstance(cube, Cube) else Cube(**cube)
            cv = None if c.value is None else self._dev(c.value, torch.int32, (P,))
            co = None if c.owner is None else self._dev(c.owner, torch.int32, (P,))
            _capi.check(self._lib.bgamd_env_rollout_cube(self._h, CUBE_ON | (CUBE_JACOBY if c.jacoby else 0) |
                                                         (CUBE_HOLD_TURN0 if c.hold_turn0 else 0), float(c.double_at),
                                                         float(c.pass_at), float(c.too_good_at), int(c.max_cube), _ptr(cv), _ptr(co)),
                        "rollout_cube")
        try:
            if match is not None:
                a1, a2, ms = (torch.from_numpy(x).to(self.device) for x in match.per_position(P))
                self._set_match(match.table, match.window_share, a1, a2, ms)
            if groups is None:
                _capi.check(self._lib.bgamd_env_rollout(self._h, flags, _ptr(st), _ptr(t), P, int(position_offset), T, int(max_plies),
                                                        int(seed) & (2 ** 64 - 1), int(lanes), _ptr(out["mean"]), _ptr(out["stderr"]),
                                                        _ptr(out["turns"]), _ptr(out["truncated"]), _ptr(out.get("trial_value")),
                                                        _ptr(out.get("trial_turns")), _stream()), "rollout")
            else:
                _capi.check(self._lib.bgamd_env_rollout_grouped(self._h, flags, _ptr(st), _ptr(t), _ptr(grp), P, int(group_offset), T,
                                                                int(max_plies), int(seed) & (2 ** 64 - 1), int(lanes), _ptr(out["mean"]),
                                                                _ptr(out["stderr"]), _ptr(out["turns"]), _ptr(out["truncated"]),
                                                                _ptr(out.get("trial_value")), _ptr(out.get("trial_turns")), _stream()),
                            "rollout_grouped")
        finally:
            if cube is not None:                           # (the setting is sticky in the C ABI; here it lasts for the call, like plies)
                _capi.check(self._lib.bgamd_env_rollout_cube(self._h, 0, 0.0, 0.0, 0.0, 0, None, None), "rollout_cube")
            if match is not None:
                _capi.check(self._lib.bgamd_env_rollout_match(self._h, 0, 0, None, None, 0.0, None, None, None), "rollout_match")
        self._rollout_shape = (P, T)
        if variance_reduction:
            out["vr_mean"], out["vr_stderr"] = self._buf((P,), torch.float64), self._buf((P,), torch.float64)
            if per_trial:
                out["trial_luck"] = self._buf((P, T), torch.float64)
            _capi.check(self._lib.bgamd_env_rollout_vr_read(self._h, _ptr(out["vr_mean"]), _ptr(out["vr_stderr"]),
                                                            _ptr(out.get("trial_luck")), _stream()), "rollout_vr_read")
        if outcomes:
            out.update(self.rollout_outcomes_read(per_trial=per_trial))
        if cube is not None:
            out.update(self.rollout_cube_read(per_trial=per_trial))
        if match is not None:
            out.update(self.rollout_match_read(per_trial=per_trial))
        return out

    def _set_match(self, table, window_share, away1, away2, state):
        """bgamd_env_rollout_match with BGAMD_MATCH_ON: the host tables are copied at the call, the three device tensors are read by the
        next rollout's intake"""
        _capi.check(self._lib.bgamd_env_rollout_match(self._h, MATCH_ON, int(table.M), C.c_void_p(table.met.ctypes.data),
                                                      C.c_void_p(table.met_pc.ctypes.data), float(window_share), _ptr(away1), _ptr(away2),
                                                      _ptr(state)), "rollout_match")

    def rollout_match_read(self, per_trial=False):
        """The last rollout's match results (bgamd_env_rollout_match_results; raises unless that rollout had match=) -> dict: mwc [P],
        mwc_stderr [P], match_counts [P, 3], per_trial: trial_mwc [P, T] -- see rollout(match=)."""
        P, T = self._rollout_shape
        out = {"mwc": self._buf((P,), torch.float64), "mwc_stderr": self._buf((P,), torch.float64),
               "match_counts": self._buf((P, 3), torch.int64)}
        if per_trial:
            out["trial_mwc"] = self._buf((P, T), torch.float64)
        _capi.check(self._lib.bgamd_env_rollout_match_results(self._h, _ptr(out["mwc"]), _ptr(out["mwc_stderr"]), _ptr(out["match_counts"]),
                                                           _ptr(out.get("trial_mwc")), _stream()), "rollout_match_read")
        return out

    def rollout_match_thresholds(self, state, cube, a, b):
        """(double_at, pass_at) of the threshold table of the last match setting, read back from the device
        (bgamd_env_rollout_match_thresholds): state 0 or 2, cube a power of two below the table's size, a the roller's and b the
        opponent's points to go; (inf, inf) where no decision is made."""
        h = (C.c_double * 2)()
        _capi.check(self._lib.bgamd_env_rollout_match_thresholds(self._h, int(state), int(cube), int(a), int(b), h), "rollout_match_thresholds")
        return float(h[0]), float(h[1])

    def rollout_cube_read(self, per_trial=False):
        """The last rollout's cube results (bgamd_env_rollout_cube_read; raises unless that rollout had cube=) -> dict: cubeful [P],
        cubeful_stderr [P], cube_counts [P, 4], per_trial: trial_cubeful, trial_cube, trial_dropped [P, T] -- see rollout(cube=)."""
        P, T = self._rollout_shape
        out = {"cubeful": self._buf((P,), torch.float64), "cubeful_stderr": self._buf((P,), torch.float64),
               "cube_counts": self._buf((P, 4), torch.int64)}
        if per_trial:
            out["trial_cubeful"] = self._buf((P, T), torch.float64)
            out["trial_cube"] = self._buf((P, T), torch.int32)
            out["trial_dropped"] = self._buf((P, T), torch.int32)
        _capi.check(self._lib.bgamd_env_rollout_cube_read(self._h, _ptr(out["cubeful"]), _ptr(out["cubeful_stderr"]),
                                                          _ptr(out["cube_counts"]), _ptr(out.get("trial_cubeful")),
                                                          _ptr(out.get("trial_cube")), _ptr(out.get("trial_dropped")), _stream()),
                    "rollout_cube_read")
        return out

    def rollout_cube_info(self):
        """The last cubeful rollout's [lane-turns played, lane-turns played after the trial's drop] (bgamd_env_rollout_cube_info)."""
        h = (C.c_int64 * 2)()
        _capi.check(self._lib.bgamd_env_rollout_cube_info(self._h, h), "rollout_cube_info")
        return list(h)

    def rollout_outcomes_read(self, per_trial=False):
        """The last rollout's games in points (bgamd_env_rollout_outcomes_read; raises before the first rollout) -> dict: counts [P, 6],
        equity [P], equity_stderr [P], per_trial: trial_points [P, T] -- see rollout(outcomes=True)."""
        P, T = self._rollout_shape
        out = {"counts": self._buf((P, 6), torch.int64), "equity": self._buf((P,), torch.float64),
               "equity_stderr": self._buf((P,), torch.float64)}
        if per_trial:
            out["trial_points"] = self._buf((P, T), torch.int8)
        _capi.check(self._lib.bgamd_env_rollout_outcomes_read(self._h, _ptr(out["counts"]), _ptr(out["equity"]),
                                                              _ptr(out["equity_stderr"]), _ptr(out.get("trial_points")), _stream()),
                    "rollout_outcomes_read")
        return out

    PAIRED_WHICH = {"value": 0, "vr": 1, "equity": 2, "cubeful": 3, "mwc": 4}

    def rollout_paired(self, ref, which="value"):
        """Paired differences of the last rollout (bgamd_env_rollout_paired_read): for each position p and its reference ref[p] (an index
        into that call's positions), mean and standard error of the per-trial differences q_i(p) - q_i(ref[p]) -- q the trial's value
        ("value"), its luck-adjusted value ("vr": the rollout must have had variance_reduction), its equity in points ("equity") or its cubeful equity ("cubeful": the rollout
        must have had cube=) or its match-winning chance ("mwc": the rollout must have had match=).  Only
        positions of one dice group share dice: a reference in another group, or out of range, gives NaN for that p; after a rollout
        without groups every ref[p] != p does.  ref[p] = p gives 0.  -> (diff_mean [P], diff_stderr [P]), float64 device tensors;
        stream-ordered."""
        if which not in self.PAIRED_WHICH:
            raise ValueError("rollout_paired: which is one of 'value', 'vr', 'equity', 'cubeful', 'mwc'")
        P, _ = self._rollout_shape
        r = torch.as_tensor(ref).to(torch.int64).reshape(-1)
        if r.shape[0] != P:
            raise ValueError("rollout_paired: ref has %d entries for %d positions" % (r.shape[0], P))
        r = r.clamp(-1, 2 ** 31 - 1).to(torch.int32).to(self.device).contiguous()          # (anything out of range stays out of range)
        dm, ds = self._buf((P,), torch.float64), self._buf((P,), torch.float64)
        _capi.check(self._lib.bgamd_env_rollout_paired_read(self._h, _ptr(r), self.PAIRED_WHICH[which], _ptr(dm), _ptr(ds), _stream()),
                    "rollout_paired_read")
        return dm, ds

    def rollout_info(self):
        """The last rollout's [lanes, env steps issued, lane-steps of live trials, turns per run]: idle share = 1 - [2] / ([0] [1])."""
        h = (C.c_int64 * 4)()
        _capi.check(self._lib.bgamd_env_rollout_info(self._h, h), "rollout_info")
        return list(h)

    def scratch_info(self):
        """Lanes of the internal envs as they stand (bgamd_env_scratch_info; host values, no launch): [the search's scratch env, the
        rollouts' trial env, the 3-ply step's mid env], 0 where there is none yet."""
        h = (C.c_int64 * 3)()
        _capi.check(self._lib.bgamd_env_scratch_info(self._h, h), "scratch_info")
        return list(h)

    def last_choice(self):
        ch, cnt = self._buf((self.n,), torch.int32), self._buf((self.n,), torch.int32)
        sq, ln = self._buf((self.n, 4, 2), torch.int8), self._buf((self.n,), torch.int32)
        val = self._buf((self.n,), torch.float32)
        _capi.check(self._lib.bgamd_env_last_choice(self._h, _ptr(ch), _ptr(cnt), _ptr(sq), _ptr(ln), _ptr(val), _stream()),
                    "last_choice")
        return {"chosen": ch, "count": cnt, "seq": sq, "seq_len": ln, "value": val}

    def unique_rows_info(self):
        """Diagnostics: (game, key | turn << 31) of every afterstate the value net evaluated in the last greedy step
        -> int64 [U, 2] device tensor (columns game, key)."""
        cap = 1 << 16
        while True:
            buf = self._buf((cap, 2), torch.int32)
            n = _capi.check(self._lib.bgamd_env_unique_rows_info(self._h, _ptr(buf), cap, _stream()), "unique_rows_info")
            if n <= cap:
                torch.cuda.current_stream().synchronize()
                return buf[:n].to(torch.int64) & 0xFFFFFFFF
            cap = int(n)

    def unique_rows(self, want_states=True):
        """Every afterstate the value net evaluated in the last greedy step, in arena order:
        -> (info int64 [U, 2] (game, key | turn << 31), states int32 [U, 28] or None, values float32 [U])."""
        info = self.unique_rows_info()
        u = int(info.shape[0])
        st = self._buf((u, 28), torch.int32) if want_states else None
        val = self._buf((u,), torch.float32)
        _capi.check(self._lib.bgamd_env_unique_rows_read(self._h, 0, u, _ptr(st), _ptr(val), _stream()), "unique_rows_read")
        torch.cuda.current_stream().synchronize()
        return info, st, val

    def choice_spread(self):
        """Do the candidates of the last greedy step still differ?  (include/bgamd.h, bgamd_env_choice_spread: reduced on the device
        over the rows unique_rows() lists.)  -> dict: count int32 [n] rows per lane, best / worst float32 [n] the extreme values from the
        mover's side (0 where count is 0), tied int32 [n] rows bit-equal to best -- device tensors -- and the host numbers choice_lanes
        (count >= 2), all_tied_lanes (of those: tied == count), rows, empty_lanes (count == 0).  Synchronises for the four numbers."""
        cnt, tied = self._buf((self.n,), torch.int32), self._buf((self.n,), torch.int32)
        best, worst = self._buf((self.n,), torch.float32), self._buf((self.n,), torch.float32)
        summ = self._buf((4,), torch.int64)
        _capi.check(self._lib.bgamd_env_choice_spread(self._h, _ptr(cnt), _ptr(best), _ptr(worst), _ptr(tied), _ptr(summ), _stream()),
                    "choice_spread")
        a, b, c, d = (int(x) for x in summ.cpu().tolist())
        return {"count": cnt, "best": best, "worst": worst, "tied": tied, "choice_lanes": a, "all_tied_lanes": b, "rows": c,
                "empty_lanes": d}

    def stats(self):
        out = (C.c_uint64 * 10)()
        _capi.check(self._lib.bgamd_env_stats(self._h, out), "stats")
        k = ("steps", "games_finished", "p1_wins", "candidates_raw", "rows_evaluated", "error_flags",
             "leaf_parent_nodes", "doubles_inner_nodes", "ksteps_executed")
        return dict(zip(k, [int(v) for v in out]))

    def reset_stats(self):
        _capi.check(self._lib.bgamd_env_reset_stats(self._h, _stream()), "reset_stats")

    # -- single-checker surface
    def legal_moves(self, player, die):
        p = self._dev(player, torch.int32, (self.n,))
        d = self._dev(die, torch.int32, (self.n,))
        # (the kernel writes a lane's first n pairs: the slots past them are zero, not whatever the allocator handed out)
        n, pairs = self._buf((self.n,), torch.int32), torch.zeros((self.n, 26, 2), dtype=torch.int8, device=self.device)
        _capi.check(self._lib.bgamd_env_legal_moves(self._h, _ptr(p), _ptr(d), _ptr(n), _ptr(pairs), _stream()), "legal_moves")
        torch.cuda.current_stream().synchronize()
        return n, pairs

    def try_move(self, player, dice, origin, dest):
        args = [self._dev(a, torch.int32, (self.n,)) for a in (player, dice, origin, dest)]
        err = self._buf((self.n,), torch.int32)
        _capi.check(self._lib.bgamd_env_try_move(self._h, *[_ptr(a) for a in args], _ptr(err), _stream()), "try_move")
        torch.cuda.current_stream().synchronize()
        return err

    # -- trajectory log for the learner
    def record_trajectory(self, max_plies: int | None):
        """Allocates (or drops, with None) the per-turn log: int32 tensor [max_plies, n, 8] of 32-byte rows."""
        if max_plies is None:
            self._traj = None
            _capi.check(self._lib.bgamd_env_set_trajectory(self._h, None, 0), "set_trajectory")
            return None
        self._traj = torch.zeros((int(max_plies), self.n, 8), dtype=torch.int32, device=self.device)
        _capi.check(self._lib.bgamd_env_set_trajectory(self._h, _ptr(self._traj), int(max_plies)), "set_trajectory")
        return self._traj

    def record_ring(self, ring_steps: int | None):
        """Ring log of continuous self-play (bgamd_env_set_trajectory_ring): greedy steps with auto_reset log the pre-move row of every
        lane by ENV STEP -> (rows int32 [ring_steps, n, 8], end int16 [ring_steps, n]); end != 0 where the turn logged in that slot was
        the last of its game: (end & 0x7FFF) logged turns, end < 0: PLAYER2 won.  None drops it."""
        if ring_steps is None:
            self._ring = None
            _capi.check(self._lib.bgamd_env_set_trajectory_ring(self._h, None, 0, None), "set_trajectory_ring")
            return None
        rows = torch.zeros((int(ring_steps), self.n, 8), dtype=torch.int32, device=self.device)
        end = torch.zeros((int(ring_steps), self.n), dtype=torch.int16, device=self.device)
        self._ring = (rows, end)
        _capi.check(self._lib.bgamd_env_set_trajectory_ring(self._h, _ptr(rows), int(ring_steps), _ptr(end)), "set_trajectory_ring")
        return rows, end

    def record_search_log(self, max_plies: int | None):
        """Log of the search steps' turns (bgamd_env_set_search_log): while set, every step_search writes, for each lane that takes part,
        at [ply, lane]: the pre-move row, the played afterstate with the opponent to roll, V2 of the played candidate (NaN where the lane
        was not searched: a filtered step's singleton, a lane without a move) and its 1-ply value -> (rows int32 [T, n, 8], after int32
        [T, n, 8], target float32 [T, n], v1 float32 [T, n]); the rows start as zeros, target and v1 as NaN.  While it is set, search steps
        with auto_reset and every other kind of step raise.  None drops it."""
        if max_plies is None:
            self._slog = None
            _capi.check(self._lib.bgamd_env_set_search_log(self._h, None, None, None, None, 0), "set_search_log")
            return None
        T = int(max_plies)
        if T <= 0:                                             # BGAMD_E_INVALID, as the library answers it; nothing is allocated for it
            _capi.check(-1, "set_search_log")
        rows = torch.zeros((T, self.n, 8), dtype=torch.int32, device=self.device)
        after = torch.zeros((T, self.n, 8), dtype=torch.int32, device=self.device)
        target = torch.full((T, self.n), float("nan"), dtype=torch.float32, device=self.device)
        v1 = torch.full((T, self.n), float("nan"), dtype=torch.float32, device=self.device)
        _capi.check(self._lib.bgamd_env_set_search_log(self._h, _ptr(rows), _ptr(after), _ptr(target), _ptr(v1), T), "set_search_log")
        self._slog = (rows, after, target, v1)
        return self._slog

    def trajectory_step(self) -> int:
        """env steps logged into the ring so far (a host counter: no synchronisation)"""
        return int(self._lib.bgamd_env_trajectory_step(self._h))

    def progress(self):
        ply, epi = self._buf((self.n,), torch.int32), self._buf((self.n,), torch.int32)
        _capi.check(self._lib.bgamd_env_get_progress(self._h, _ptr(ply), _ptr(epi), _stream()), "get_progress")
        return ply, epi

    def encode_rows(self, rows):
        """rows: int32 [..., 8] device tensor of 32-byte rows -> float32 [..., 198]."""
        r = rows.contiguous()
        n = r.numel() // 8
        out = self._buf((n, 198), torch.float32)
        _capi.check(self._lib.bgamd_encode_rows(_ptr(r), n, _ptr(out), _stream()), "encode_rows")
        return out.reshape(*rows.shape[:-1], 198)

    # -- stateless operators on caller-provided states
    def encode(self, states28, turn):
        st = torch.as_tensor(states28, dtype=torch.int32).to(self.device).contiguous().reshape(-1, 28)
        n = st.shape[0]
        t = self._dev(turn, torch.int32, (n,))
        out = self._buf((n, 198), torch.float32)
        _capi.check(self._lib.bgamd_encode(_ptr(st), _ptr(t), n, _ptr(out), _stream()), "encode")
        torch.cuda.current_stream().synchronize()
        return out

    def evaluate(self, states28, turn, precision=F32, slot=0):
        st = torch.as_tensor(states28, dtype=torch.int32).to(self.device).contiguous().reshape(-1, 28)
        n = st.shape[0]
        t = self._dev(turn, torch.int32, (n,))
        out = self._buf((n,), torch.float32)
        _capi.check(self._lib.bgamd_evaluate_slot(self._h, int(slot), _ptr(st), _ptr(t), n, int(precision), _ptr(out), _stream()),
                    "evaluate")
        torch.cuda.current_stream().synchronize()
        return out

    def evaluate_incremental(self, root_states28, root_turn, states28, root_index, slot=0):
        """Values of afterstates through the greedy step's incremental fp32 path: root position's hidden layer (dense,
        per root) + the W1 columns of the features afterstate i changes against root root_index[i]."""
        rs = torch.as_tensor(root_states28, dtype=torch.int32).to(self.device).contiguous().reshape(-1, 28)
        nr = rs.shape[0]
        rt = self._dev(root_turn, torch.int32, (nr,))
        st = torch.as_tensor(states28, dtype=torch.int32).to(self.device).contiguous().reshape(-1, 28)
        n = st.shape[0]
        ri = self._dev(root_index, torch.int32, (n,))
        out = self._buf((n,), torch.float32)
        _capi.check(self._lib.bgamd_evaluate_incremental(self._h, int(slot), _ptr(rs), _ptr(rt), nr, _ptr(st), _ptr(ri), n,
                                                         _ptr(out), _stream()), "evaluate_incremental")
        torch.cuda.current_stream().synchronize()
        return out

    # -- kernel timing (bench.py)
    def time_kernels(self, enable=True, groups=None, stride=1):
        """groups: iterable of group names to bracket (default: all): enumerate_ordered, eval, apply, step_random,
        expand, leaves, root (the per-game dense pass of the incremental value net)."""
        names = ("enumerate_ordered", "eval", "apply", "step_random", "expand", "leaves", "root")
        arg = int(bool(enable))
        if enable and (groups is not None or stride > 1):
            arg = (sum(1 << names.index(g) for g in (groups if groups is not None else names)) << 8) | (int(stride) << 20)
        _capi.check(self._lib.bgamd_env_time_kernels(self._h, arg), "time_kernels")

    def kernel_choice(self):
        """What the last greedy step launched (bgamd_env_kernel_choice): names of the value-net kernel and of the root pass, whether the root
        pass ran on the env's second stream, the kernel(s) of the expansion below the roots, and whether the library is the experimental build."""
        out = (C.c_int32 * 4)()
        _capi.check(self._lib.bgamd_env_kernel_choice(self._h, out), "kernel_choice")
        ev = ("eval_rows_delta_kernel", "eval_rows_mdelta_kernel", "eval_rows_f32_kernel", "eval_rows_f16x2_kernel", "eval_rows_d16_kernel",
              "eval_rows_bf16_kernel")
        rt = (None, "root_hidden_resident_kernel", "root_hidden_bf16x3_kernel", "eval_rows_f32_kernel<root>", "inside boundary_kernel<true>")
        return {"eval": ev[out[0]], "root": rt[out[1]], "root_on_second_stream": bool(out[2] & 1),
                "expand": "expand_all_kernel" if out[2] & 2 else "doubles_kernel + expand_kernel<LEAF>", "experimental_build": bool(out[3])}

    def kernel_times(self):
        ms, n = (C.c_double * 8)(), (C.c_uint64 * 8)()
        _capi.check(self._lib.bgamd_env_kernel_times(self._h, ms, n), "kernel_times")
        names = ("enumerate_ordered", "eval", "apply", "step_random", "expand", "leaves", "root")
        return {k: {"ms": ms[i], "launches": int(n[i])} for i, k in enumerate(names)}


_POOL = {}          # device index -> idle one-lane envs (a Game that dies hands its env back)


class Game:
    """The reference `Game` (bindings.cpp:62-93) on a one-lane device env.

    One-lane envs are pooled: constructing a Game (or clone(), which reference-style callers do per candidate) reuses
    an idle env instead of allocating a new one, and the getters read a host mirror that ONE snapshot launch fills after
    each mutation (the reference's getters are plain member reads)."""

    _ARENA = 32768          # > the largest doubles enumeration observed (10 063)

    def __init__(self, player: int = 0):
        global _next_scalar_id
        dev = torch.cuda.current_device() if torch.cuda.is_available() else 0
        pool = _POOL.setdefault(dev, [])
        if pool:
            # a fresh game on a pooled env: the dice a NEW env would roll (seed of set_seed(), game id = the running count),
            # last_dice {1,1} (game.hpp:44), no error flags left over from the previous owner -- issued on the NULL stream,
            # where the host-argument surface (bgamd_game_*) runs: a caller inside `with torch.cuda.stream(s)` must not see
            # the reset overtake the set_state that follows
            self._v = pool.pop()
            self._order()                # ... and not overtake what THIS thread still has queued on its current stream either
            self._v.reseed(_seed, _next_scalar_id, 1 << 40, null_stream=True)
            _capi.check(self._v._lib.bgamd_env_reset_stats(self._v._h, None), "reset_stats")
        else:
            self._v = VecGame(1, device=dev, seed=_seed, lane_offset=_next_scalar_id, lane_stride=1 << 40,
                              arena_rows=self._ARENA)
        _next_scalar_id += 1
        self._players = [None, None]
        self._snap = None
        self._put(None, int(player) % 2)                     # Game::Game(int): turn = parity (game.cpp:44-53)

    def __del__(self):
        v = getattr(self, "_v", None)
        if v is not None and getattr(v, "_h", None) and _POOL is not None:
            self._v = None
            try:                                             # work the dying Game queued on a side stream (make_move's step) must be done
                self._order()                                # before the env's next owner resets it on the NULL stream
            except Exception:
                pass
            pool = _POOL.setdefault(v.device.index or 0, [])
            if len(pool) < 64:
                pool.append(v)
            else:
                v.close()

    def _dirty(self):
        self._snap = None

    @staticmethod
    def _order():
        """The bgamd_game_* calls run on the NULL stream and torch's side streams are non-blocking: work this thread queued
        on its current stream for the same env (step_greedy of make_move, last_choice) has to be done first."""
        st = torch.cuda.current_stream()
        if st != torch.cuda.default_stream(st.device):
            st.synchronize()

    def _s(self):
        """state28 | turn | die1 | die2 | flags: ONE call of the host-argument scalar surface (bgamd_game_snapshot)."""
        if self._snap is None:
            self._order()
            buf = (C.c_int32 * 32)()
            _capi.check(self._v._lib.bgamd_game_snapshot(self._v._h, buf), "snapshot")
            self._snap = list(buf)
        return self._snap

    def _put(self, state28=None, turn=-1):
        arr = (C.c_int32 * 28)(*[int(v) for v in state28]) if state28 is not None else None
        self._order()
        _capi.check(self._v._lib.bgamd_game_set_state(self._v._h, arr, int(turn)), "set_state")
        self._dirty()

    # players ------------------------------------------------------------------------------
    def setPlayers(self, p1: Player, p2: Player):
        self._players = [p1, p2]                              # kept alive here (reference keeps raw pointers)

    def getPlayers(self, num):
        p = self._players[0 if int(num) == 0 else 1]
        return Player(p.getName(), PlayerType(p.getNum()))    # by-value copy, as the binding returns

    # turn / board ---------------------------------------------------------------------------
    def getTurn(self):
        return self._s()[28]

    def setTurn(self, turn):
        self._put(None, int(turn) & 1)

    def _state(self):
        return list(self._s()[:28])

    def getGameBoard(self):
        return self._state()[:24]

    def getPieces(self):
        return Pieces(self)

    def getJailedCount(self, player):
        return self._s()[24 + (0 if int(player) == 0 else 1)]

    def getBornOffCount(self, player):
        return self._s()[26 + (0 if int(player) == 0 else 1)]

    def setGameBoard(self, board):
        board = [int(v) for v in board]
        if len(board) != 24:
            raise ValueError("gameboard must have 24 entries")
        s = self._state()
        self._put(board + s[24:])

    def setBorneOffPieces(self, player, num):
        s = self._state()
        s[26 + (0 if int(player) == 0 else 1)] = int(num)
        self._put(s)

    def _set_jailed(self, player, num):
        """Not in the reference binding (bar counts are only reachable by hits); used by tests/clone."""
        s = self._state()
        s[24 + (0 if int(player) == 0 else 1)] = int(num)
        self._put(s)

    def reset(self):
        self.populateBoard()                                   # binding maps reset -> populateBoard only

    def populateBoard(self):
        s = self._state()
        self._put([2, 0, 0, 0, 0, -5, 0, -3, 0, 0, 0, 5, -5, 0, 0, 0, 3, 0, 5, 0, 0, 0, 0, -2] + s[24:])

    def printGameBoard(self):
        s = self._state()
        print("board", s[:24], "| jail", s[24:26], "| free", s[26:28])

    # dice -------------------------------------------------------------------------------------
    def setDice(self, d1, d2):
        self._order()
        _capi.check(self._v._lib.bgamd_game_set_dice(self._v._h, int(d1), int(d2)), "setDice")
        self._dirty()

    def roll_dice(self):
        d = (C.c_int32 * 2)()
        self._order()
        _capi.check(self._v._lib.bgamd_game_roll(self._v._h, d), "roll_dice")
        self._dirty()
        return [int(d[0]), int(d[1])]

    def get_last_dice(self):
        d = self._s()[29:31]
        return list(d) if d[0] else [1, 1]

    # rules --------------------------------------------------------------------------------------
    def legalMoves(self, player, die):
        pairs = (C.c_int8 * 52)()
        self._order()
        k = _capi.check(self._v._lib.bgamd_game_legal_moves(self._v._h, int(player), int(die), pairs), "legalMoves")
        return [(int(pairs[2 * i]), int(pairs[2 * i + 1])) for i in range(k)]

    def _enumerate(self, player, d1, d2, want_states=True):
        """One call of bgamd_game_enumerate when the list fits the first guess, a second one otherwise."""
        cap = 2048
        for _ in range(2):
            st = np.empty((cap, 28), dtype=np.int32) if want_states else None
            sq, ln = np.empty((cap, 4, 2), dtype=np.int8), np.empty((cap,), dtype=np.int32)
            self._order()
            k = _capi.check(self._v._lib.bgamd_game_enumerate(self._v._h, int(player), int(d1), int(d2),
                                                             st.ctypes.data_as(C.c_void_p) if want_states else None,
                                                             sq.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), cap), "enumerate")
            if k <= cap:
                break
            cap = k
        sql, lnl = sq[:k].tolist(), ln[:k].tolist()
        seqs = [[(sql[i][j][0], sql[i][j][1]) for j in range(lnl[i])] for i in range(k)]
        return seqs, (st[:k].copy() if want_states else None)

    def legalTurnSequences(self, player, die1, die2):
        return self._enumerate(player, die1, die2, want_states=False)[0]

    def evaluateTurnSequences(self, player, die1, die2):
        return self._enumerate(player, die1, die2)

    def tryMove(self, player: Player, dice, origin, dest):
        self._order()
        err = _capi.check(self._v._lib.bgamd_game_try_move(self._v._h, player.getNum(), int(dice), int(origin), int(dest)), "tryMove")
        if err == 0:
            self._dirty()
        return err == 0, ERR_MESSAGES[err]

    def is_game_over(self):
        f = self._s()[31]
        return (True, (f >> 1) & 1) if f & 1 else (False, -1)

    def clone(self):
        g = Game(0)
        g._players = list(self._players)
        s = self._s()
        g._put(s[:28], s[28])                                  # last_dice stays [1,1] (game.cpp:68-77)
        return g
