"""Every device path that embodies the board rules, on the end-game set of tests/endgame_cases.py (exact bear-offs and overruns with the
opponent inside the mover's home board -- where SURVEY Q1 makes the two sides differ --, stragglers that come home and bear off, hits on
the way off, borne-off counts 0..14 and the fifteenth checker leaving mid-turn as a single game, a gammon and a backgammon), every lane.

The expected answers are the UNMODIFIED reference's (fixture G12: ordered sequences, afterstates, legalMoves, is_game_over, every tryMove
probe) wherever it recorded them, and the oracle's -- which tests/test_endgame_cases_cpu.py holds to G12 on every lane -- for what only a
step produces (the turn flip, the restart).  Where a rule is applied to values (the search's selection and choice, the sampled step, the
rollouts) the exact models of tests/search_model.py, tests/sample_model.py, tests/rollout_ref.py and tests/outcome_ref.py speak.  Integer
work is bit-exact; values are within the project's 1e-5 of the fp64 forward pass, under each of the seven parity families of tests/nets.py.

The end record that names a game's winner is the ring log's (record_ring); the per-ply trajectory log has none.  A turn that enters from
the bar and bears off does not exist (tests/endgame_cases.py), so no test asks for one.

Runtime of the whole file on the MI355X: 26 tests in 11.2 s, expected answers included; the slowest (the second step, whose every live
lane is replayed through the oracle and the fp64 forward pass) takes 3.4 s, the next 0.8 s.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import endgame_cases as EC
import nets as N
import outcome_ref as OC
import rollout_ref as R
import rollout_vr_ref as V
import sample_model as SM
import search_model as M
from test_gpu_parity import _check_greedy_step, _np, _replay_key
from test_gpu_rollout_vr import _ties

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BOUND = 1e-5
SEED = 5
START = OC.START


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


class _Set:
    """The set and its expected answers, computed once: G12 per lane (seqs -1 padded as the device pads them), the oracle's answers, the
    distinct afterstates and the census classes of every lane."""

    def __init__(self, golden_dir):
        g = self.g12 = dict(np.load(os.path.join(golden_dir, "g12_endgame_boards.npz")))
        self.st, self.mv, self.dc = g["boards"].astype(np.int32), g["mover"].astype(np.int32), g["dice"].astype(np.int32)
        self.n = len(self.st)
        self.n_seq = g["n_seq"].astype(np.int32)
        self.off = np.concatenate([[0], np.cumsum(self.n_seq)]).astype(np.int64)
        self.total = int(self.off[-1])
        self.states = g["states"].astype(np.int32)
        self.over = g["over"].astype(np.int32)                  # per sequence: -1 nothing borne off, 0 not over, 1 / 2 the winner + 1
        self.seq_len = g["seq_len"].astype(np.int32)
        self.seqs = g["seqs"].astype(np.int8).copy()
        self.seqs[np.arange(4)[None, :] >= self.seq_len[:, None]] = -1
        self.mv_off = np.concatenate([[0], np.cumsum(g["n_moves"].ravel())])
        self.moves = g["moves"]
        self.answers = EC.enumerate_oracle(self.st, self.mv, self.dc)
        self.counts, total, self.classes = EC.census((self.st, self.mv, self.dc), self.answers)
        assert total == self.total and all(v >= EC.MIN_LANES for v in self.counts.values())
        self.distinct = [{tuple(int(v) for v in r) for r in self.lane_states(i)} for i in range(self.n)]
        self.blocked_doubles = np.array([self.n_seq[i] == 1 and self.seq_len[self.off[i]] == 0 for i in range(self.n)])
        self.blocked_plain = self.n_seq == 0
        assert self.blocked_doubles.sum() >= 8 and self.blocked_plain.sum() >= 8
        # the first sequence that ends the game, per lane (-1: none)
        self.first_win = np.array([next((k for k in range(self.n_seq[i]) if self.over[self.off[i] + k] >= 1), -1) for i in range(self.n)])
        self.beside = np.array([any(c.startswith("win_beside_nonwin") for c in cl) for cl in self.classes])

    def lane_states(self, i):
        return self.states[self.off[i]:self.off[i + 1]]

    def g12_moves(self, i, die):
        j = i * 6 + die - 1
        return [(int(o), int(d)) for o, d in self.moves[self.mv_off[j]:self.mv_off[j + 1]]]

    def spread(self, k, classes=EC.CLASSES):
        """k lanes spread over the classes: class by class, the next lane of each that is not taken yet"""
        by_class = {c: [i for i in range(self.n) if c in self.classes[i]] for c in classes}
        taken, depth = [], 0
        while len(taken) < k:
            for c in classes:
                rest = [i for i in by_class[c] if i not in taken]
                if rest and len(taken) < k:
                    taken.append(rest[min(depth, len(rest) - 1)])
            depth += 1
        return np.array(sorted(taken))


@pytest.fixture(scope="module")
def S(golden_dir):
    return _Set(golden_dir)


def _env(bg, S, idx=None, weights=None, seed=SEED):
    idx = np.arange(S.n) if idx is None else np.asarray(idx)
    env = bg.VecGame(len(idx), seed=seed, arena_rows=S.total + 65536)
    if weights is not None:
        env.load_weights(weights)
    env.set_states(S.st[idx], S.mv[idx])
    env.set_dice(S.dc[idx])
    return env


# ---- 1-3: enumeration, legalMoves, tryMove -------------------------------------------------------------------------------------------

def test_enumerate_vs_reference(bg, S):
    """Counts, ordered sequences, lengths and afterstates of every lane against G12, bit for bit; the boards are left as they were."""
    env = _env(bg, S)
    offs, cnts, st, sq, ln = [_np(x) for x in env.enumerate(player=S.mv, dice=S.dc)]
    assert np.array_equal(cnts, S.n_seq) and int(cnts.sum()) == S.total == len(st)
    for i in range(S.n):
        a, b = int(offs[i]), int(offs[i]) + int(cnts[i])
        r = slice(S.off[i], S.off[i + 1])
        assert np.array_equal(st[a:b], S.states[r]), (i, sorted(S.classes[i]))
        assert np.array_equal(ln[a:b], S.seq_len[r]) and np.array_equal(sq[a:b], S.seqs[r]), (i, sorted(S.classes[i]))
    assert np.array_equal(_np(env.states()), S.st) and np.array_equal(_np(env.turns()), S.mv)
    # ... and for the lanes' own turn and dice (no explicit arguments), the same lists
    offs2, cnts2, st2, sq2, ln2 = [_np(x) for x in env.enumerate()]
    assert np.array_equal(cnts2, cnts)
    for i in range(0, S.n, 7):
        a, b = int(offs2[i]), int(offs2[i]) + int(cnts2[i])
        assert np.array_equal(st2[a:b], S.lane_states(i)) and np.array_equal(sq2[a:b], S.seqs[S.off[i]:S.off[i + 1]])
    assert env.stats()["error_flags"] == 0
    env.close()


def test_legal_moves_both_players_six_dice(bg, O, S):
    env = _env(bg, S)
    for die in range(1, 7):
        for who in ("mover", "opponent"):
            pl = S.mv if who == "mover" else 1 - S.mv
            cnt, pairs = [_np(x) for x in env.legal_moves(pl, np.full(S.n, die))]
            for i in range(S.n):
                got = [tuple(x) for x in pairs[i, :cnt[i]].tolist()]
                if who == "mover":
                    assert got == S.g12_moves(i, die) == S.answers[i][2][die - 1], (i, die)
                else:
                    assert got == O.legal_moves(O.State.from28(S.st[i], S.mv[i]), int(pl[i]), die), (i, die, who)
    env.close()


def test_try_move_every_probe(bg, S):
    """Every probe of fixture G12 -- legal bear-offs, overruns the rules deny, the wrong end, a point outside home, the bar, the wrong
    direction, the wrong die, a held point, origins and destinations off the board -- each from the lane's own position: the code names
    the reference's message, an accepted probe leaves the reference's position and a refused one leaves the lane untouched."""
    g = S.g12
    pr, code = g["probes"].astype(np.int32), g["probe_code"].astype(np.int32)
    after = np.repeat(S.st, np.bincount(pr[:, 0], minlength=S.n), axis=0)
    assert np.array_equal(np.repeat(np.arange(S.n), np.bincount(pr[:, 0], minlength=S.n)), pr[:, 0])     # probes are grouped by lane
    after[code == 0] = g["probe_after"]
    assert [bg.ERR_MESSAGES[k] for k in range(8)] == g["messages"].tolist()
    first = np.concatenate([[0], np.cumsum(np.bincount(pr[:, 0], minlength=S.n))])
    per_lane = np.diff(first)
    env = _env(bg, S)
    done = 0
    for r in range(int(per_lane.max())):
        has = per_lane > r
        j = np.where(has, first[:-1] + r, 0)
        # a lane whose probes are used up sends origin -1: refused, untouched
        pl, die = np.where(has, pr[j, 2], S.mv), np.where(has, pr[j, 3], 1)
        org, dst = np.where(has, pr[j, 4], -1), np.where(has, pr[j, 5], 5)
        env.set_states(S.st, S.mv)
        err = _np(env.try_move(pl, die, org, dst))
        got = _np(env.states())
        want_code, want_state = np.where(has, code[j], 1), np.where(has[:, None], after[j], S.st)
        bad = np.nonzero((err != want_code) | (got != want_state).any(1))[0]
        assert len(bad) == 0, [(int(i), EC.PROBE_KINDS[pr[j[i], 1]], pr[j[i]].tolist(), int(err[i]), int(want_code[i])) for i in bad[:5]]
        assert np.array_equal(_np(env.turns()), S.mv)
        done += int(has.sum())
    assert done == len(pr) and env.stats()["error_flags"] == 0
    env.close()


# ---- 4: the random step: the bounded kernels and the whole-tree walk -------------------------------------------------------------------

@pytest.mark.parametrize("auto_reset", [False, True])
def test_random_step_first_last_and_winning_index(bg, O, S, auto_reset):
    """choice_u32 injected so that the first, the last and -- where there is one -- a winning sequence is picked: the afterstate is
    sequence k of G12's list, flags, winner and turn follow the oracle's step; with auto_reset a finished lane holds the start position
    and the opening turn of its next game."""
    picks = {"first": np.zeros(S.n, np.int64), "last": np.maximum(S.n_seq - 1, 0).astype(np.int64),
             "win": np.where(S.first_win >= 0, S.first_win, S.n_seq // 2).astype(np.int64)}
    assert (S.first_win > 0).sum() >= 8                       # a win that is not the first sequence
    for name, k in picks.items():
        u = np.array([EC.u32_for(k[i], S.n_seq[i]) if S.n_seq[i] else 0 for i in range(S.n)], dtype=np.uint32)
        got = {}
        for walk in (False, True):
            env = _env(bg, S)
            env.step_random(roll=False, auto_reset=auto_reset, choice_u32=u, walk=walk)
            lc = env.last_choice()
            got[walk] = dict(states=_np(env.states()), turns=_np(env.turns()), flags=_np(env.flags()),
                             **{key: _np(lc[key]) for key in ("chosen", "count", "seq", "seq_len")})
            st = env.stats()
            assert st["error_flags"] == 0
            env.close()
        a = got[False]
        n_over = n_p1 = 0
        for i in range(S.n):
            where = (name, i, sorted(S.classes[i]))
            s = O.State.from28(S.st[i], S.mv[i])
            o = O.step(s, int(S.dc[i, 0]), int(S.dc[i, 1]), 0, choice_u32=int(u[i]))
            assert a["count"][i] == o.n_candidates == S.n_seq[i] and a["chosen"][i] == o.chosen == (k[i] if S.n_seq[i] else -1), where
            if o.chosen >= 0:
                r = S.off[i] + o.chosen
                assert np.array_equal(s.to28(), S.states[r]) and bool(o.over) == (S.over[r] >= 1), where
                assert not o.over or o.winner == S.over[r] - 1 == S.mv[i], where
                assert a["seq_len"][i] == S.seq_len[r] and np.array_equal(a["seq"][i], S.seqs[r]), where
            assert ((a["flags"][i] >> 4) & 3) == ((1 | (o.winner << 1)) if o.over else 0), where
            n_over += int(o.over); n_p1 += int(o.over and o.winner == 0)
            if o.over and auto_reset:
                assert np.array_equal(a["states"][i], START) and (a["flags"][i] & 7) == 0, where
                assert a["turns"][i] == O.lib().bgo_opening_turn(SEED, i + S.n), where
            else:
                assert np.array_equal(a["states"][i], s.to28()) and a["turns"][i] == s.turn, where
                assert (a["flags"][i] & 7) == ((1 | (o.winner << 1) | 4) if o.over else 0), where
        for key in a:
            assert np.array_equal(a[key], got[True][key]), (name, key)
        assert (st["games_finished"], st["p1_wins"]) == (n_over, n_p1)
        if name == "win":
            assert n_over == (S.first_win >= 0).sum() >= 500 and 0.2 * n_over < n_p1 < 0.8 * n_over
        assert (a["count"][S.blocked_doubles] == 1).all() and (a["chosen"][S.blocked_doubles] == 0).all()
        assert (a["seq_len"][S.blocked_doubles] == 0).all()
        assert (a["count"][S.blocked_plain] == 0).all() and (a["chosen"][S.blocked_plain] == -1).all()
        blocked = S.blocked_doubles | S.blocked_plain
        assert np.array_equal(a["states"][blocked], S.st[blocked]) and (a["turns"][blocked] == 1 - S.mv[blocked]).all()


# ---- 5-9: the greedy step: staged rows, their values, the choice, the end of the game ---------------------------------------------------

def _rows_by_game(env):
    by_game = {}
    for g, k in _np(env.unique_rows_info()):
        by_game.setdefault(int(g), []).append(int(k))
    return by_game


def _check_staged_rows(bg, O, S, weights, idx):
    """The keys handed to the value net, replayed through the oracle, are exactly the distinct afterstates of every lane."""
    env = _env(bg, S, idx, weights)
    env.step_greedy(roll=False, auto_reset=False)
    assert env.stats()["error_flags"] == 0
    by_game = _rows_by_game(env)
    rows = 0
    for j, i in enumerate(idx):
        turn, d1, d2 = int(S.mv[i]), int(S.dc[i, 0]), int(S.dc[i, 1])
        keys = by_game.get(j, [])
        assert all((k >> 31) == turn for k in keys), i
        got = {_replay_key(O, S.st[i], turn, d1, d2, k & 0x7FFFFFFF) for k in keys}
        assert got == S.distinct[i], (i, sorted(S.classes[i]), len(got), len(S.distinct[i]))
        rows += len(keys)
    env.close()
    return rows


def _check_choice(bg, O, S, weights, idx):
    """The applied afterstate is value-optimal for the oracle; with want_index the index is the first occurrence in the ordered list;
    blocked lanes report what the reference's lists say and flip the turn; a lane whose played sequence ends the game says so."""
    env = _env(bg, S, idx, weights)
    env.step_greedy(roll=False, auto_reset=False, want_index=True)
    post, turns, fl = _np(env.states()), _np(env.turns()), _np(env.flags())
    lc = env.last_choice()
    ch, cn, cs, cl = (_np(lc[k]) for k in ("chosen", "count", "seq", "seq_len"))
    assert env.stats()["error_flags"] == 0
    _check_greedy_step(O, weights, S.st[idx], S.mv[idx], S.dc[idx], post, range(len(idx)))
    for j, i in enumerate(idx):
        where = (i, sorted(S.classes[i]))
        assert cn[j] == S.n_seq[i], where
        over = False
        if S.n_seq[i] == 0:
            assert ch[j] == -1 and np.array_equal(post[j], S.st[i]), where
        else:
            states = S.lane_states(i)
            assert 0 <= ch[j] < S.n_seq[i] and np.array_equal(states[ch[j]], post[j]), where     # a row of the list, whatever it is
            assert not (states[:ch[j]] == post[j]).all(1).any(), where            # the first occurrence
            r = S.off[i] + ch[j]
            assert cl[j] == S.seq_len[r] and np.array_equal(cs[j], S.seqs[r]), where
            over = S.over[r] >= 1                                                 # the reference's is_game_over of that sequence
        assert over == bool(post[j, 26] == 15 or post[j, 27] == 15), where
        assert (fl[j] & 1) == over and turns[j] == (S.mv[i] if over else 1 - S.mv[i]), where
    bd, bp = S.blocked_doubles[idx], S.blocked_plain[idx]
    assert (cn[bd] == 1).all() and (ch[bd] == 0).all() and (cl[bd] == 0).all() and (cn[bp] == 0).all() and (ch[bp] == -1).all()
    env.close()
    return post, ch


def test_staged_rows_are_the_distinct_afterstates(bg, O, S, weights):
    rows = _check_staged_rows(bg, O, S, weights, np.arange(S.n))
    distinct = sum(len(d) for d in S.distinct)
    print("staged rows %d for %d distinct afterstates of %d sequences" % (rows, distinct, S.total))
    assert rows < 1.25 * distinct + S.n


@pytest.mark.parametrize("family", N.PARITY)
def test_row_values(bg, O, S, family):
    """Every unique row's value against the fp64 forward pass, at the project's 1e-5 (tests/test_endgame_cases_cpu.py checks the condition
    the bound rests on for these rows).  Rows that end the game go through the net like any other."""
    w = N.table(family)
    env = _env(bg, S, None, w)
    env.step_greedy(roll=False, auto_reset=False, precision=bg.F32)
    info, st, val = [_np(x) for x in env.unique_rows()]
    assert env.stats()["error_flags"] == 0
    game = info[:, 0].astype(np.int64)
    assert len(st) >= sum(len(d) for d in S.distinct)
    for i in range(0, S.n, 3):
        assert {tuple(int(v) for v in s) for s in st[game == i]} == S.distinct[i], (family, i)
    turn = S.mv[game]
    ref = np.empty(len(st), dtype=np.float64)
    for t in (0, 1):
        ref[turn == t] = O.forward_f64(w, O.encode(st[turn == t], t))
    err = np.abs(val.astype(np.float64) - ref)
    worst = float(err.max())
    print("NETS-MAX %-13s %-28s %6d rows: max |gpu - fp64| = %.3g" % (family, "greedy step rows (G12)", len(st), worst))
    k = int(err.argmax())
    assert np.isfinite(val).all() and worst <= BOUND, (family, k, st[k].tolist(), float(val[k]), float(ref[k]))
    assert ((st[:, 26] == 15) | (st[:, 27] == 15)).sum() >= 500
    env.close()


def test_choice_is_value_optimal_and_first_in_order(bg, O, S, weights):
    post, ch = _check_choice(bg, O, S, weights, np.arange(S.n))
    took = np.array([S.over[S.off[i] + ch[i]] >= 1 if S.n_seq[i] else False for i in range(S.n)])
    print("win beside a sequence that does not win: %d lanes, the checkpoint takes the win on %d" % (S.beside.sum(), (took & S.beside).sum()))
    assert S.beside.sum() >= 16
    # strictly the first candidate in reference order under a net that gives every row the same value
    w0 = N.table("zero_w1")
    env = _env(bg, S, None, w0)
    env.step_greedy(roll=False, auto_reset=False, want_index=True)
    post, ch = _np(env.states()), _np(env.last_choice()["chosen"])
    has = S.n_seq > 0
    assert (ch[has] == 0).all() and (ch[~has] == -1).all()
    assert np.array_equal(post[has], S.states[S.off[:-1][has]]) and np.array_equal(post[~has], S.st[~has])
    _check_greedy_step(O, w0, S.st, S.mv, S.dc, post, range(0, S.n, 4), strict=True)
    env.close()


def test_terminal_bookkeeping_after_one_greedy_step(bg, S, weights):
    """After one greedy step from these roots: flags (over, winner, frozen, and the last step's over / winner in bits 4-5), outcomes()
    against outcome_ref.points on every lane, and the counters against the sums over the lanes -- the game is over exactly where the
    reference's is_game_over said so for the played sequence.  With auto_reset the same counters, and the ring log's end record names
    the winner."""
    env = _env(bg, S, None, weights)
    env.step_greedy(roll=False, auto_reset=False, want_index=True)
    post, fl, ch, out = _np(env.states()), _np(env.flags()), _np(env.last_choice()["chosen"]), _np(env.outcomes())
    st = env.stats()
    env.close()
    over = np.array([S.over[S.off[i] + ch[i]] if ch[i] >= 0 else -1 for i in range(S.n)])
    ended, winner = over >= 1, np.where(over >= 1, over - 1, 0)
    assert (winner[ended] == S.mv[ended]).all() and ended.sum() >= 300
    want = np.where(ended, 1 | (winner << 1) | 4 | 16 | (winner << 5), 0)
    assert np.array_equal(fl & 0x37, want), np.nonzero((fl & 0x37) != want)[0][:8]
    pts = OC.points_many(post)
    assert np.array_equal(out, pts) and ((pts != 0) == ended).all() and ((pts > 0) == (ended & (winner == 0))).all()
    assert set(pts.tolist()) == {0, 1, 2, 3, -1, -2, -3}
    assert (st["games_finished"], st["p1_wins"], st["error_flags"]) == (int(ended.sum()), int((ended & (winner == 0)).sum()), 0)
    # the same step with auto_reset: the counters, the end records, and the lanes that ended stand on their next game
    env = _env(bg, S, None, weights)
    rows, end = env.record_ring(1)
    env.step_greedy(roll=False, auto_reset=True)
    post2, fl2, out2, st2 = _np(env.states()), _np(env.flags()), _np(env.outcomes()), env.stats()
    end = _np(end)[0].astype(np.int64) & 0xFFFF
    assert torch.equal(rows[0], bg.pack_rows(S.st, S.mv))
    env.record_ring(None)
    env.close()
    assert (st2["games_finished"], st2["p1_wins"], st2["error_flags"]) == (st["games_finished"], st["p1_wins"], 0)
    assert np.array_equal(end != 0, ended) and np.array_equal((end >> 15)[ended], winner[ended])
    assert np.array_equal(post2[~ended], post[~ended]) and (post2[ended] == START).all()
    assert np.array_equal(fl2 & 0x37, np.where(ended, 16 | (winner << 5), 0))
    assert not out2.any()                                                         # still playing, or on the next game: no points


def test_second_step_from_the_roots_the_first_wrote(bg, O, S, weights):
    """Two steps on the lanes' dice: run_greedy(2) equals two step_greedy, the lanes that ended stay as they are, and the second step --
    the other side moves, from a root the first step's apply wrote -- is again value-optimal for the oracle on every lane."""
    a, b = _env(bg, S, None, weights), _env(bg, S, None, weights)
    a.step_greedy(roll=False, auto_reset=False)
    pre, pt, fl = _np(a.states()), _np(a.turns()), _np(a.flags())
    a.step_greedy(roll=False, auto_reset=False)
    b.run_greedy(2, roll=False, auto_reset=False)
    post = _np(a.states())
    assert np.array_equal(post, _np(b.states())) and np.array_equal(_np(a.turns()), _np(b.turns()))
    assert np.array_equal(_np(a.flags()), _np(b.flags()))
    live = (fl & 4) == 0
    assert 300 <= (~live).sum() and live.sum() > 0.5 * S.n and np.array_equal(post[~live], pre[~live])
    assert (pt[live] == 1 - S.mv[live]).all() and (pt[~live] == S.mv[~live]).all()
    _check_greedy_step(O, weights, pre, pt, S.dc, post, [i for i in range(S.n) if live[i]])
    over = (post[:, 26] == 15) | (post[:, 27] == 15)
    assert (over & live).sum() >= 8                                               # games the second mover ends
    assert (_np(a.turns())[live & ~over] == S.mv[live & ~over]).all()
    assert np.array_equal(_np(a.outcomes()), OC.points_many(post))
    assert a.stats()["error_flags"] == 0 and b.stats()["error_flags"] == 0
    a.close(); b.close()


# ---- 10-12: the search's candidates, the pre-roll evaluation, the sampled step ------------------------------------------------------------

_full = {}            # lane -> {reference-order index: (v1, v2)} of the full-width search, for the top_k = 3 run that follows it


@pytest.mark.parametrize("top_k", [0, 3])
def test_search_candidates(bg, O, S, weights, top_k):
    """The 2-ply search on these roots against tests/search_model.py fed with the device's own values: the kept candidates are distinct
    afterstates of the lane in select()'s order (all of them at top_k = 0), a candidate that ends the game has exactly its outcome as v1
    and V2, any other has the fp64 forward pass as v1 (1e-5) and v2_from_replies() of evaluate_preroll's reply values as V2 (bit for
    bit), and the played candidate is choose() of the device's V2."""
    env = _env(bg, S, None, weights)
    env.step_search(top_k=top_k, roll=False, auto_reset=False, no_flip=True)
    states, v1, v2, kept = (_np(x) for x in env.search_candidates())
    after, lc = _np(env.states()), {k: _np(v) for k, v in env.last_choice().items()}
    assert env.stats()["error_flags"] == 0
    env.close()
    worst, n_term = 0.0, 0
    cmp_rows, cmp_mover, cmp_v2 = [], [], []
    for i in range(S.n):
        k, mover = int(kept[i]), int(S.mv[i])
        where = (top_k, i, sorted(S.classes[i]))
        # reference-order index of every distinct afterstate: its first occurrence in G12's list
        index = {}
        for j, r in enumerate(S.lane_states(i)):
            index.setdefault(r.tobytes(), j)
        m = len(index)
        assert k == (min(top_k, m) if top_k else m), where
        if k == 0:
            assert np.array_equal(after[i], S.st[i]), where
            continue
        idx = np.array([index[np.ascontiguousarray(s, dtype=np.int32).tobytes()] for s in states[i, :k]], np.int64)
        assert len(set(idx.tolist())) == k, where
        if top_k == 0:
            assert np.array_equal(idx, M.select(idx, v1[i, :k], mover, 0)), where
            _full[i] = dict(zip(idx.tolist(), zip(v1[i, :k].copy(), v2[i, :k].copy())))
        elif i in _full:                                                          # the cut: the first top_k of the full order, same values
            all_idx = np.array(sorted(_full[i]), np.int64)
            all_v1 = np.array([_full[i][j][0] for j in all_idx], np.float32)
            assert np.array_equal(idx, M.select(all_idx, all_v1, mover, top_k)), where
            assert np.array_equal(_u32(v1[i, :k]), _u32(np.array([_full[i][j][0] for j in idx], np.float32))), where
            assert np.array_equal(_u32(v2[i, :k]), _u32(np.array([_full[i][j][1] for j in idx], np.float32))), where
        term = states[i, :k, 26 + mover] == 15
        outcome = np.float32(1.0 if mover == 0 else 0.0)
        assert (_u32(v1[i, :k][term]) == _u32(outcome)).all() and (_u32(v2[i, :k][term]) == _u32(outcome)).all(), where
        assert np.array_equal(term, np.array([S.over[S.off[i] + j] >= 1 for j in idx])), where
        n_term += int(term.sum())
        if (~term).any():
            ref = O.forward_f64(weights, O.encode(states[i, :k][~term], mover))
            worst = max(worst, float(np.abs(v1[i, :k][~term] - ref).max()))
            if k >= 2:                                                            # (a lane that keeps one candidate plays it unsearched)
                cmp_rows.append(states[i, :k][~term]); cmp_mover.append(np.full(int((~term).sum()), mover)); cmp_v2.append(v2[i, :k][~term])
        j = M.choose(idx, v2[i, :k], mover)
        assert np.array_equal(after[i], states[i, j]) and _u32(lc["value"][i]) == _u32(v2[i, j]), where
    print("NETS-MAX %-13s %-28s max |gpu - fp64| = %.3g" % ("ckpt", "search v1 (G12, top_k %d)" % top_k, worst))
    assert worst <= BOUND and n_term >= (500 if top_k == 0 else 300)
    cand, mover, got = np.concatenate(cmp_rows), np.concatenate(cmp_mover), np.concatenate(cmp_v2)
    pre = bg.VecGame(64)
    pre.load_weights(weights)
    f, _ = (_np(x) for x in pre.evaluate_preroll(cand, 1 - mover))
    assert pre.stats()["error_flags"] == 0
    pre.close()
    bad = np.nonzero(_u32(got) != _u32(M.v2_from_replies(f)))[0]
    assert len(bad) == 0, (len(bad), cand[bad[:2]].tolist(), got[bad[:4]].tolist())


def test_preroll_from_overrun_roots(bg, S, weights):
    """All 21 rolls from 128 roots that hold every overrun class against the fp64 reference, at the bound and with the tie rule of
    test_gpu_nets.test_preroll."""
    overrun = [c for c in EC.CLASSES if c.startswith(("exact", "overrun", "must_move_inside", "home_blocked"))]
    idx = S.spread(128, overrun)
    assert all(any(c in S.classes[i] for i in idx) for c in overrun) and len(overrun) >= 13
    ps, pt = S.st[idx], S.mv[idx]
    env = bg.VecGame(64)
    env.load_weights(weights)
    f, m = (_np(x) for x in env.evaluate_preroll(ps, pt))
    n_cmp, worst = 0, 0.0
    for q in range(len(ps)):
        rf, rm = V.preroll(weights, ps[q], int(pt[q]))
        ok = ~_ties(weights, ps[q], int(pt[q]))
        n_cmp += int(ok.sum())
        worst = max(worst, float(np.abs(f[q] - rf)[ok].max()) if ok.any() else 0.0)
        np.testing.assert_allclose(f[q][ok], rf[ok], atol=BOUND, rtol=0, err_msg="lane %d" % idx[q])
        if ok.all():
            assert abs(m[q] - rm) < BOUND
    print("NETS-MAX %-13s %-28s %6d rolls: max |gpu - fp64| = %.3g" % ("ckpt", "evaluate_preroll (G12)", n_cmp, worst))
    assert n_cmp >= 0.9 * 21 * len(ps)
    assert env.stats()["error_flags"] == 0
    env.close()


def test_sampled_step_lane_by_lane(bg, S, weights):
    """step_sampled at T = 0.05 against tests/sample_model.py fed with the device's own rows and values: the rows are the lane's distinct
    afterstates, and outside the near ties (at most 1 % of the lanes) the played board and value are the model's winner."""
    T = 0.05
    env = _env(bg, S, None, weights, seed=SM.SEED)
    env.step_sampled(T, roll=False, auto_reset=False, no_flip=True)
    info, ust, uval = (_np(x) for x in env.unique_rows())
    post, lc = _np(env.states()), {k: _np(v) for k, v in env.last_choice().items()}
    fl = _np(env.flags())
    assert env.stats()["error_flags"] == 0
    env.close()
    ust = np.ascontiguousarray(ust, dtype=np.int32)
    game, key = info[:, 0], info[:, 1] & 0x7FFFFFFF
    assert ((info[:, 1] >> 31) == S.mv[game]).all()
    order = np.argsort(game, kind="stable")
    bounds = np.searchsorted(game[order], np.arange(S.n + 1))
    planes = SM.planes(ust)
    left_out = moved = other = 0
    for i in range(S.n):
        idx = order[bounds[i]:bounds[i + 1]]
        where = (i, sorted(S.classes[i]))
        if len(idx) == 0:
            assert S.n_seq[i] == 0 and np.array_equal(post[i], S.st[i]) and lc["chosen"][i] == -1, where
            continue
        assert {tuple(int(v) for v in s) for s in ust[idx]} == S.distinct[i], where
        m = SM.lane(planes[idx], key[idx], uval[idx], S.mv[i], SM.SEED, i, 0, T)
        moved += 1
        over = bool(post[i, 26 + S.mv[i]] == 15)
        assert (fl[i] & 1) == over, where
        if m["near"]:
            left_out += 1
            continue
        w = idx[m["winner"]]
        assert np.array_equal(post[i], ust[w]) and _u32(lc["value"][i]) == _u32(uval[w]), where
        a = SM.mover_side(uval[idx], S.mv[i])
        other += int(_u32(uval[w]).item() != _u32(uval[idx][np.argmax(a)]).item())
    print("sampled step, T %g: lanes with a move %d, near ties left out %d, lanes that left the arg-max %d" % (T, moved, left_out, other))
    assert left_out <= 0.01 * S.n and moved == (S.n_seq > 0).sum() and other >= 8


# ---- 13: rollouts played out ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rotate", [True, False])
def test_rollouts_played_out(bg, S, weights, rotate):
    """36 trials to the end of the game from 24 positions of the set: turns, value, points and the six counts of every trial against
    rollout_ref / outcome_ref, outside the near ties (tests/test_endgame_cases_cpu.py: under 1 % of the trials)."""
    lanes = EC.rollout_lanes((S.st, S.mv, S.dc), S.classes)
    st, tu, T = S.st[lanes], S.mv[lanes], EC.ROLLOUT_TRIALS
    env = bg.VecGame(64, seed=7)
    env.load_weights(weights)
    r = {k: _np(v) for k, v in env.rollout(st, tu, T, max_plies=0, rotate=rotate, seed=EC.SEED, per_trial=True, outcomes=True).items()}
    assert env.stats()["error_flags"] == 0
    env.close()
    P = len(lanes)
    val, turns, pts, near = np.zeros((P, T)), np.zeros((P, T), np.int64), np.zeros((P, T), np.int64), np.zeros((P, T), bool)
    for p in range(P):
        for t in range(T):
            val[p, t], turns[p, t], trunc, near[p, t], board = OC.trial_with_board(weights, st[p], int(tu[p]), EC.SEED, p * T + t, t, 0, rotate)
            pts[p, t] = OC.points(board)
            assert not trunc
    cmp = ~near
    assert R.TIE_EPS == 2e-5 and near.mean() < 0.01, near.mean()
    np.testing.assert_array_equal(r["trial_turns"][cmp], turns[cmp])
    np.testing.assert_array_equal(r["trial_value"][cmp], val[cmp].astype(np.float32))
    np.testing.assert_array_equal(r["trial_points"][cmp], pts[cmp])
    assert set(pts[cmp].tolist()) == {1, 2, 3, -1, -2, -3} and (r["truncated"] == 0).all()
    clean = cmp.all(1)
    want = np.stack([(pts == c).sum(1) for c in (1, 2, 3, -1, -2, -3)], axis=1)
    assert clean.sum() >= 16 and np.array_equal(r["counts"][clean], want[clean])
    assert np.array_equal(r["counts"].sum(1), np.full(P, T))


# ---- 14-15: other launch shapes, the scalar surface ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 65])
def test_small_lane_counts(bg, O, S, weights, n):
    """The staged-rows and choice checks on envs of 1 and 65 lanes that hold a win, a denied overrun and a home-blocked lane: other
    launch shapes, the same rules."""
    need = ("win_P1", "win_P2", "overrun_denied_oppbehind_P2", "overrun_denied_own_higher_P1", "home_blocked_P1", "home_blocked_P2")
    if n == 1:
        lanes = [next(i for i in range(S.n) if c in S.classes[i]) for c in need]
        for i in lanes:
            _check_staged_rows(bg, O, S, weights, np.array([i]))
            _check_choice(bg, O, S, weights, np.array([i]))
    else:
        idx = S.spread(65)
        assert all(any(c in S.classes[i] for i in idx) for c in need)
        _check_staged_rows(bg, O, S, weights, idx)
        _check_choice(bg, O, S, weights, idx)


def test_scalar_surface(bg, S):
    """64 lanes through the package's Game: setGameBoard / setBorneOffPieces, evaluateTurnSequences, legalMoves, tryMove (three of the
    lane's probes, and sequences that bear off played move by move), is_game_over -- against G12."""
    lanes = EC.scalar_lanes(S.st)
    cls = set().union(*(S.classes[i] for i in lanes))
    assert {"win_P1", "win_P2", "overrun_denied_oppbehind_P2", "overrun_ok_oppbehind_P1"} <= cls, sorted(cls)
    played, ended = EC.scalar_surface_check(bg, S.g12, lanes)
    print("scalar surface: %d sequences played through tryMove, %d of them end the game" % (played, ended))
    assert played >= 64 and ended >= 8


def test_scalar_surface_compiled_module(S):
    """The same 64 lanes through the compiled pybind11 module, in a process of its own (tests/pybind_driver.py)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pybind_driver.py"), "endgame"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    tag, played, ended = r.stdout.split()[-3:]
    assert tag == "OK" and int(played) >= 64 and int(ended) >= 8
