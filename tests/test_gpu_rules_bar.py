"""Every device path that embodies the board rules, on the bar-heavy set of tests/rule_cases.py (both bars 0..15, three and four entries on
doubles, entries that leave the bar occupied, hits and entries that carry a bar count across 3|4 and 7|8), every lane.

The expected answers are the UNMODIFIED reference's (fixture G11: ordered sequences, afterstates, legalMoves) wherever it recorded them,
and the oracle's -- which tests/test_rule_cases_cpu.py holds to G11 on every lane -- for what only a step produces (tryMove's messages,
the random and the greedy choice, flags, the turn flip).  Integer work is bit-exact; values are within the project's 1e-5 of the fp64
forward pass, under each of the seven parity families of tests/nets.py.

Runtime of the whole file on the MI355X: 19 tests in 5.4 s, expected answers included; the slowest takes 0.7 s.
"""
import ctypes as C
import os

import numpy as np
import pytest

import nets as N
import rollout_vr_ref as V
import rule_cases as RC
from test_gpu_parity import _check_greedy_step, _np, _replay_key
from test_gpu_rollout_vr import _ties

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BOUND = 1e-5


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


class _Set:
    """The set and its expected answers, computed once: G11 per lane (seqs -1 padded as the device pads them), the oracle's answers, the
    distinct afterstates and the census classes of every lane."""

    def __init__(self, golden_dir):
        g = np.load(os.path.join(golden_dir, "g11_bar_boards.npz"))
        self.st, self.mv, self.dc = g["boards"].astype(np.int32), g["mover"].astype(np.int32), g["dice"].astype(np.int32)
        self.n = len(self.st)
        self.n_seq = g["n_seq"].astype(np.int32)
        self.off = np.concatenate([[0], np.cumsum(self.n_seq)]).astype(np.int64)
        self.total = int(self.off[-1])
        self.states = g["states"].astype(np.int32)
        self.seq_len = g["seq_len"].astype(np.int32)
        self.seqs = g["seqs"].astype(np.int8).copy()
        self.seqs[np.arange(4)[None, :] >= self.seq_len[:, None]] = -1
        self.n_moves = g["n_moves"]
        self.mv_off = np.concatenate([[0], np.cumsum(g["n_moves"].ravel())])
        self.moves = g["moves"]
        self.answers = RC.enumerate_oracle(self.st, self.mv, self.dc)
        self.counts, total, self.classes = RC.census((self.st, self.mv, self.dc), self.answers)
        assert total == self.total and all(v >= RC.MIN_LANES for v in self.counts.values())
        self.distinct = [{tuple(int(v) for v in r) for r in self.lane_states(i)} for i in range(self.n)]
        self.blocked_doubles = np.array([self.n_seq[i] == 1 and self.seq_len[self.off[i]] == 0 for i in range(self.n)])
        self.blocked_plain = self.n_seq == 0
        assert self.blocked_doubles.sum() >= 8 and self.blocked_plain.sum() >= 8

    def lane_states(self, i):
        return self.states[self.off[i]:self.off[i + 1]]

    def g11_moves(self, i, die):
        j = i * 6 + die - 1
        return [(int(o), int(d)) for o, d in self.moves[self.mv_off[j]:self.mv_off[j + 1]]]

    def spread(self, k):
        """k lanes spread over the census classes: class by class, the next lane of each that is not taken yet"""
        by_class = {c: [i for i in range(self.n) if c in self.classes[i]] for c in RC.CLASSES}
        taken, depth = [], 0
        while len(taken) < k:
            for c in RC.CLASSES:
                rest = [i for i in by_class[c] if i not in taken]
                if rest and len(taken) < k:
                    taken.append(rest[min(depth, len(rest) - 1)])
            depth += 1
        return np.array(sorted(taken))


@pytest.fixture(scope="module")
def S(golden_dir):
    return _Set(golden_dir)


def _env(bg, S, idx=None, weights=None):
    idx = np.arange(S.n) if idx is None else np.asarray(idx)
    env = bg.VecGame(len(idx), seed=5, arena_rows=S.total + 65536)
    if weights is not None:
        env.load_weights(weights)
    env.set_states(S.st[idx], S.mv[idx])
    env.set_dice(S.dc[idx])
    return env


# ---- enumeration, legalMoves, tryMove ----------------------------------------------------------------------------------------------

def test_enumerate_vs_reference(bg, S):
    """Counts, ordered sequences, lengths and afterstates of every lane against G11, bit for bit; the boards are left as they were."""
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
                    assert got == S.g11_moves(i, die) == S.answers[i][2][die - 1], (i, die)
                else:
                    assert got == O.legal_moves(O.State.from28(S.st[i], S.mv[i]), int(pl[i]), die), (i, die, who)
    env.close()


def test_try_move_entries_and_refusals(bg, O, S):
    """Per lane: one legal entry, one move from a point while the bar is occupied, one blocked entry, one arbitrary probe -- tryMove's
    message and the state it leaves against the oracle."""
    env = _env(bg, S)
    rng = np.random.RandomState(12)
    sign = np.where(S.mv == 0, 1, -1)
    bar_o = np.where(S.mv == 0, 0, 25)
    b = S.st[np.arange(S.n), 24 + S.mv]
    probes = {}
    # a legal entry (a lane without one: its first legal move of any die, or the bar origin with die 1)
    pl, die, org, dst = S.mv.copy(), np.ones(S.n, np.int32), bar_o.copy(), bar_o + sign
    for i in range(S.n):
        for d in rng.permutation(6) + 1:
            if S.answers[i][2][d - 1]:
                die[i] = d
                org[i], dst[i] = S.answers[i][2][d - 1][0]
                break
    probes["entry"] = (pl, die, org, dst)
    # a move from a point of the mover's while the bar is occupied
    org2 = np.array([next((p + 1 for p in rng.permutation(24) if S.st[i, p] * sign[i] > 0), 12) for i in range(S.n)], dtype=np.int32)
    die2 = S.dc[:, 0].copy()
    probes["point"] = (S.mv.copy(), die2, org2, np.clip(org2 + sign * die2, 1, 24))
    # an entry onto a point the opponent holds (a lane without one: the die of its roll)
    die3 = S.dc[:, 1].copy()
    for i in range(S.n):
        held = [d for d in range(1, 7) if S.st[i, (d if S.mv[i] == 0 else 25 - d) - 1] * sign[i] <= -2]
        if held:
            die3[i] = held[rng.randint(len(held))]
    probes["blocked"] = (S.mv.copy(), die3, bar_o.copy(), bar_o + sign * die3)
    probes["arbitrary"] = (rng.randint(0, 2, S.n), rng.randint(1, 7, S.n), rng.randint(-1, 27, S.n), rng.randint(-1, 27, S.n))
    seen = {}
    for name, (pl, die, org, dst) in probes.items():
        env.set_states(S.st, S.mv)
        err = _np(env.try_move(pl, die, org, dst))
        after = _np(env.states())
        msgs = []
        for i in range(S.n):
            s = O.State.from28(S.st[i], S.mv[i])
            ok, msg = O.try_move(s, int(pl[i]), int(die[i]), int(org[i]), int(dst[i]))
            assert bg.ERR_MESSAGES[int(err[i])] == msg, (name, i, int(err[i]), msg)
            assert np.array_equal(after[i], s.to28()), (name, i)
            msgs.append(msg)
        seen[name] = np.array(msgs)
    from_bar = (probes["entry"][2] == bar_o) & (b > 0)
    assert ((seen["entry"] == "") & from_bar).sum() > 1000                       # entries that were made, bar counts 1..15
    assert ((seen["entry"] == "") & from_bar & (b >= 4)).sum() > 300
    assert ((seen["point"] == "Invalid origin") & (b > 0)).sum() > 1000          # the bar comes first
    assert ((seen["blocked"] == "Invalid destination.") & (b > 0)).sum() > 300
    assert len(set(seen["arbitrary"].tolist())) >= 5
    env.close()


# ---- the random step: the bounded kernels and the whole-tree walk ---------------------------------------------------------------------

def test_random_step_bounded_and_walk(bg, O, S):
    u = np.random.RandomState(13).randint(0, 2 ** 32, S.n, dtype=np.uint64).astype(np.uint32)
    got = {}
    for walk in (False, True):
        env = _env(bg, S)
        env.step_random(roll=False, auto_reset=False, choice_u32=u, walk=walk)
        lc = env.last_choice()
        got[walk] = dict(states=_np(env.states()), turns=_np(env.turns()), flags=_np(env.flags()),
                         **{k: _np(lc[k]) for k in ("chosen", "count", "seq", "seq_len")})
        assert env.stats()["error_flags"] == 0
        env.close()
    a = got[False]
    for i in range(S.n):
        s = O.State.from28(S.st[i], S.mv[i])
        o = O.step(s, int(S.dc[i, 0]), int(S.dc[i, 1]), 0, choice_u32=int(u[i]))
        where = (i, sorted(S.classes[i]))
        assert a["count"][i] == o.n_candidates == S.n_seq[i] and a["chosen"][i] == o.chosen, where
        assert np.array_equal(a["states"][i], s.to28()) and a["turns"][i] == s.turn, where
        assert ((a["flags"][i] >> 4) & 3) == (o.over | (o.winner << 1) if o.over else 0) and (a["flags"][i] & 1) == o.over, where
        if o.chosen >= 0:
            r = S.off[i] + o.chosen
            assert a["seq_len"][i] == S.seq_len[r] and np.array_equal(a["seq"][i], S.seqs[r]), where
            assert np.array_equal(a["states"][i], S.states[r]), where
    for k in a:
        assert np.array_equal(a[k], got[True][k]), k
    live = (a["flags"] & 1) == 0
    assert (a["turns"] != S.mv)[live].all()                                      # blocked lanes flip the turn as well
    assert (a["count"][S.blocked_doubles] == 1).all() and (a["chosen"][S.blocked_doubles] == 0).all()
    assert (a["seq_len"][S.blocked_doubles] == 0).all()
    assert (a["count"][S.blocked_plain] == 0).all() and (a["chosen"][S.blocked_plain] == -1).all()
    assert np.array_equal(a["states"][S.blocked_doubles | S.blocked_plain], S.st[S.blocked_doubles | S.blocked_plain])


# ---- the greedy step: staged rows, their values, the choice ---------------------------------------------------------------------------

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
    blocked lanes report what the reference's lists say and flip the turn."""
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
        if S.n_seq[i] == 0:
            assert ch[j] == -1 and np.array_equal(post[j], S.st[i]), where
        else:
            states = S.lane_states(i)
            assert 0 <= ch[j] < S.n_seq[i] and np.array_equal(states[ch[j]], post[j]), where
            assert not (states[:ch[j]] == post[j]).all(1).any(), where            # the first occurrence
            r = S.off[i] + ch[j]
            assert cl[j] == S.seq_len[r] and np.array_equal(cs[j], S.seqs[r]), where
        over = bool(post[j, 26] == 15 or post[j, 27] == 15)
        assert (fl[j] & 1) == over and turns[j] == (S.mv[i] if over else 1 - S.mv[i]), where
    bd, bp = S.blocked_doubles[idx], S.blocked_plain[idx]
    assert (cn[bd] == 1).all() and (ch[bd] == 0).all() and (cl[bd] == 0).all() and (cn[bp] == 0).all() and (ch[bp] == -1).all()
    env.close()


def test_staged_rows_are_the_distinct_afterstates(bg, O, S, weights):
    rows = _check_staged_rows(bg, O, S, weights, np.arange(S.n))
    distinct = sum(len(d) for d in S.distinct)
    print("staged rows %d for %d distinct afterstates of %d sequences" % (rows, distinct, S.total))
    assert rows < 1.25 * distinct + S.n


@pytest.mark.parametrize("family", N.PARITY)
def test_row_values(bg, O, S, family):
    """Every unique row's value against the fp64 forward pass, at the project's 1e-5 (tests/test_rule_cases_cpu.py checks the condition
    the bound rests on for these rows)."""
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
    print("NETS-MAX %-13s %-28s %6d rows: max |gpu - fp64| = %.3g" % (family, "greedy step rows (G11)", len(st), worst))
    k = int(err.argmax())
    assert np.isfinite(val).all() and worst <= BOUND, (family, k, st[k].tolist(), float(val[k]), float(ref[k]))
    env.close()


def test_choice_is_value_optimal_and_first_in_order(bg, O, S, weights):
    _check_choice(bg, O, S, weights, np.arange(S.n))
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


def test_second_step_from_bar_heavy_roots(bg, O, S, weights):
    """Two steps on the lanes' dice: run_greedy(2) equals two step_greedy, and the second step -- the side with the other bar moves, from a
    root the first step's apply wrote -- is again value-optimal for the oracle on every lane."""
    a, b = _env(bg, S, None, weights), _env(bg, S, None, weights)
    a.step_greedy(roll=False, auto_reset=False)
    pre, pt, fl = _np(a.states()), _np(a.turns()), _np(a.flags())
    a.step_greedy(roll=False, auto_reset=False)
    b.run_greedy(2, roll=False, auto_reset=False)
    post = _np(a.states())
    assert np.array_equal(post, _np(b.states())) and np.array_equal(_np(a.turns()), _np(b.turns()))
    assert np.array_equal(_np(a.flags()), _np(b.flags()))
    live = (fl & 4) == 0
    assert live.sum() > 0.9 * S.n and np.array_equal(post[~live], pre[~live])
    assert (pt[live] == 1 - S.mv[live]).all()
    heavy = pre[np.arange(S.n), 24 + pt] >= 3
    assert (heavy & live).sum() > 500                                             # the second mover's bar is heavy too
    _check_greedy_step(O, weights, pre, pt, S.dc, post, [i for i in range(S.n) if live[i]])
    over = (post[:, 26] == 15) | (post[:, 27] == 15)
    assert (_np(a.turns())[live & ~over] == S.mv[live & ~over]).all()
    assert a.stats()["error_flags"] == 0 and b.stats()["error_flags"] == 0
    a.close(); b.close()


def test_search_candidates(bg, O, S, weights):
    """The 2-ply search keeping every candidate: `kept` and the candidate states are exactly the distinct afterstates of every lane (a
    blocked lane keeps none, or one on doubles); v1 is the fp64 forward pass (the outcome for a candidate that ends the game)."""
    env = _env(bg, S, None, weights)
    env.step_search(top_k=0, margin=float("inf"), roll=False, auto_reset=False)
    states, v1, v2, kept = (_np(x) for x in env.search_candidates())
    assert env.stats()["error_flags"] == 0
    worst = 0.0
    for i in range(S.n):
        k, turn = int(kept[i]), int(S.mv[i])
        where = (i, sorted(S.classes[i]))
        assert k == len(S.distinct[i]), where
        assert {tuple(int(v) for v in s) for s in states[i, :k]} == S.distinct[i], where
        if k == 0:
            continue
        ref = O.forward_f64(weights, O.encode(states[i, :k], turn))
        for j in range(k):
            if states[i, j, 26 + turn] == 15:
                assert v1[i, j] == (1.0 if turn == 0 else 0.0), where
            else:
                worst = max(worst, abs(float(v1[i, j]) - float(ref[j])))
    print("NETS-MAX %-13s %-28s max |gpu - fp64| = %.3g" % ("ckpt", "search v1 (G11)", worst))
    assert worst <= BOUND
    assert (kept[S.blocked_plain] == 0).all() and (kept[S.blocked_doubles] == 1).all()
    env.close()


def test_preroll_from_bar_heavy_roots(bg, S, weights):
    """All 21 rolls from 128 roots spread over the classes (many of the rolls are passes) against the fp64 reference, at the bound and
    with the tie rule of test_gpu_nets.test_preroll."""
    idx = S.spread(128)
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
    print("NETS-MAX %-13s %-28s %6d rolls: max |gpu - fp64| = %.3g" % ("ckpt", "evaluate_preroll (G11)", n_cmp, worst))
    assert n_cmp >= 0.9 * 21 * len(ps)
    assert env.stats()["error_flags"] == 0
    env.close()


@pytest.mark.parametrize("n", [1, 65])
def test_small_lane_counts(bg, O, S, weights, n):
    """The staged-rows and choice checks on envs of 1 and 65 lanes: other launch shapes, the same rules."""
    idx = S.spread(65)
    if n == 1:
        for i in (idx[np.argmax(S.st[idx, 24 + S.mv[idx]])], int(np.nonzero(S.blocked_doubles)[0][0])):
            _check_staged_rows(bg, O, S, weights, np.array([i]))
            _check_choice(bg, O, S, weights, np.array([i]))
    else:
        _check_staged_rows(bg, O, S, weights, idx)
        _check_choice(bg, O, S, weights, idx)


def test_scalar_surface(bg, S):
    """32 lanes through bgamd_game_set_state / bgamd_game_enumerate / bgamd_game_legal_moves on a one-lane env, against G11."""
    one = bg.VecGame(1, seed=11, arena_rows=32768)
    lib, h = one._lib, one._h
    cap = 4096
    st, sq, ln = np.empty((cap, 28), np.int32), np.empty((cap, 4, 2), np.int8), np.empty((cap,), np.int32)
    pairs = (C.c_int8 * 52)()
    for i in S.spread(32):
        arr = (C.c_int32 * 28)(*[int(v) for v in S.st[i]])
        assert lib.bgamd_game_set_state(h, arr, int(S.mv[i])) == 0
        k = lib.bgamd_game_enumerate(h, int(S.mv[i]), int(S.dc[i, 0]), int(S.dc[i, 1]), *(x.ctypes.data_as(C.c_void_p) for x in (st, sq, ln)), cap)
        r = slice(S.off[i], S.off[i + 1])
        assert k == S.n_seq[i] <= cap, i
        assert np.array_equal(st[:k], S.states[r]) and np.array_equal(ln[:k], S.seq_len[r]) and np.array_equal(sq[:k], S.seqs[r]), i
        for die in range(1, 7):
            m = lib.bgamd_game_legal_moves(h, int(S.mv[i]), die, pairs)
            assert [(int(pairs[2 * j]), int(pairs[2 * j + 1])) for j in range(m)] == S.g11_moves(i, die), (i, die)
        snap = (C.c_int32 * 32)()
        assert lib.bgamd_game_snapshot(h, snap) == 0 and list(snap)[:29] == S.st[i].tolist() + [int(S.mv[i])]
    assert one.stats()["error_flags"] == 0
    one.close()
