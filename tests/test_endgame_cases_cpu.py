"""The end-game position set (tests/endgame_cases.py) on the CPU: its census condition, the oracle against the UNMODIFIED reference on every
lane (fixture G12: sequences, afterstates, legalMoves, is_game_over and every tryMove probe -- refusals and the unchecked bear-off branch
of SURVEY Q6 included -- and the compiled reference itself where oracle/_ref is present), the plain-Python restatement of the rules
(tests/rules_ref.py) against the oracle, the set's power -- each deliberately wrong reading of the end-game rules differs from the oracle
on at least 8 lanes -- and the conditions that tests/test_gpu_rules_endgame.py rests on."""
import os
import re

import numpy as np
import pytest

import endgame_cases as EC
import nets as N
import outcome_ref as OC
import rollout_ref as R
import rule_cases as RC
import rules_ref as RR
from oracle import oracle as O
from test_rule_cases_cpu import _load_reference

G10_BYTES = 506616


@pytest.fixture(scope="module")
def case_set():
    return EC.cases()


@pytest.fixture(scope="module")
def answers(case_set):
    return EC.enumerate_oracle(*case_set)


@pytest.fixture(scope="module")
def cen(case_set, answers):
    return EC.census(case_set, answers)


@pytest.fixture(scope="module")
def g12(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g12_endgame_boards.npz")))


@pytest.fixture(scope="module")
def probe_rows(case_set):
    return EC.probes(case_set)


def test_generator_reproduces_the_fixture_inputs(case_set, probe_rows, g12):
    st, mv, dc = case_set
    assert len(st) <= 4096
    for got, key in ((st, "boards"), (mv, "mover"), (dc, "dice")):
        assert got.shape == g12[key].shape and got.astype(np.int8).tobytes() == g12[key].tobytes(), key
        assert (got.astype(np.int8) == got).all()
    assert np.array_equal(probe_rows, g12["probes"])
    st2, mv2, dc2 = EC.cases()                                # the same arrays on every call
    assert st2.tobytes() == st.tobytes() and mv2.tobytes() == mv.tobytes() and dc2.tobytes() == dc.tobytes()
    assert np.array_equal(EC.probes((st2, mv2, dc2)), probe_rows)


def test_boards_are_legal_and_not_over(case_set):
    st, mv, dc = case_set
    assert (np.clip(st[:, :24], 0, None).sum(1) + st[:, 24] + st[:, 26] == 15).all()
    assert (np.clip(-st[:, :24], 0, None).sum(1) + st[:, 25] + st[:, 27] == 15).all()
    assert (st[:, 24:] >= 0).all() and (st[:, 26:] <= 14).all() and np.isin(mv, (0, 1)).all() and ((dc >= 1) & (dc <= 6)).all()
    assert not any(O.over(O.State.from28(st[i], int(mv[i])))[0] for i in range(len(st)))
    drawn = slice(0, EC.N_RANDOM)
    doubles = (dc[drawn, 0] == dc[drawn, 1]).mean()
    assert 0.3 <= doubles <= 0.4, doubles
    own_off = st[np.arange(len(st)), 26 + mv]
    assert sorted(set(own_off.tolist())) == list(range(15)) and np.abs(st[:, :24]).max() == 15
    sign = np.where(mv == 0, 1, -1)[:, None]
    home = np.where(mv[:, None] == 0, st[:, 18:24], st[:, 0:6])
    in_home = ((home * sign) < 0).any(1)
    assert 0.3 <= in_home[drawn].mean() <= 0.7, in_home[drawn].mean()      # the opponent inside the mover's home: about half the boards


def test_census_condition(case_set, answers, cen, g12, golden_dir):
    """The condition of the set: every class holds at least 8 lanes; the whole set stays within 80 000 sequences and the fixture no larger
    than G10's file.  The probes reach every message tryMove can give, and success, at least 8 times each."""
    counts, total, _ = cen
    st, mv, dc = case_set
    print("ENDGAME-CENSUS lanes %d, doubles %d, sequences %d" % (len(st), int((dc[:, 0] == dc[:, 1]).sum()), total))
    for k in EC.CLASSES:
        print("ENDGAME-CENSUS %-32s %5d" % (k, counts[k]))
    smallest = min(counts, key=counts.get)
    print("ENDGAME-CENSUS smallest class %s: %d lanes" % (smallest, counts[smallest]))
    short = {k: v for k, v in counts.items() if v < EC.MIN_LANES}
    assert not short, short
    assert sorted(counts) == sorted(EC.CLASSES) and EC.MIN_LANES == 8
    for k in EC.CLASSES:                                      # the table in the module's docstring is this census
        assert re.search(r"\b%s\s+%d\b" % (k, counts[k]), EC.__doc__), (k, counts[k])
    assert total <= EC.MAX_SEQUENCES == 80000 and total == len(g12["states"])
    assert os.path.getsize(os.path.join(golden_dir, "g12_endgame_boards.npz")) <= G10_BYTES
    per_msg = np.bincount(g12["probe_code"], minlength=8)
    per_kind = np.bincount(g12["probes"][:, 1], minlength=len(EC.PROBE_KINDS))
    print("ENDGAME-CENSUS probes %d; per message %s; per kind %s" % (len(g12["probes"]), per_msg.tolist(), per_kind.tolist()))
    assert g12["messages"].tolist() == [O.ERR_MESSAGES[k] for k in range(8)] == list(RR.MESSAGES)
    # "Origin out of range" is the one message the reference never gives: its test of the origin comes first and refuses every origin
    # outside 0..25 as "Invalid origin" (the probes with origin -1 and 26 show it)
    assert per_msg[2] == 0 and (np.delete(per_msg, 2) >= 8).all() and (per_kind >= 8).all()
    kinds = g12["probes"][:, 1]
    K = {k: j for j, k in enumerate(EC.PROBE_KINDS)}
    assert (g12["probe_code"][np.isin(kinds, (K["origin_m1"], K["origin_26"]))] == 1).all()


def _g12_lane(g12, seq_off, mv_off, i):
    r = slice(seq_off[i], seq_off[i + 1])
    seqs = [[(int(o), int(d)) for o, d in x[:n]] for x, n in zip(g12["seqs"][r], g12["seq_len"][r])]
    dies = [x[:n].tolist() for x, n in zip(g12["seq_dies"][r], g12["seq_len"][r])]
    nd = len(g12["dies"])
    moves = [[(int(o), int(d)) for o, d in g12["moves"][mv_off[i * nd + k]:mv_off[i * nd + k + 1]]] for k in range(nd)]
    return seqs, g12["states"][r].astype(np.int32), moves, dies, g12["over"][r]


def test_oracle_vs_reference_on_every_lane(case_set, answers, g12):
    """Fixture G12 (the unmodified reference): sequences in order, the die of every move, afterstates, legalMoves for the six dice,
    is_game_over of every afterstate that bears off -- every lane."""
    st, mv, dc = case_set
    assert g12["dies"].tolist() == [1, 2, 3, 4, 5, 6]
    seq_off = np.concatenate([[0], np.cumsum(g12["n_seq"])])
    mv_off = np.concatenate([[0], np.cumsum(g12["n_moves"].ravel())])
    assert seq_off[-1] == len(g12["seqs"]) == len(g12["states"]) == len(g12["over"]) and mv_off[-1] == len(g12["moves"])
    n_over = 0
    for i in range(len(st)):
        ref_seqs, ref_states, ref_moves, ref_dies, ref_over = _g12_lane(g12, seq_off, mv_off, i)
        seqs, states, moves, dies = answers[i]
        where = (i, st[i].tolist(), int(mv[i]), dc[i].tolist())
        assert seqs == ref_seqs and dies == ref_dies, where
        assert states.shape == ref_states.shape and (states == ref_states).all(), where
        assert moves == ref_moves, where
        for k in range(len(seqs)):
            bears = states[k, 26 + mv[i]] != st[i, 26 + mv[i]]
            assert bears == (ref_over[k] >= 0), where
            if bears:
                over, winner = O.over(O.State.from28(states[k], int(mv[i])))
                assert (1 + winner if over else 0) == ref_over[k], where
                n_over += int(over)
    assert n_over == int((g12["over"] >= 1).sum()) >= 500       # sequences that end the game


def test_oracle_try_move_vs_reference_on_every_probe(case_set, probe_rows, g12):
    """Every probe of every lane: the message, and the position afterwards -- the reference's where it accepted the move (the bear-off
    branch accepts an overrun the rules deny, the wrong end and a point outside home: SURVEY Q6), untouched where it refused."""
    st, mv, dc = case_set
    code, after = EC.probe_oracle(case_set, probe_rows)
    bad = np.nonzero(code != g12["probe_code"])[0]
    assert len(bad) == 0, [(probe_rows[j].tolist(), int(code[j]), int(g12["probe_code"][j])) for j in bad[:5]]
    ok = code == 0
    assert ok.sum() == len(g12["probe_after"])
    assert np.array_equal(after[ok], g12["probe_after"].astype(np.int32))
    assert np.array_equal(after[~ok], st[probe_rows[~ok, 0]])
    K = {k: j for j, k in enumerate(EC.PROBE_KINDS)}
    kind = probe_rows[:, 1]
    on_bar = st[probe_rows[:, 0], 24 + probe_rows[:, 2]] > 0
    for name in ("exact", "overrun_far", "overrun_near", "wrong_end", "from_outside"):     # accepted whenever the mover is off the bar
        sel = kind == K[name]
        assert (code[sel & ~on_bar] == 0).all() and (code[sel & on_bar] == 1).all() and (sel & ~on_bar).sum() >= 8, name
    assert (code[(kind == K["bar_to_off"]) & on_bar] == 7).all() and (code[(kind == K["bar_to_off"]) & ~on_bar] == 1).all()
    assert (code[kind == K["point_while_on_bar"]] == 1).all()
    for name, want in (("direction", 4), ("dice_mismatch", 5), ("blocked", 6), ("dest_m1", 3), ("dest_26", 3)):
        sel = (kind == K[name]) & ~on_bar
        assert (code[sel] == want).all() and sel.sum() >= 8, name
    assert (code[(kind == K["forward"]) & ~on_bar] == 0).sum() >= 8


def test_live_reference_on_a_sample(case_set, answers, probe_rows):
    """Where the compiled reference is present it is asked again; where it is absent the fixture alone speaks (the tests above) and this
    one has nothing to add."""
    rb = _load_reference()
    if rb is None:
        return
    st, mv, dc = case_set
    p1, p2 = rb.Player("a", rb.PlayerType.PLAYER1), rb.Player("b", rb.PlayerType.PLAYER2)
    code, after = EC.probe_oracle(case_set, probe_rows)
    for i in range(0, len(st), 5):
        g = RC.reference_game(rb, p1, p2, st[i])
        pl, d1, d2 = int(mv[i]), int(dc[i, 0]), int(dc[i, 1])
        q, a = g.evaluateTurnSequences(pl, d1, d2)
        seqs, states, moves, dies = answers[i]
        assert [list(map(tuple, x)) for x in q] == seqs, i
        assert a.shape == states.shape and (a == states).all(), i
        for die in range(1, 7):
            assert g.legalMoves(pl, die) == moves[die - 1], (i, die)
        for j in np.nonzero(probe_rows[:, 0] == i)[0]:
            _, kind, player, die, o, d = probe_rows[j].tolist()
            c = g.clone()
            ok, msg = c.tryMove(p1 if player == 0 else p2, die, o, d)
            assert (ok, msg) == (code[j] == 0, O.ERR_MESSAGES[int(code[j])]), (i, EC.PROBE_KINDS[kind])
            got = c.getGameBoard() + [c.getJailedCount(0), c.getJailedCount(1), c.getBornOffCount(0), c.getBornOffCount(1)]
            assert got == after[j].tolist(), (i, EC.PROBE_KINDS[kind])
            assert c.is_game_over() == O.over(O.State.from28(after[j], pl)), (i, EC.PROBE_KINDS[kind])


def _differs(case_set, answers, wrong):
    st, mv, dc = case_set
    lanes = []
    for i in range(len(st)):
        seqs, states = RR.turn_sequences(st[i].tolist(), int(mv[i]), int(dc[i, 0]), int(dc[i, 1]), wrong=wrong)
        same = seqs == answers[i][0] and np.array_equal(np.array(states, dtype=np.int32).reshape(-1, 28), answers[i][1])
        if not same:
            lanes.append(i)
    return lanes


def _turn_end_differs(case_set, answers, wrong):
    """The lanes on which turn_end disagrees with the oracle's step (over, winner, the side to move) for the first, the last or the first
    winning sequence."""
    st, mv, dc = case_set
    lanes = []
    for i in range(len(st)):
        seqs, states = answers[i][0], answers[i][1]
        n, pl = len(seqs), int(mv[i])
        wins = np.nonzero(states[:, 26 + pl] == 15)[0] if n else []
        for k in sorted({0, n - 1} | {int(w) for w in wins[:1]}) if n else [None]:
            s = O.State.from28(st[i], pl)
            o = O.step(s, int(dc[i, 0]), int(dc[i, 1]), 0, choice_u32=EC.u32_for(k, n) if n else 0)
            assert o.chosen == (k if n else -1)
            if (bool(o.over), o.winner if o.over else -1, s.turn) != RR.turn_end(s.to28().tolist(), pl, wrong=wrong):
                lanes.append(i)
                break
    return lanes


def test_restatement_equals_the_oracle(case_set, answers, probe_rows):
    st, mv, dc = case_set
    assert _differs(case_set, answers, None) == []
    assert _turn_end_differs(case_set, answers, None) == []
    for i in range(len(st)):
        for die in range(1, 7):
            assert RR.legal_moves(st[i].tolist(), int(mv[i]), die) == answers[i][2][die - 1], (i, die)
    code, after = EC.probe_oracle(case_set, probe_rows)
    for j, (i, kind, player, die, o, d) in enumerate(probe_rows.tolist()):
        msg, t = RR.try_move(st[i].tolist(), player, die, o, d)
        assert msg == O.ERR_MESSAGES[int(code[j])] and t == after[j].tolist(), (i, EC.PROBE_KINDS[kind])


@pytest.mark.parametrize("wrong", RR.ENDGAME_VARIANTS)
def test_each_wrong_variant_differs_on_at_least_8_lanes(case_set, answers, wrong):
    """The set's power: a device (or an oracle) that read the end-game rules in one of these ways would fail on at least 8 lanes."""
    lanes = _turn_end_differs(case_set, answers, wrong) if wrong == "o" else _differs(case_set, answers, wrong)
    print("ENDGAME-POWER variant %s differs on %d lanes" % (wrong, len(lanes)))
    assert len(lanes) >= 8, (wrong, len(lanes))


def test_points_of_every_winning_afterstate(case_set, answers, cen, g12):
    """outcome_ref.points on every afterstate that ends the game: the winner is the one is_game_over named to the fixture, and each of
    the six results (and both kinds of backgammon) is held by at least 8 lanes."""
    counts, _, per_lane = cen
    pts = OC.points_many(g12["states"].astype(np.int32))
    over = g12["over"]
    assert ((pts != 0) == (over >= 1)).all()
    assert ((pts > 0) == (over == 1)).all() and ((pts < 0) == (over == 2)).all()
    lane = np.repeat(np.arange(len(g12["n_seq"])), g12["n_seq"])
    for v in (1, 2, 3, -1, -2, -3):
        lanes = len(set(lane[pts == v].tolist()))
        print("ENDGAME-POINTS %+d: %d lanes, %d afterstates" % (v, lanes, int((pts == v).sum())))
        assert lanes >= 8 and lanes == counts["win_points_%d_P%d" % (abs(v), 1 if v > 0 else 2)]
    assert counts["win_bg_bar"] >= 8 and counts["win_bg_home"] >= 8


@pytest.mark.parametrize("family", N.PARITY)
def test_fp32_forward_is_within_a_quarter_of_the_parity_bound_on_these_rows(answers, case_set, family):
    """The condition the flat 1e-5 bound of the GPU tests rests on (tests/test_nets_cpu.py states it for the rows used there), on the
    afterstates of this set: borne-off counts up to 15 (the rows that end the game go through the net like any other) and stacks of
    up to 15 checkers."""
    w = N.table(family)
    worst = 0.0
    for t in (0, 1):
        rows = np.unique(np.concatenate([a[1] for i, a in enumerate(answers) if case_set[1][i] == t and len(a[1])]), axis=0)
        X = O.encode(rows, t)
        worst = max(worst, float(np.abs(N.forward_np32(w, X).astype(np.float64) - O.forward_f64(w, X)).max()))
    print("ENDGAME-FP32 %-13s max |numpy fp32 - fp64| = %.3g" % (family, worst))
    assert worst <= 2.5e-6, (family, worst)


def test_rollout_positions_hold_few_near_ties(case_set, cen, weights):
    """The condition the rollout test of the GPU file rests on: from its 24 positions, the reference alone marks fewer than 1 % of the
    trials as near ties (rotation on and off), and the trials it compares reach all six results."""
    st, mv, dc = case_set
    lanes = EC.rollout_lanes(case_set, cen[2])
    T = EC.ROLLOUT_TRIALS
    seen = set()
    for rotate in (False, True):
        near = np.zeros((len(lanes), T), bool)
        for p, i in enumerate(lanes):
            for t in range(T):
                pts, near[p, t] = OC.trial_points(weights, st[i], int(mv[i]), EC.SEED, p * T + t, t, 0, rotate)
                if not near[p, t]:
                    seen.add(pts)
        print("ENDGAME-ROLLOUT rotate %d: %d of %d trials near a tie" % (rotate, int(near.sum()), near.size))
        assert near.mean() < 0.01, near.mean()
    assert R.TIE_EPS == 2e-5 and seen == {1, 2, 3, -1, -2, -3}, seen
