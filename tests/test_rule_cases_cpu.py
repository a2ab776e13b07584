"""The bar-heavy position set (tests/rule_cases.py) on the CPU: its census condition, the oracle against the UNMODIFIED reference on every
lane (fixture G11, and the compiled reference itself where oracle/_ref is present), the plain-Python restatement of the rules
(tests/rules_ref.py) against the oracle, and the set's power -- each deliberately wrong reading of the bar rules differs from the oracle on
at least 8 lanes."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

import nets as N
import rule_cases as RC
import rules_ref as RR
from oracle import oracle as O


@pytest.fixture(scope="module")
def case_set():
    return RC.cases()


@pytest.fixture(scope="module")
def answers(case_set):
    return RC.enumerate_oracle(*case_set)


@pytest.fixture(scope="module")
def g11(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g11_bar_boards.npz")))


def test_generator_reproduces_the_fixture_inputs(case_set, g11):
    st, mv, dc = case_set
    assert len(st) <= 4096
    for got, key in ((st, "boards"), (mv, "mover"), (dc, "dice")):
        assert got.shape == g11[key].shape and got.astype(np.int8).tobytes() == g11[key].tobytes(), key
        assert (got.astype(np.int8) == got).all()
    st2, mv2, dc2 = RC.cases()                                # the same arrays on every call
    assert st2.tobytes() == st.tobytes() and mv2.tobytes() == mv.tobytes() and dc2.tobytes() == dc.tobytes()


def test_boards_are_legal_and_not_over(case_set):
    st, mv, dc = case_set
    assert (np.clip(st[:, :24], 0, None).sum(1) + st[:, 24] + st[:, 26] == 15).all()
    assert (np.clip(-st[:, :24], 0, None).sum(1) + st[:, 25] + st[:, 27] == 15).all()
    assert (st[:, 24:] >= 0).all() and (st[:, 24:26] <= 15).all() and np.isin(mv, (0, 1)).all() and ((dc >= 1) & (dc <= 6)).all()
    assert not any(O.over(O.State.from28(st[i], int(mv[i])))[0] for i in range(len(st)))
    doubles = (dc[:, 0] == dc[:, 1]).mean()
    assert 0.4 <= doubles <= 0.6, doubles
    assert st[:, 24].max() == 15 and st[:, 25].max() == 15


def test_census_condition(case_set, answers):
    """The condition of the set: every class holds at least 8 lanes, and the lists stay small (under 200 000 sequences in all)."""
    counts, total, _ = RC.census(case_set, answers)
    print("RULE-CENSUS lanes %d, doubles %d, sequences %d" % (len(case_set[0]), int((case_set[2][:, 0] == case_set[2][:, 1]).sum()), total))
    for k in RC.CLASSES:
        print("RULE-CENSUS %-26s %5d" % (k, counts[k]))
    short = {k: v for k, v in counts.items() if v < RC.MIN_LANES}
    assert not short, short
    assert sorted(counts) == sorted(RC.CLASSES)
    for k in RC.CLASSES:                                      # the table in the module's docstring is this census
        assert re.search(r"\b%s\s+%d\b" % (k, counts[k]), RC.__doc__), (k, counts[k])
    assert total < 200000


def _g11_lane(g11, seq_off, mv_off, i):
    r = slice(seq_off[i], seq_off[i + 1])
    seqs = [[(int(o), int(d)) for o, d in x[:n]] for x, n in zip(g11["seqs"][r], g11["seq_len"][r])]
    nd = len(g11["dies"])
    moves = [[(int(o), int(d)) for o, d in g11["moves"][mv_off[i * nd + k]:mv_off[i * nd + k + 1]]] for k in range(nd)]
    return seqs, g11["states"][r].astype(np.int32), moves


def test_oracle_vs_reference_on_every_lane(case_set, answers, g11):
    """Fixture G11 (the unmodified reference, its bar counts built through hits): sequences in order, afterstates, legalMoves for the six
    dice -- every lane."""
    st, mv, dc = case_set
    assert g11["dies"].tolist() == [1, 2, 3, 4, 5, 6]
    seq_off = np.concatenate([[0], np.cumsum(g11["n_seq"])])
    mv_off = np.concatenate([[0], np.cumsum(g11["n_moves"].ravel())])
    assert seq_off[-1] == len(g11["seqs"]) == len(g11["states"]) and mv_off[-1] == len(g11["moves"])
    for i in range(len(st)):
        ref_seqs, ref_states, ref_moves = _g11_lane(g11, seq_off, mv_off, i)
        seqs, states, moves = answers[i]
        where = (i, st[i].tolist(), int(mv[i]), dc[i].tolist())
        assert seqs == ref_seqs, where
        assert states.shape == ref_states.shape and (states == ref_states).all(), where
        assert moves == ref_moves, where


def _load_reference():
    ref_dir = os.path.join(os.path.dirname(__file__), "..", "oracle", "_ref")
    so = [f for f in os.listdir(ref_dir)] if os.path.isdir(ref_dir) else []
    so = sorted(f for f in so if f.startswith("backgammon_env") and f.endswith(".so"))
    if not so:
        return None
    spec = importlib.util.spec_from_file_location("backgammon_env", os.path.join(ref_dir, so[0]))
    saved = sys.modules.pop("backgammon_env", None)
    try:
        rb = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(rb)
    finally:
        if saved is not None:
            sys.modules["backgammon_env"] = saved
    return rb


def test_live_reference_on_a_sample(case_set, answers):
    """Where the compiled reference is present it is asked again, with its bars built as the fixture's script builds them; where it is
    absent the fixture alone speaks (the test above) and this one has nothing to add."""
    rb = _load_reference()
    if rb is None:
        return
    st, mv, dc = case_set
    p1, p2 = rb.Player("a", rb.PlayerType.PLAYER1), rb.Player("b", rb.PlayerType.PLAYER2)
    for i in range(0, len(st), 5):
        g = RC.reference_game(rb, p1, p2, st[i])
        pl, d1, d2 = int(mv[i]), int(dc[i, 0]), int(dc[i, 1])
        q, a = g.evaluateTurnSequences(pl, d1, d2)
        seqs, states, moves = answers[i]
        assert [list(map(tuple, x)) for x in q] == seqs, i
        assert a.shape == states.shape and (a == states).all(), i
        for die in range(1, 7):
            assert g.legalMoves(pl, die) == moves[die - 1], (i, die)
        # one applied move: tryMove's message and the state it leaves, bar counts included
        for die in (d1, d2):
            if moves[die - 1]:
                o, d = moves[die - 1][-1]
                s = O.State.from28(st[i], pl)
                ok, msg = O.try_move(s, pl, die, o, d)
                assert g.tryMove(p1 if pl == 0 else p2, die, o, d) == (ok, msg) and ok
                got = g.getGameBoard() + [g.getJailedCount(0), g.getJailedCount(1), g.getBornOffCount(0), g.getBornOffCount(1)]
                assert got == s.to28().tolist(), (i, die)
                break


def _differs(case_set, answers, wrong):
    st, mv, dc = case_set
    lanes = []
    for i in range(len(st)):
        seqs, states = RR.turn_sequences(st[i].tolist(), int(mv[i]), int(dc[i, 0]), int(dc[i, 1]), wrong=wrong)
        same = seqs == answers[i][0] and np.array_equal(np.array(states, dtype=np.int32).reshape(-1, 28), answers[i][1])
        if not same:
            lanes.append(i)
    return lanes


def test_restatement_equals_the_oracle(case_set, answers):
    st, mv, dc = case_set
    assert _differs(case_set, answers, None) == []
    for i in range(len(st)):
        for die in range(1, 7):
            assert RR.legal_moves(st[i].tolist(), int(mv[i]), die) == answers[i][2][die - 1], (i, die)
    # and away from the bar: the restatement is a reading of all the rules (bear-off and its overrun asymmetry included)
    from helpers import random_boards
    sb = random_boards(600, 5)
    rng = np.random.RandomState(6)
    for i in range(len(sb)):
        pl, d1, d2 = int(rng.randint(2)), int(rng.randint(1, 7)), int(rng.randint(1, 7))
        q, ln, a = O.evaluate_turn_sequences(O.State.from28(sb[i], pl), pl, d1, d2 if i % 4 else d1)
        if len(ln) > 3000:
            continue
        seqs, states = RR.turn_sequences(sb[i].tolist(), pl, d1, d2 if i % 4 else d1)
        assert seqs == O.sequences_as_lists(q, ln), i
        assert np.array_equal(np.array(states, dtype=np.int32).reshape(-1, 28), a), i


@pytest.mark.parametrize("family", N.PARITY)
def test_fp32_forward_is_within_a_quarter_of_the_parity_bound_on_these_rows(answers, case_set, family):
    """The condition the flat 1e-5 bound of the GPU tests rests on (tests/test_nets_cpu.py states it for the rows used there), on the
    afterstates of this set: bar features up to 7.5, where the checkpoint's games stop at 1 or 1.5."""
    w = N.table(family)
    worst = 0.0
    for t in (0, 1):
        rows = np.unique(np.concatenate([a[1] for i, a in enumerate(answers) if case_set[1][i] == t and len(a[1])]), axis=0)
        X = O.encode(rows, t)
        worst = max(worst, float(np.abs(N.forward_np32(w, X).astype(np.float64) - O.forward_f64(w, X)).max()))
    print("RULE-FP32 %-13s max |numpy fp32 - fp64| = %.3g" % (family, worst))
    assert worst <= 2.5e-6, (family, worst)


@pytest.mark.parametrize("wrong", RR.VARIANTS)
def test_each_wrong_variant_differs_on_at_least_8_lanes(case_set, answers, wrong):
    """The set's power: a device (or an oracle) that read the bar rules in one of these ways would fail on at least 8 lanes."""
    lanes = _differs(case_set, answers, wrong)
    print("RULE-POWER variant %s differs on %d lanes" % (wrong, len(lanes)))
    assert len(lanes) >= 8, (wrong, len(lanes))
