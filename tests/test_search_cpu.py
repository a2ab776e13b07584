"""CPU checks of the 2-ply expectimax search (bgamd_env_step_search): the ABI is declared and exported, the fp64 reference
(tests/search_ref.py) gets its known answers right, and the 21-roll form holds for this engine's rules."""
import ctypes
import os
import re

import numpy as np
import pytest

import search_ref as S
from oracle import oracle as O

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def W():
    w = np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)
    assert w.size == O.N_PARAMS
    return w


def test_search_entry_points_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from backgammon_env import _capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bgamd.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in ("bgamd_env_step_search", "bgamd_env_search_read"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in {n for n, _, _ in _capi.SYMBOLS}, name


def _bearoff(mover):
    """Two checkers left on the mover's home board, 13 off; the opponent far from home.  For dice (6, 1) from the 6- and 1-point
    exactly one distinct afterstate bears both off."""
    s = np.zeros(28, np.int32)
    if mover == 0:                                   # PLAYER1 moves up the board: home 18..23
        s[18] = 1; s[23] = 1; s[26] = 13
        s[0:5] = -3; s[27] = 0
    else:                                            # PLAYER2 moves down: home 0..5
        s[5] = -1; s[0] = -1; s[27] = 13
        s[19:24] = 3; s[26] = 0
    return s


@pytest.mark.parametrize("mover", [0, 1])
def test_reference_takes_the_winning_bear_off(W, mover):
    s = _bearoff(mover)
    r = S.search(W, s, mover, 6, 1, 0)
    assert len(r["states"]) >= 2 and r["terminal"].sum() == 1
    want = 1.0 if mover == 0 else 0.0
    assert r["terminal"][r["choice"]] and r["v2"][r["choice"]] == want
    assert S.outcome(r["states"][r["choice"]], mover) == want


def test_reference_pass_rule_when_the_opponent_is_shut_out(W):
    """PLAYER2 on the bar against a closed board (PLAYER1 holds 18..23 with two each): for every roll PLAYER2 has no move, so the
    V2 of a candidate that keeps the board closed is the net's value of it with PLAYER2's turn bit."""
    s = np.zeros(28, np.int32)
    s[18:24] = 2; s[10] = 3
    s[25] = 1; s[2:6] = -3; s[7] = -2
    for a, b in S.ROLLS:                             # no move (a double: one empty sequence, the position itself)
        x = S.distinct_afterstates(s, 1, a, b)
        assert len(x) == 0 or (len(x) == 1 and (x[0] == s).all())
    r = S.search(W, s, 0, 2, 1, 0)
    assert r["passes"] >= 21
    closed = [i for i, c in enumerate(r["states"]) if (c[18:24] >= 2).all()]
    assert closed
    for i in closed:
        assert abs(r["v2"][i] - S.net(W, r["states"][i], 1)[0]) < 1e-12


def test_reference_top_k_1_is_the_greedy_choice(W):
    d = np.load(os.path.join(ROOT, "tests", "golden", "g10_arbitrary_boards.npz"))
    boards, dice = d["boards"], d["dice"]
    n = 0
    for i in range(0, 400, 7):
        mover, a, b = (int(x) for x in dice[i])           # (player, d1, d2)
        r = S.search(W, boards[i], mover, a, b, 1)
        cand = S.distinct_afterstates(boards[i], mover, a, b)
        if len(cand) == 0 or any(S.outcome(c, mover) is not None for c in cand):
            continue
        v = S.net(W, cand, mover)
        g = int(np.argmax(v) if mover == 0 else np.argmin(v))       # first index wins ties
        assert (r["states"][r["choice"]] == cand[g]).all()
        n += 1
    assert n >= 30


def test_afterstate_sets_do_not_depend_on_die_order():
    """The 21-roll form: for (a, b) and (b, a) the sets of distinct afterstates are equal, on the G10 boards, both players."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "g10_arbitrary_boards.npz"))
    for s in d["boards"]:
        for player in (0, 1):
            for a in range(1, 7):
                for b in range(a + 1, 7):
                    x = S.distinct_afterstates(s, player, a, b)
                    y = S.distinct_afterstates(s, player, b, a)
                    assert len(x) == len(y)
                    if len(x):
                        assert (np.unique(x, axis=0) == np.unique(y, axis=0)).all()
