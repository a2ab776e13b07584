"""CPU checks of the points of a finished game (bgamd_outcomes, bgamd_env_outcomes, bgamd_env_rollout_outcomes_read): the ABI is declared
and exported, the numpy reference (tests/outcome_ref.py) gets its known answers right, and the forced positions the GPU tests use to
meet all six classes end the way tests/test_gpu_outcome.py assumes -- checked with the oracle and the fp64 net."""
import ctypes
import os
import re

import numpy as np
import pytest

import outcome_ref as OR
from oracle import oracle as O

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SEED = 4242


@pytest.fixture(scope="module")
def W():
    w = np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)
    assert w.size == O.N_PARAMS
    return w


def test_outcome_entry_points_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from backgammon_env import _capi
    src = open(os.path.join(ROOT, "include", "bgamd.h")).read()
    assert re.search(r"#define\s+BGAMD_OUTCOME_BAD\s+INT32_MIN\b", src)
    hdr = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in ("bgamd_outcomes", "bgamd_env_outcomes", "bgamd_env_rollout_outcomes_read"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in {n for n, _, _ in _capi.SYMBOLS}, name
    assert _capi.OUTCOME_BAD == -2 ** 31
    # argument checks that need no device
    buf = (ctypes.c_int32 * 28)()
    out = (ctypes.c_int32 * 1)()
    fn = _capi.load().bgamd_outcomes
    assert fn(ctypes.addressof(buf), 0, ctypes.addressof(out), None) == _capi.E_INVALID
    assert fn(None, 1, ctypes.addressof(out), None) == _capi.E_INVALID
    assert fn(ctypes.addressof(buf), 1, None, None) == _capi.E_INVALID
    assert _capi.load().bgamd_env_outcomes(None, ctypes.addressof(out), None) == _capi.E_INVALID
    assert _capi.load().bgamd_env_rollout_outcomes_read(None, None, None, None, None, None) == _capi.E_INVALID


def test_python_surface_has_the_keywords():
    import inspect
    import backgammon_env as bg
    from backgammon_env import analysis, arena
    assert callable(bg.outcomes) and callable(bg.VecGame.outcomes)
    assert inspect.signature(bg.VecGame.rollout).parameters["outcomes"].default is False
    assert inspect.signature(analysis.rollout_moves).parameters["outcomes"].default is False
    assert "a_points" in inspect.getsource(arena.head_to_head)


def test_start_position_and_both_sides_off():
    assert OR.points(OR.START) == 0
    both = np.zeros(28, np.int32)
    both[26] = both[27] = 15
    assert OR.points(both) == 1                              # PLAYER1 is checked first, and PLAYER2 has borne off: a single game
    st, want = OR.over_boards()
    assert OR.points_many(st).tolist() == want.tolist() == [1, -2]


def test_generated_family():
    st, want = OR.probe_family()
    assert len(st) == 100 and (np.abs(st[:, :24]).sum(1) + st[:, 24:].sum(1) == 30).all()
    np.testing.assert_array_equal(OR.points_many(st), want)
    # each winner: 18 gammons, 7 backgammons (6 home points + the bar), 25 single games
    assert [int((want == v).sum()) for v in (1, 2, 3, -1, -2, -3)] == [25, 18, 7, 25, 18, 7]


def _p2_probe(point=None, bar=0, off=0):
    s = np.zeros(28, np.int32)
    s[0], s[1], s[2] = -5, -5, -(4 - off)
    if point is not None:
        s[point - 1] -= 1
    s[25], s[26], s[27] = bar, 15, off
    return s


def _p1_probe(point=None, bar=0, off=0):
    s = np.zeros(28, np.int32)
    s[23], s[22], s[21] = 5, 5, 4 - off
    if point is not None:
        s[point - 1] += 1
    s[24], s[26], s[27] = bar, off, 15
    return s


def test_boundaries():
    assert OR.points(_p2_probe(18)) == 2 and OR.points(_p2_probe(19)) == 3          # PLAYER1's home starts at point 19
    assert OR.points(_p2_probe(24)) == 3 and OR.points(_p2_probe(1)) == 2
    assert OR.points(_p1_probe(7)) == -2 and OR.points(_p1_probe(6)) == -3          # PLAYER2's home ends at point 6
    assert OR.points(_p1_probe(1)) == -3 and OR.points(_p1_probe(24)) == -2
    assert OR.points(_p2_probe(None, bar=1)) == 3 and OR.points(_p1_probe(None, bar=1)) == -3     # either side's bar
    # a checker borne off outweighs everything else
    assert OR.points(_p2_probe(None, bar=1, off=1)) == 1 and OR.points(_p1_probe(None, bar=1, off=1)) == -1
    assert OR.points(_p2_probe(20, off=1)) == 1 and OR.points(_p1_probe(3, off=1)) == -1
    # the winner's own off count (15: on the planes, the bit of the loser's bar / off) is never read as the loser's
    g1, g2 = _p2_probe(10), _p1_probe(10)
    assert g1[26] == 15 and g1[27] == 0 and g1[25] == 0 and OR.points(g1) == 2
    assert g2[27] == 15 and g2[26] == 0 and g2[24] == 0 and OR.points(g2) == -2


def test_trial_with_board_is_rollout_refs_trial(W):
    import rollout_ref as R
    st, tu, _, _ = OR.forced_positions()
    for p in (0, 7, 9):
        for i in (0, 5, 17):
            for M in (0, 2):
                a = R.trial(W, st[p], tu[p], SEED, 100 * p + i, i, M, True)
                b = OR.trial_with_board(W, st[p], tu[p], SEED, 100 * p + i, i, M, True)
                assert a == b[:4]


def test_forced_positions_end_as_the_gpu_tests_assume(W):
    """Every ordered pair of the rotation ends positions 1a .. 7 in one turn with the listed points; position 8 ends at -3 exactly for the
    rolls holding a 1 (a PLAYER1 checker on points 2-7 blocks PLAYER2's overrun) and is not over after one turn
    otherwise.  Position 7 also unrotated, with the dice of its trial ids.  So a rotated rollout with T a multiple of 36 over these
    positions meets all six classes."""
    st, tu, want, names = OR.forced_positions()
    assert names == ["1a", "1b", "2a", "2b", "3", "4", "5", "6", "7", "8"]
    assert want.tolist() == [2, 2, 3, 3, 3, 1, -2, -3, -1, -3]
    assert {int(x) for x in want} == {1, 2, 3, -1, -2, -3}
    assert (OR.points_many(st) == 0).all()
    for p in range(9):
        for i in range(36):
            v, turns, trunc, near, board = OR.trial_with_board(W, st[p], tu[p], SEED, p * 36 + i, i, 0, True)
            assert turns == 1 and not trunc and not near, (names[p], i)
            assert OR.points(board) == want[p] and v == (1.0 if want[p] > 0 else 0.0), (names[p], i)
    for i in range(36):                                       # position 7 unrotated
        v, turns, trunc, near, board = OR.trial_with_board(W, st[8], tu[8], SEED, 8 * 72 + i, i, 0, False)
        assert turns == 1 and OR.points(board) == -1 and v == 0.0
    n3 = 0
    for i in range(36):
        d1, d2 = 1 + i // 6, 1 + i % 6
        v, turns, trunc, near, board = OR.trial_with_board(W, st[9], tu[9], SEED, 9 * 36 + i, i, 1, True)
        if d1 == 1 or d2 == 1:
            assert turns == 1 and not trunc and OR.points(board) == -3, i
            n3 += 1
        else:
            assert trunc and turns == 1 and OR.points(board) == 0, i
    assert n3 == 11
