"""CPU checks of the Monte Carlo rollout (bgamd_env_rollout): the ABI is declared and exported, and the fp64 reference
(tests/rollout_ref.py) gets its known answers right."""
import ctypes
import os
import re

import numpy as np
import pytest

import rollout_ref as R
import search_ref as S
from oracle import oracle as O

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SEED = 99


@pytest.fixture(scope="module")
def W():
    w = np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)
    assert w.size == O.N_PARAMS
    return w


def test_rollout_entry_points_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from backgammon_env import _capi
    src = open(os.path.join(ROOT, "include", "bgamd.h")).read()
    assert re.search(r"\bBGAMD_ROLLOUT_ROTATE\s*=\s*128\b", src)
    hdr = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in ("bgamd_env_rollout", "bgamd_env_rollout_info"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in {n for n, _, _ in _capi.SYMBOLS}, name
    assert _capi.ROLLOUT_ROTATE == 128


def _last_checker(mover):
    """The mover has one checker left, on its own ace point (any die bears it off); the opponent has all 15 on the board."""
    s = np.zeros(28, np.int32)
    if mover == 0:
        s[23] = 1; s[26] = 14
        s[0:5] = -3
    else:
        s[0] = -1; s[27] = 14
        s[19:24] = 3
    return s


@pytest.mark.parametrize("mover", [0, 1])
@pytest.mark.parametrize("rotate", [False, True])
def test_reference_last_checker_wins_in_one_turn(W, mover, rotate):
    out = R.rollout(W, [_last_checker(mover)], [mover], 40, SEED, rotate=rotate)
    assert (out["value"] == (1.0 if mover == 0 else 0.0)).all()
    assert (out["turns"] == 1).all() and not out["truncated"].any()


def test_reference_rotation_runs_through_the_36_pairs(W, monkeypatch):
    """With rotation and T = 36 the first dice of trial i are ordered pair i: (1,1), (1,2), ..., (6,6); later turns draw TURN-stream dice."""
    start = np.array([-2, 0, 0, 0, 0, 5, 0, 3, 0, 0, 0, -5, 5, 0, 0, 0, -3, 0, -5, 0, 0, 0, 0, 2, 0, 0, 0, 0], np.int32)
    seen = []
    real = S.distinct_afterstates

    def spy(s28, player, d1, d2):
        seen.append((d1, d2))
        return real(s28, player, d1, d2)
    monkeypatch.setattr(S, "distinct_afterstates", spy)
    firsts = []
    for i in range(36):
        seen.clear()
        R.trial(W, start, 0, SEED, i, i, max_plies=2, rotate=True)
        firsts.append(seen[0])
        assert seen[1] == O.turn_randoms(SEED, i, 1)[:2]
    assert firsts == [(a, b) for a in range(1, 7) for b in range(1, 7)]


def test_reference_one_turn_scores_the_afterstate_with_the_opponent_bit(W):
    start = np.array([-2, 0, 0, 0, 0, 5, 0, 3, 0, 0, 0, -5, 5, 0, 0, 0, -3, 0, -5, 0, 0, 0, 0, 2, 0, 0, 0, 0], np.int32)
    for mover in (0, 1):
        for i in (0, 7, 20, 35):
            d1, d2 = 1 + i // 6, 1 + i % 6
            cand = S.distinct_afterstates(start, mover, d1, d2)
            v = S.net(W, cand, mover)
            after = cand[int(np.argmax(v) if mover == 0 else np.argmin(v))]
            val, turns, trunc, _ = R.trial(W, start, mover, SEED, 1000 + i, i, max_plies=1, rotate=True)
            assert trunc and turns == 1
            assert val == float(S.net(W, after, 1 - mover)[0])


@pytest.mark.parametrize("winner", [0, 1])
def test_reference_finished_position_scores_its_winner_at_zero_turns(W, winner):
    s = np.zeros(28, np.int32)
    if winner == 0:
        s[26] = 15; s[0:5] = -3
    else:
        s[27] = 15; s[19:24] = 3
    for turn in (0, 1):
        out = R.rollout(W, [s], [turn], 8, SEED, max_plies=3, rotate=True)
        assert (out["value"] == (1.0 if winner == 0 else 0.0)).all()
        assert (out["turns"] == 0).all() and not out["truncated"].any()
