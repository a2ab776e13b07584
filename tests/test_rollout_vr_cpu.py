"""CPU checks of the pre-roll evaluation and the luck-adjusted rollout (bgamd_env_evaluate_preroll, BGAMD_ROLLOUT_VR): the ABI is
declared and exported, and the fp64 reference (tests/rollout_vr_ref.py) gets its known answers right."""
import ctypes
import os
import re

import numpy as np
import pytest

import rollout_vr_ref as V
import search_ref as S
from oracle import oracle as O

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SEED = 99
START = np.array([-2, 0, 0, 0, 0, 5, 0, 3, 0, 0, 0, -5, 5, 0, 0, 0, -3, 0, -5, 0, 0, 0, 0, 2, 0, 0, 0, 0], np.int32)


@pytest.fixture(scope="module")
def W():
    w = np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)
    assert w.size == O.N_PARAMS
    return w


def test_vr_entry_points_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from backgammon_env import _capi
    src = open(os.path.join(ROOT, "include", "bgamd.h")).read()
    assert re.search(r"\bBGAMD_ROLLOUT_VR\s*=\s*256\b", src)
    hdr = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in ("bgamd_env_evaluate_preroll", "bgamd_env_rollout_vr_read"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in {n for n, _, _ in _capi.SYMBOLS}, name
    assert _capi.ROLLOUT_VR == 256


def test_roll_index_follows_the_search_order():
    assert [V.roll_index(a, b) for a, b in S.ROLLS] == list(range(21))
    assert all(V.roll_index(b, a) == V.roll_index(a, b) for a, b in S.ROLLS)


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
def test_last_checker_has_no_luck(W, mover, rotate):
    """Every roll bears the last checker off to the same afterstate: every f is equal and the luck vanishes."""
    f, mean = V.preroll(W, _last_checker(mover), mover)
    assert (f == f[0]).all()
    assert abs(mean - f[0]) < 1e-15
    for i in range(40):
        x, turns, trunc, _, L = V.trial(W, _last_checker(mover), mover, SEED, i, i, rotate=rotate)
        assert turns == 1 and not trunc and x == (1.0 if mover == 0 else 0.0)
        assert abs(L) < 1e-14
        assert abs((x - L) - x) < 1e-14


@pytest.mark.parametrize("mover", [0, 1])
def test_mean_over_the_36_ordered_pairs_is_the_weighted_mean(W, mover):
    """Why rotated turn-0 luck cancels: the 36 ordered pairs visit each non-double roll twice and each double once."""
    g10 = np.load(os.path.join(ROOT, "tests", "golden", "g10_arbitrary_boards.npz"))
    for s in (START, g10["boards"][7], g10["boards"][700]):
        f, mean = V.preroll(W, np.asarray(s, np.int32), mover)
        pairs = np.mean([f[V.roll_index(1 + k // 6, 1 + k % 6)] for k in range(36)])
        assert abs(pairs - mean) < 1e-15


@pytest.mark.parametrize("winner", [0, 1])
def test_finished_position_has_no_luck(W, winner):
    s = np.zeros(28, np.int32)
    if winner == 0:
        s[26] = 15; s[0:5] = -3
    else:
        s[27] = 15; s[19:24] = 3
    for turn in (0, 1):
        f, _ = V.preroll(W, s, turn)
        assert (f == (1.0 if winner == 0 else 0.0)).all()
        for rotate in (False, True):
            out = V.rollout(W, [s], [turn], 8, SEED, max_plies=3, rotate=rotate)
            assert (out["luck"] == 0.0).all() and (out["turns"] == 0).all()


@pytest.mark.parametrize("mover", [0, 1])
def test_two_turn_truncated_trial_from_reply_values(W, mover):
    j = 17
    x, turns, trunc, _, L = V.trial(W, START, mover, SEED, j, j, max_plies=2)
    assert trunc and turns == 2
    s, m, want = START.copy(), mover, 0.0
    for k in range(2):
        d1, d2, _, _ = O.turn_randoms(SEED, j, k)
        R, _ = S.reply_values(W, s, m)
        E = sum(w * r for w, r in zip(S.ROLL_W, R))
        want += R[V.roll_index(d1, d2)] - E
        cand = S.distinct_afterstates(s, m, d1, d2)
        v = S.net(W, cand, m)
        s = cand[int(np.argmax(v) if m == 0 else np.argmin(v))]
        m ^= 1
    assert abs(L - want) < 1e-12
    assert x == float(S.net(W, s, m)[0])


def test_luck_has_mean_zero(W):
    """E[luck | history] = 0: over a few hundred truncated trials the mean luck total is within 4 standard errors of 0."""
    g10 = np.load(os.path.join(ROOT, "tests", "golden", "g10_arbitrary_boards.npz"))
    idx = np.arange(4) * (len(g10["boards"]) // 4)
    st = np.concatenate([START[None], g10["boards"][idx]]).astype(np.int32)
    tu = np.concatenate([[0], g10["dice"][idx, 0]]).astype(np.int32)
    out = V.rollout(W, st, tu, 64, SEED, max_plies=2, rotate=False)
    L = out["luck"].ravel()
    assert np.count_nonzero(L) > len(L) // 2
    assert abs(L.mean()) <= 4 * L.std(ddof=1) / np.sqrt(len(L)), (L.mean(), L.std(ddof=1))
