"""CPU checks of the doubling cube (include/bgamd.h, bgamd_env_rollout_cube):
  (1) tests/cube_model.py against a second statement of the rule, written as one loop over the turns with nothing shared;
  (2) four deliberately wrong models are told apart from it on the same test set;
  (3) the conditions tests/test_gpu_rollout_cube.py rests on, under the fp64 rollout reference: for its positions, shapes, thresholds and
      start tables every class of cube history occurs, and still does when every mean moves by the value tolerance;
  (4) plumbing that fails without the feature: the header declares the entry points, the ctypes table binds them, VecGame.rollout
      accepts cube=, analysis.cube_action exists."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import cube_cases as CC
import cube_model as CM

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- (1) a second statement of the rule -------------------------------------------------------------------------------------------------

def restated(turns, points, value, double_at, pass_at, too_good_at, max_cube, jacoby, hold, c0, o0, bug=None):
    """One loop over the turns, plain ints and floats.  -> (cube, owner, dropped, passed, doubles, equity).  bug: one of the four wrong
    models of (2), else the rule."""
    c, o, dropped, passed, n = c0, o0, -1, 0, 0
    k = 0
    for mover, mean, over in turns:
        side = 1 if mover == 0 else 2
        other = 3 - side
        may = dropped == -1 and (not over) and c < max_cube and (o == 0 or o == side or bug == "offer without access")
        if may and not (hold and k == 0):
            w = mean if side == 1 else 1.0 - mean
            if w >= double_at and w <= too_good_at:
                if (w >= pass_at) if bug == ">= at pass_at" else (w > pass_at):
                    dropped, passed = k, other
                else:
                    c, o, n = c + c, other, n + 1
        k += 1
    if dropped != -1:
        stake = 2 * c if bug == "drop pays 2c" else c
        e = float(stake) if passed == 2 else -float(stake)
    elif points == 0:
        e = c * (2.0 * float(np.float32(value)) - 1.0)
    else:
        single = jacoby and ((c0 == 1) if bug == "jacoby by the starting cube" else (n == 0))
        e = float(c) * float((1 if points > 0 else -1) if single else points)
    return c, o, dropped, passed, n, e


def _test_set():
    """(turns, points, value, rule, start value, start owner): every mean a few ulps and a little away from each threshold on both
    sides, both movers, every owner, two start cubes, every ending -- and the reference's own trials of the GPU cases"""
    rules = [CM.Rule(), CM.Rule(0.6, 0.7, 0.9, 4), CM.Rule(0.5, 0.5, 1.0, 8, True), CM.Rule(0.6, 0.75, 0.95, 2, True, True),
             CC.RULE, CC.RULE_TIGHT, CC.RULE_JACOBY]
    out = []
    rng = np.random.RandomState(11)
    for rule in rules:
        marks = sorted({0.0, 1.0, 0.3, 0.5} | {float(np.nextafter(t, d)) for t in rule[:3] for d in (0.0, 1.0)} | set(rule[:3])
                       | {t + s for t in rule[:3] for s in (-0.04, 0.04) if 0.0 <= t + s <= 1.0})
        for _ in range(160):
            n = int(rng.randint(1, 7))
            first = int(rng.randint(2))
            turns = []
            for k in range(n):
                mover = (first + k) % 2
                w = marks[int(rng.randint(len(marks)))]
                turns.append((mover, w if mover == 0 else 1.0 - w, False))
            points = int(rng.choice([0, 1, 2, 3, -1, -2, -3]))
            value = float(np.float32(rng.rand()))
            out.append((turns, points, value, rule, int(rng.choice([1, 2, 4])), int(rng.randint(3))))
    for (rotate, T), (_, rule, table) in itertools.product(CC.SHAPES, CC.CONFIGS):
        values, owners = CC.TABLES[table]
        for p, row in enumerate(CC.reference(rotate, T, CC.HORIZON)):
            out += [(turns, points, value, rule, values[p], owners[p]) for turns, points, value, _ in row]
    return out


@pytest.fixture(scope="module")
def test_set():
    return _test_set()


def _model(case):
    turns, points, value, rule, c0, o0 = case
    rec, e = CM.trial(turns, points, value, rule, c0, o0)
    return (rec.cube, rec.owner, rec.dropped, rec.passed, rec.doubles, e)


def test_model_against_the_restatement(test_set):
    assert len(test_set) > 1000
    for case in test_set:
        turns, points, value, rule, c0, o0 = case
        assert _model(case) == restated(turns, points, value, *rule, c0, o0), case


def test_exact_thresholds():
    """at the thresholds themselves: w == double_at doubles, w == pass_at is a take, w == too_good_at doubles; one ulp beyond does not"""
    r = CM.Rule(0.6, 0.7, 0.9, 64)
    up, down = (lambda x: float(np.nextafter(x, 1.0))), (lambda x: float(np.nextafter(x, 0.0)))
    play = lambda w, mover=0: CM.play([(mover, w if mover == 0 else 1.0 - w, False)], r)
    assert play(0.6).doubles == 1 and play(down(0.6)).doubles == 0 and play(down(0.6)).dropped == -1
    assert play(0.7).doubles == 1 and play(up(0.7)).dropped == 0 and play(up(0.7)).passed == 2
    assert play(0.9).dropped == 0 and play(up(0.9)).dropped == -1 and play(up(0.9)).doubles == 0
    assert play(0.75, mover=1).passed == 1 and play(0.65, mover=1).owner == 1
    # the cube's value at the drop is the one before the double; a take doubles it and hands it over
    rec, e = CM.trial([(0, 0.65, False), (1, 0.35, False)], 0, 0.5, r, 2, 1)
    assert (rec.cube, rec.owner, rec.dropped, rec.doubles) == (8, 1, -1, 2) and e == 0.0
    rec, e = CM.trial([(0, 0.65, False), (1, 0.2, False)], -3, 0.0, CM.Rule(0.6, 0.7, 0.9, 4), 2, 1)
    assert (rec.cube, rec.owner, rec.dropped, rec.passed) == (4, 2, -1, 0) and e == -12.0      # max_cube reached: PLAYER2 cannot redouble
    rec, e = CM.trial([(1, 0.2, False)], 3, 1.0, r, 2, 2)
    assert rec.dropped == 0 and rec.passed == 1 and e == -2.0


# ---- (2) wrong models -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bug", ["offer without access", ">= at pass_at", "drop pays 2c", "jacoby by the starting cube"])
def test_wrong_models_are_told_apart(test_set, bug):
    differing = 0
    for case in test_set:
        turns, points, value, rule, c0, o0 = case
        differing += _model(case) != restated(turns, points, value, *rule, c0, o0, bug=bug)
    assert differing > 0, bug


def test_statistics_order():
    """the wave's order against exactly rounded sums, and that it is an order: T past one stride, partial strides"""
    import math
    rng = np.random.RandomState(3)
    for T in (1, 36, 40, 64, 65, 200):
        eq = [float(x) for x in rng.choice([-4.0, -2.0, -1.0, 1.0, 2.0, 0.37, -0.81], T)]
        m, se = CM.statistics(eq)
        assert abs(m - math.fsum(eq) / T) <= T * 2.0 ** -50
        want = math.sqrt(math.fsum((e - math.fsum(eq) / T) ** 2 for e in eq) / (T * (T - 1))) if T > 1 else 0.0
        assert abs(se - want) <= 1e-12 * want + T * 2.0 ** -50
        dm, ds = CM.paired(eq, eq)
        assert dm == 0.0 and ds == 0.0


# ---- (3) the conditions the GPU tests rest on ----------------------------------------------------------------------------------------------

def test_every_class_occurs_under_the_reference():
    """... and still does when the means move by the value tolerance, each on its own: with tol, a trial counts for a class only if it
    belongs to it under every combination of its means moved by -tol, 0, +tol"""
    trials_of = lambda rotate, T: CC.reference(rotate, T, CC.HORIZON)
    for tol in (0.0, CC.MEAN_TOL):
        got = CC.full_census(trials_of, tol)
        print("tol %.0e:" % tol, got)
        for c in CC.CLASSES:
            assert got.get(c, 0) >= 1, (c, tol, got)


def test_positions_are_what_they_are_called():
    st, tu = CC.positions()
    for rotate, T in CC.SHAPES:
        contact, bear, over = CC.reference(rotate, T, CC.HORIZON)
        assert all(t[3] and len(t[0]) == CC.HORIZON for t in contact)                       # contact: every trial is cut at the horizon
        assert all(not t[3] and 1 <= len(t[0]) < CC.HORIZON and t[1] in (-1, -2) for t in bear)
        assert {t[1] for t in bear} == {-1, -2}                                             # gammons (a doubles roll at turn 0) and single games
        assert all(t[0][0][2] and t[1] == -2 for t in over)
    assert (st[0][:24] > 0).any() and np.where(st[0][:24] > 0)[0].min() < np.where(st[0][:24] < 0)[0].max()


def test_start_at_max_cube_is_the_cubeless_equity_times_the_cube():
    values, owners = CC.TABLES["at max"]
    for rotate, T in CC.SHAPES:
        for p, row in enumerate(CC.reference(rotate, T, CC.HORIZON)):
            for turns, points, value, _ in row:
                rec, e = CM.trial(turns, points, value, CC.RULE, values[p], owners[p])
                cubeless = float(points) if points else 2.0 * float(np.float32(value)) - 1.0
                assert rec == CM.start(values[p], owners[p]) and e == 4.0 * cubeless


# ---- (4) plumbing ------------------------------------------------------------------------------------------------------------------------

NEW = ("bgamd_env_rollout_cube", "bgamd_env_rollout_cube_read", "bgamd_env_rollout_cube_info")


def test_cube_entry_points_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from backgammon_env import _capi
    src = open(os.path.join(ROOT, "include", "bgamd.h")).read()
    assert re.search(r"\bBGAMD_CUBE_ON\s*=\s*1\b", src) and re.search(r"\bBGAMD_CUBE_JACOBY\s*=\s*2\b", src)
    hdr = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in {n for n, _, _ in _capi.SYMBOLS}, name
    assert (_capi.CUBE_ON, _capi.CUBE_JACOBY) == (1, 2)
    # host-side argument checks need no device
    assert lib.bgamd_env_rollout_cube(None, 1, ctypes.c_double(0.7), ctypes.c_double(0.78), ctypes.c_double(1.0), ctypes.c_int64(64), None, None) == -1
    assert lib.bgamd_env_rollout_cube_info(None, None) == -1


def test_python_surface_accepts_the_cube():
    import backgammon_env as bg
    from backgammon_env import analysis
    assert "cube" in inspect.signature(bg.VecGame.rollout).parameters
    assert bg.VecGame.PAIRED_WHICH["cubeful"] == 3
    c = bg.Cube()
    assert (c.double_at, c.pass_at, c.too_good_at, c.max_cube, c.jacoby) == (0.70, 0.78, 1.0, 64, False)
    assert callable(analysis.cube_action)
    # GNU Backgammon's table on (nd, dt, dp)
    assert analysis.cube_decision(0.3, 0.5, 1.0) == "double, take"
    assert analysis.cube_decision(0.5, 0.3, 1.0) == "no double, take"
    assert analysis.cube_decision(0.9, 1.4, 1.0) == "double, pass"
    assert analysis.cube_decision(1.2, 1.4, 1.0) == "too good, pass"
    assert analysis.cube_decision(1.2, 0.9, 1.0) == "too good, take"
    assert set(analysis.CUBE_ACTIONS) == {"no double, take", "double, take", "double, pass", "too good, pass", "too good, take"}
