"""The doubling cube on the rollout's trials on the MI355X (bgamd_env_rollout_cube, VecGame.rollout(cube=...)):
  (1) replay: every trial's cube history bit for bit against tests/cube_model.py fed with the device's own pre-roll means -- lane j of
      a VecGame plays game id j, evaluate_preroll before every turn --, played by the greedy step and by the 2-ply search; the
      statistics against the fixed reduction order;
  (2) the classes of cube history tests/test_cube_model_cpu.py finds under the fp64 reference occur on the device too;
  (3) overlay: everything the rollout returned before is bit-identical with and without the cube;
  (4) independence of lanes, call order, position_offset splits and grouping;
  (5) start tables, Jacoby, the paired read's which = 3, error codes;
  (6) analysis.cube_action end to end, and the example in a child process.
The thresholds are those of tests/cube_cases.py (not the header's suggested defaults: see there)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import cube_cases as CC
import cube_model as CM

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PLAIN = ("mean", "stderr", "turns", "truncated", "trial_value", "trial_turns", "vr_mean", "vr_stderr", "trial_luck", "counts", "equity",
         "equity_stderr", "trial_points")
CUBE = ("cubeful", "cubeful_stderr", "cube_counts", "trial_cubeful", "trial_cube", "trial_dropped")
TOP_K, MARGIN = 2, 0.04


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


@pytest.fixture(scope="module")
def env(bg, weights):
    e = bg.VecGame(64, seed=7)
    e.load_weights(weights)
    yield e
    e.close()


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _same(a, b, keys=None):
    for k in keys or a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _cube(bg, rule, table="centre", P=3):
    values, owners = CC.TABLES[table]
    return bg.Cube(rule.double_at, rule.pass_at, rule.too_good_at, rule.max_cube, rule.jacoby, rule.hold_turn0, values[:P], owners[:P])


def _args(rotate, M, **kw):
    return dict(max_plies=M, rotate=rotate, seed=CC.SEED, lanes=CC.LANES, per_trial=True, variance_reduction=True, outcomes=True, **kw)


# ---- the replay ----------------------------------------------------------------------------------------------------------------------------

_REPLAYS = {}


def _replay_position(bg, weights, state, turn, T, lane_offset, rotate, M, plies):
    """-> [T] of (turns [(mover, mean, over)], points, value, truncated): cube_cases.ref_trial's tuple from the device"""
    if state[26] == 15 or state[27] == 15:
        pts = int(bg.outcomes(state[None]).cpu().numpy()[0])
        x = 1.0 if state[26] == 15 else 0.0
        return [([(int(turn), x, True)], pts, x, False) for _ in range(T)]
    e = bg.VecGame(T, seed=CC.SEED, lane_offset=lane_offset)
    e.load_weights(weights)
    e.set_states(np.tile(state, (T, 1)), np.full(T, turn))
    ar = np.arange(T)
    first = np.stack([1 + (ar % 36) // 6, 1 + (ar % 36) % 6], 1).astype(np.int32)
    seqs = [[] for _ in range(T)]
    k = 0
    while M == 0 or k < M:
        live = (e.flags().cpu().numpy() & 4) == 0
        if not live.any():
            break
        tu = e.turns()
        _, mean = e.evaluate_preroll(e.states(), tu)
        tu, mean = tu.cpu().numpy(), mean.cpu().numpy()
        for i in np.flatnonzero(live):
            seqs[i].append((int(tu[i]), float(mean[i]), False))
        roll = not (k == 0 and rotate)
        if not roll:
            e.set_dice(first)
        if plies == 2:
            e.step_search(top_k=TOP_K, roll=roll, auto_reset=False, margin=MARGIN)
        else:
            e.step_greedy(roll=roll, auto_reset=False)
        k += 1
    frozen = (e.flags().cpu().numpy() & 4) != 0
    value = np.where((e.flags().cpu().numpy() >> 1) & 1, 0.0, 1.0).astype(np.float32)
    if (~frozen).any():
        value = np.where(frozen, value, e.evaluate(e.states(), e.turns()).cpu().numpy()).astype(np.float32)
    points = np.where(frozen, e.outcomes().cpu().numpy(), 0)
    assert e.stats()["error_flags"] == 0
    e.close()
    return [(seqs[i], int(points[i]), float(value[i]), not frozen[i]) for i in range(T)]


def _replay(bg, weights, rotate, T, M, plies=1):
    key = (rotate, T, M, plies)
    if key not in _REPLAYS:
        st, tu = CC.positions()
        _REPLAYS[key] = [_replay_position(bg, weights, st[p], int(tu[p]), T, (CC.OFFSET + p) * T, rotate, M, plies) for p in range(len(st))]
    return _REPLAYS[key]


def _expect(trials, rule, values, owners):
    """the model on the replayed trials -> dict of the cube outputs"""
    P, T = len(trials), len(trials[0])
    out = {"trial_cubeful": np.zeros((P, T)), "trial_cube": np.zeros((P, T), np.int32), "trial_dropped": np.zeros((P, T), np.int32),
           "cube_counts": np.zeros((P, 4), np.int64), "cubeful": np.zeros(P), "cubeful_stderr": np.zeros(P)}
    for p in range(P):
        recs = []
        for i, (turns, points, value, _) in enumerate(trials[p]):
            rec, e = CM.trial(turns, points, value, rule, values[p], owners[p])
            recs.append(rec)
            out["trial_cubeful"][p, i], out["trial_cube"][p, i], out["trial_dropped"][p, i] = e, rec.cube, rec.dropped
        out["cube_counts"][p] = CM.counts(recs, rule)
        out["cubeful"][p], out["cubeful_stderr"][p] = CM.statistics(out["trial_cubeful"][p])
    return out


def _check(r, want, trials):
    np.testing.assert_array_equal(r["trial_value"], np.array([[t[2] for t in row] for row in trials], np.float32))
    np.testing.assert_array_equal(r["trial_points"], np.array([[t[1] for t in row] for row in trials]))
    for k in ("trial_dropped", "trial_cube", "trial_cubeful", "cube_counts", "cubeful"):
        np.testing.assert_array_equal(r[k], want[k], err_msg=k)
    # the standard error as the plain statistics' is compared (tests/test_gpu_rollout.py): the sum of squares is exact, the square root
    # and the two divisions are the device's
    np.testing.assert_allclose(r["cubeful_stderr"], want["cubeful_stderr"], rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("M", [4, 0])
@pytest.mark.parametrize("rotate,T", CC.SHAPES)
def test_trials_against_the_model_on_the_devices_own_means(bg, weights, env, rotate, T, M):
    st, tu = CC.positions()
    trials = _replay(bg, weights, rotate, T, M)
    for name, rule, table in CC.CONFIGS + [("at max", CC.RULE, "at max")]:
        values, owners = CC.TABLES[table]
        r = _np(env.rollout(st, tu, T, position_offset=CC.OFFSET, cube=_cube(bg, rule, table), **_args(rotate, M)))
        _check(r, _expect(trials, rule, values, owners), trials)
        played, after = env.rollout_cube_info()
        assert played == int(r["trial_turns"].sum()) - (r["trial_turns"] > 0).sum() * (1 if rotate else 0)
        want_after = sum(len(t[0]) - max(CM.play(t[0], rule, values[p], owners[p]).dropped, 1 if rotate else 0)
                         for p, row in enumerate(trials) for t in row if CM.play(t[0], rule, values[p], owners[p]).dropped >= 0)
        assert after == want_after, name
    assert (r["trial_turns"][0] == 4).all() if M else (r["truncated"] == 0).all()


def test_trials_played_by_the_two_ply_search(bg, weights, env):
    st, tu = CC.positions()
    rotate, T, M = True, 36, 4
    trials = _replay(bg, weights, rotate, T, M, plies=2)
    for _, rule, table in CC.CONFIGS[:3]:
        values, owners = CC.TABLES[table]
        r = _np(env.rollout(st, tu, T, position_offset=CC.OFFSET, cube=_cube(bg, rule, table), plies=2, top_k=TOP_K, margin=MARGIN,
                            **_args(rotate, M)))
        assert env.rollout_info()[3] == 1
        _check(r, _expect(trials, rule, values, owners), trials)
    # a hold at turn 0: the roller's double of the "take" call is not made
    hold = CC.RULE._replace(hold_turn0=True)
    r = _np(env.rollout(st, tu, T, position_offset=CC.OFFSET, cube=_cube(bg, hold), plies=2, top_k=TOP_K, margin=MARGIN, **_args(rotate, M)))
    _check(r, _expect(trials, hold, *CC.TABLES["centre"]), trials)
    assert (r["trial_dropped"] != 0).all()


# ---- (2) the classes on the device ---------------------------------------------------------------------------------------------------------

def test_every_class_occurs_on_the_device(bg, weights, env):
    got = CC.full_census(lambda rotate, T: _replay(bg, weights, rotate, T, CC.HORIZON))
    print(got)
    for c in CC.CLASSES:
        assert got.get(c, 0) >= 1, (c, got)
    # ... and in the device's own outputs, not only in the model's reading of its means
    st, tu = CC.positions()
    rotate, T = CC.SHAPES[0]
    take = _np(env.rollout(st, tu, T, position_offset=CC.OFFSET, cube=_cube(bg, CC.RULE), **_args(rotate, CC.HORIZON)))
    assert (take["trial_cube"][0] == 2).any() and (take["trial_cube"][0] == 4).any()              # double / take; redouble to max_cube
    assert take["cube_counts"][0].tolist() == [0, 0, int((take["trial_cube"][0] == 2).sum() + 2 * (take["trial_cube"][0] == 4).sum()),
                                               int((take["trial_cube"][0] == 4).sum())]
    assert (take["trial_dropped"][1] == 0).all() and take["cube_counts"][1].tolist() == [T, 0, 0, 0]      # PLAYER1 passes at the rotated turn 0
    assert (take["trial_cubeful"][1] == -1.0).all()
    assert (take["trial_cube"][2] == 1).all() and (take["trial_cubeful"][2] == -2.0).all()         # over: never doubled, a gammon
    tight = _np(env.rollout(st, tu, T, position_offset=CC.OFFSET, cube=_cube(bg, CC.RULE_TIGHT), **_args(rotate, CC.HORIZON)))
    assert tight["cube_counts"][0].tolist() == [0, T, 0, 0] and (tight["trial_cubeful"][0] == 1.0).all()   # PLAYER2 passes at turn 0
    na = _np(env.rollout(st, tu, T, position_offset=CC.OFFSET, cube=_cube(bg, CC.RULE_TIGHT, "no access"), **_args(rotate, CC.HORIZON)))
    assert (na["trial_dropped"][0] != 0).all() and na["cube_counts"][0][0] > 0                    # the contact position's roller must hold; PLAYER2's doubles at turn 1
    assert (na["trial_dropped"][1] == -1).all() and (na["trial_cube"][1] == 1).all()              # the bear-off's roller never has access


# ---- (3) overlay ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rotate,T", CC.SHAPES)
def test_the_cube_changes_nothing_else(bg, weights, env, rotate, T):
    st, tu = CC.positions()
    st, tu = np.concatenate([st, st[:1]]), np.concatenate([tu, tu[:1]])
    groups, ref = [2, 0, 2, 2], [3, 1, 0, 0]
    args = _args(rotate, CC.HORIZON, groups=groups, group_offset=1)
    a = _np(env.rollout(st, tu, T, **args))
    ia = env.rollout_info()
    pa = [[x.cpu().numpy() for x in env.rollout_paired(ref, w)] for w in ("value", "vr", "equity")]
    b = _np(env.rollout(st, tu, T, cube=bg.Cube(CC.RULE.double_at, CC.RULE.pass_at, 1.0, 4, value=[1, 2, 1, 4], owner=[0, 1, 0, 2]), **args))
    assert env.rollout_info() == ia
    pb = [[x.cpu().numpy() for x in env.rollout_paired(ref, w)] for w in ("value", "vr", "equity")]
    assert set(a) == set(PLAIN) and set(b) == set(PLAIN) | set(CUBE)
    _same(a, b, PLAIN)
    for x, y in zip(pa, pb):
        np.testing.assert_array_equal(x[0], y[0])
        np.testing.assert_array_equal(x[1], y[1])
    assert b["cube_counts"][:, 2].sum() > 0                                        # (the cube was there)


def test_an_env_that_cleared_the_cube_is_one_that_never_set_it(bg, weights):
    from backgammon_env import _capi
    st, tu = CC.positions()
    out = []
    for setter in (False, True):
        e = bg.VecGame(64, seed=7)
        e.load_weights(weights)
        if setter:
            e.rollout(st, tu, 36, cube=_cube(bg, CC.RULE), **_args(True, 2))         # a cubeful rollout first: rollout() clears the setting
            _capi.check(e._lib.bgamd_env_rollout_cube(e._h, _capi.CUBE_ON | _capi.CUBE_JACOBY, 0.6, 0.7, 0.9, 8, None, None), "rollout_cube")
            _capi.check(e._lib.bgamd_env_rollout_cube(e._h, 0, 0.0, 0.0, 0.0, 0, None, None), "rollout_cube")
        out.append((_np(e.rollout(st, tu, 72, max_plies=9, rotate=True, seed=CC.SEED, per_trial=True, variance_reduction=True, outcomes=True)),
                    _np(e.rollout(st, tu, 40, max_plies=3, rotate=False, seed=CC.SEED, per_trial=True)), e.rollout_info()))
        with pytest.raises(bg.BgamdError, match="-1"):                               # the last rollout had no cube
            e.rollout_cube_read()
        e.close()
    _same(out[0][0], out[1][0])
    _same(out[0][1], out[1][1])
    assert out[0][2] == out[1][2]


# ---- (4) independence ----------------------------------------------------------------------------------------------------------------------

def test_independence_of_lanes_calls_offsets_and_groups(bg, env):
    st, tu = CC.positions()
    st, tu = np.concatenate([st, st[:1]]), np.concatenate([tu, tu[:1]])
    P, T = 4, 144
    cube = bg.Cube(CC.RULE.double_at, CC.RULE.pass_at, 1.0, 4, value=[1, 2, 1, 1], owner=[0, 2, 0, 0])
    args = dict(max_plies=5, rotate=True, seed=CC.SEED, per_trial=True, variance_reduction=True, outcomes=True)
    base = _np(env.rollout(st, tu, T, cube=cube, **args))
    info = env.rollout_cube_info()
    assert env.rollout_info()[0] == 768
    for lanes in (256, 512):
        _same(base, _np(env.rollout(st, tu, T, lanes=lanes, cube=cube, **args)))
        assert env.rollout_info()[0] == lanes and env.rollout_cube_info() == info
    _same(base, _np(env.rollout(st, tu, T, cube=cube, **args)))
    half = lambda lo, hi: bg.Cube(cube.double_at, cube.pass_at, 1.0, 4, value=cube.value[lo:hi], owner=cube.owner[lo:hi])
    a = _np(env.rollout(st[:2], tu[:2], T, position_offset=0, cube=half(0, 2), **args))
    b = _np(env.rollout(st[2:], tu[2:], T, position_offset=2, cube=half(2, 4), **args))
    _same(base, {k: np.concatenate([a[k], b[k]]) for k in base})
    assert not np.array_equal(base["trial_cubeful"][0], base["trial_cubeful"][3])  # the same position under other trial ids: other dice
    # grouped against single-position calls
    groups = [4, 1, 4, 1]
    g = _np(env.rollout(st, tu, T, groups=groups, group_offset=2, cube=cube, **args))
    for p in range(P):
        one = _np(env.rollout(st[p:p + 1], tu[p:p + 1], T, position_offset=2 + groups[p], cube=half(p, p + 1), **args))
        _same({k: g[k][p:p + 1] for k in g}, one)


# ---- (5) start tables, Jacoby, the paired read, errors -------------------------------------------------------------------------------------

@pytest.mark.parametrize("rotate,T", CC.SHAPES)
def test_start_tables(bg, env, rotate, T):
    st, tu = CC.positions()
    r = _np(env.rollout(st, tu, T, cube=_cube(bg, CC.RULE, "at max"), **_args(rotate, CC.HORIZON)))
    # max_cube equal to the start value: no decision is ever made, and the cubeful equity is the cube times the cubeless one, exactly
    eq = np.where(r["trial_points"] != 0, r["trial_points"].astype(np.float64), 2.0 * r["trial_value"].astype(np.float64) - 1.0)
    np.testing.assert_array_equal(r["trial_cubeful"], 4.0 * eq)
    assert (r["trial_cube"] == 4).all() and (r["trial_dropped"] == -1).all()
    np.testing.assert_array_equal(r["cube_counts"], np.tile([0, 0, 0, T], (3, 1)))
    # a cube of 2 owned by PLAYER1 (contact: its roller doubles at turn 0 to 4 = max_cube), by PLAYER2 (bear-off: its roller doubles,
    # PLAYER1 passes and loses 2), centred (over: no decision)
    r = _np(env.rollout(st, tu, T, cube=_cube(bg, CC.RULE, "owned"), **_args(rotate, CC.HORIZON)))
    assert (r["trial_cube"][0] == 4).all() and r["cube_counts"][0].tolist() == [0, 0, T, T]
    assert (r["trial_cubeful"][1] == -2.0).all() and (r["trial_dropped"][1] == 0).all() and (r["trial_cube"][1] == 2).all()
    assert (r["trial_cubeful"][2] == -4.0).all()
    # the same cube in the other side's hands: the rollers must hold
    swapped = bg.Cube(CC.RULE.double_at, CC.RULE.pass_at, 1.0, 4, value=[2, 2, 2], owner=[2, 1, 0])
    r = _np(env.rollout(st, tu, T, cube=swapped, **_args(rotate, CC.HORIZON)))
    assert (r["trial_dropped"] != 0).all()


@pytest.mark.parametrize("rotate,T", CC.SHAPES)
def test_jacoby(bg, env, rotate, T):
    st, tu = CC.positions()
    off = CC.RULE_JACOBY._replace(jacoby=False)
    for table in ("centre", "owned"):
        a = _np(env.rollout(st, tu, T, cube=_cube(bg, CC.RULE_JACOBY, table), **_args(rotate, 0 if table == "owned" else CC.HORIZON)))
        b = _np(env.rollout(st, tu, T, cube=_cube(bg, off, table), **_args(rotate, 0 if table == "owned" else CC.HORIZON)))
        _same(a, b, PLAIN + ("trial_cube", "trial_dropped", "cube_counts"))
        start = np.array(CC.TABLES[table][0])[:, None]
        undoubled_gammon = (a["trial_dropped"] < 0) & (a["trial_cube"] == start) & (np.abs(a["trial_points"]) >= 2)
        if table == "centre":
            assert undoubled_gammon[1].any() and not undoubled_gammon[1].all() and undoubled_gammon[2].all()
        differ = a["trial_cubeful"] != b["trial_cubeful"]
        # under "owned" a trial's cube equals the start value only if it was never turned (it only grows)
        np.testing.assert_array_equal(differ, undoubled_gammon)
        np.testing.assert_array_equal(a["trial_cubeful"][differ], (a["trial_cube"] * np.sign(a["trial_points"]))[differ].astype(np.float64))
        np.testing.assert_array_equal(b["trial_cubeful"][differ], (b["trial_cube"] * b["trial_points"].astype(np.int64))[differ].astype(np.float64))


def test_paired_read_of_the_cubeful_equity(bg, env):
    st, tu = CC.positions()
    st, tu = st[[0, 0, 1, 0]], tu[[0, 0, 1, 0]]
    groups, ref = [5, 5, 6, 5], [1, 0, 0, 7]
    T = 73
    # the contact position twice on the same dice: a 2-cube in PLAYER2's hands (it may redouble at turn 1) against one in PLAYER1's (its
    # roller redoubles at turn 0, to max_cube): the trials in which PLAYER2 does not redouble are truncated under cubes of 2 and of 4
    cube = bg.Cube(CC.RULE.double_at, CC.RULE.pass_at, 1.0, 4, value=[2, 2, 1, 1], owner=[2, 1, 0, 0])
    r = _np(env.rollout(st, tu, T, groups=groups, cube=cube, max_plies=4, rotate=True, seed=CC.SEED, per_trial=True, variance_reduction=True))
    dm, ds = (x.cpu().numpy() for x in env.rollout_paired(ref, "cubeful"))
    q = r["trial_cubeful"]
    for p in (0, 1):
        m, se = CM.paired(q[p], q[ref[p]])
        assert dm[p] == m and math.isclose(ds[p], se, rel_tol=1e-12)
    assert dm[0] == -dm[1] and dm[0] != 0.0 and ds[0] > 0.0
    assert np.isnan(dm[2]) and np.isnan(ds[2]) and np.isnan(dm[3]) and np.isnan(ds[3])       # another group; out of range
    same, zero = (x.cpu().numpy() for x in env.rollout_paired([0, 1, 2, 3], "cubeful"))
    assert (same == 0.0).all() and (zero == 0.0).all()
    env.rollout(st, tu, T, groups=groups, max_plies=4, rotate=True, seed=CC.SEED, variance_reduction=True)
    with pytest.raises(bg.BgamdError, match="-1"):
        env.rollout_paired(ref, "cubeful")
    env.rollout_paired(ref, "vr")


def test_error_codes(bg, weights):
    from backgammon_env import _capi
    st, tu = CC.positions()
    e = bg.VecGame(64, seed=1)
    e.load_weights(weights)
    lib = e._lib
    good = _np(e.rollout(st, tu, 36, cube=_cube(bg, CC.RULE), **_args(True, 4)))
    info, cinfo = e.rollout_info(), e.rollout_cube_info()

    def setter(flags=1, d=0.7, p=0.78, t=1.0, m=64):
        return lib.bgamd_env_rollout_cube(e._h, flags, d, p, t, m, None, None)
    nan = float("nan")
    for kw in (dict(d=nan), dict(p=nan), dict(t=nan), dict(d=-0.1), dict(p=1.1), dict(t=1.5), dict(d=0.9, t=0.8), dict(m=0), dict(m=3),
               dict(m=-4), dict(m=2 ** 31), dict(m=96), dict(flags=8), dict(flags=2), dict(flags=9)):
        assert setter(**kw) == -1, kw
    assert lib.bgamd_env_rollout_cube(None, 1, 0.7, 0.78, 1.0, 64, None, None) == -1
    assert setter(d=0.0, p=0.0, t=0.0, m=1) == 0 and setter(d=1.0, p=1.0, t=1.0, m=2 ** 30) == 0 and setter(flags=0, d=nan, m=-1) == 0
    # the cube on without the luck pass: refused before anything is played, by the C ABI and by the Python surface
    assert setter() == 0
    with pytest.raises(bg.BgamdError, match="-1"):
        e.rollout(st, tu, 36, max_plies=4, seed=CC.SEED)
    assert setter(flags=0) == 0
    with pytest.raises(ValueError):
        e.rollout(st, tu, 36, max_plies=4, seed=CC.SEED, cube=_cube(bg, CC.RULE))
    with pytest.raises(bg.BgamdError, match="-1"):           # bad thresholds through the Python surface; the setting stays off
        e.rollout(st, tu, 36, cube=bg.Cube(double_at=0.9, too_good_at=0.8), **_args(True, 4))
    # a bad table entry: refused with the bad states, before anything is played
    for value, owner in (([1, 3, 1], None), ([1, 0, 1], None), ([1, 1, -2], None), (None, [0, 3, 0]), (None, [-1, 0, 0]), ([2 ** 30, 1, 2 ** 30 + 1], None)):
        with pytest.raises(bg.BgamdError, match="-1"):
            e.rollout(st, tu, 36, cube=bg.Cube(value=value, owner=owner), **_args(True, 4))
        with pytest.raises(bg.BgamdError, match="-1"):
            e.rollout_cube_read()
    e.rollout(st, tu, 36, cube=bg.Cube(value=[2 ** 30, 1, 2], owner=[2, 1, 0], max_cube=2 ** 30), **_args(True, 4))
    bad = st.copy()
    bad[0, 3] = 16
    with pytest.raises(bg.BgamdError, match="-5"):
        e.rollout(bad, tu, 36, cube=_cube(bg, CC.RULE), **_args(True, 4))
    # ... and the env is as good as before
    again = _np(e.rollout(st, tu, 36, cube=_cube(bg, CC.RULE), **_args(True, 4)))
    _same(good, again)
    assert e.rollout_info() == info and e.rollout_cube_info() == cinfo
    e.close()


# ---- (6) analysis.cube_action --------------------------------------------------------------------------------------------------------------

def test_cube_action_end_to_end(bg, weights, env):
    import nets as N
    from backgammon_env import analysis
    from backgammon_env.analysis import cube_action
    cst, ctu = CC.positions()
    b_st, b_tu = N._bearoffs()
    # PLAYER2 to roll bears its last two checkers off with any roll, PLAYER1 has borne off 14: a certain single game
    st = np.stack([b_st[2], cst[2], cst[0], cst[0]]).astype(np.int32)
    tu = np.array([b_tu[2], 0, 0, 0], np.int32)
    value, owner = [1, 2, 2, 1], [0, 0, 2, 0]
    T, M, off = 72, 6, 3
    res = cube_action(env, st, tu, cube_value=value, cube_owner=owner, trials=T, max_plies=M, seed=CC.SEED, group_offset=off)
    info = env.rollout_cube_info()
    assert [r["action"] for r in res[:3]] == ["double, pass", "game over", "no access"]
    # (the roller cannot win a gammon -- PLAYER1 has borne off 14 --, so not doubling is worth at most the cube; doubled, it wins two points
    # more often than three times in four)
    assert res[0]["nd"] <= 1.0 and res[0]["dt"] > 1.0 and res[0]["dp"] == 1.0 and res[0]["diff"] > 0.0
    assert res[0]["cubeless"] > 0.5 and res[0]["shares"]["win"] > 0.75 and res[0]["shares"]["win_gammon"] == 0.0
    assert res[1]["nd"] == -4.0 and "dt" not in res[1] and "dt" not in res[2]
    assert res[3]["action"] in analysis.CUBE_ACTIONS and res[3]["dp"] == 1.0
    # nd and dt are the two single rollouts, bit for bit; dt - nd is the paired read
    rule = bg.Cube()
    for p in (0, 3):
        sg = 1.0 if tu[p] == 0 else -1.0
        kw = dict(max_plies=M, rotate=True, seed=CC.SEED, position_offset=off + p, variance_reduction=True, per_trial=True)
        nd = _np(env.rollout(st[p:p + 1], tu[p:p + 1], T, cube=bg.Cube(hold_turn0=True, value=[value[p]], owner=[owner[p]]), **kw))
        dt = _np(env.rollout(st[p:p + 1], tu[p:p + 1], T, cube=bg.Cube(hold_turn0=True, value=[2 * value[p]], owner=[2 - int(tu[p])]), **kw))
        assert res[p]["nd"] == sg * nd["cubeful"][0] and res[p]["nd_stderr"] == nd["cubeful_stderr"][0]
        assert res[p]["dt"] == sg * dt["cubeful"][0] and res[p]["dt_stderr"] == dt["cubeful_stderr"][0]
        m, se = CM.paired(dt["trial_cubeful"][0], nd["trial_cubeful"][0])
        assert res[p]["diff"] == sg * m and math.isclose(res[p]["diff_stderr"], se, rel_tol=1e-12, abs_tol=0.0)
        assert res[p]["action"] == analysis.cube_decision(res[p]["nd"], res[p]["dt"], res[p]["dp"])
    assert info[0] > 0
    with pytest.raises(ValueError):
        cube_action(env, st, tu, trials=T, cube=bg.Cube(jacoby=True))


def test_the_example_runs():
    # (the child under this process's own site settings: an interpreter started without the user's site-packages stays without them,
    # so that the example can only import the package, and load the library, of this tree)
    site_flags = (["-s"] if sys.flags.no_user_site else []) + (["-E"] if sys.flags.ignore_environment else [])
    r = subprocess.run([sys.executable, *site_flags, os.path.join(ROOT, "examples", "cube_action.py"), "--trials", "72", "--max-plies", "6"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 9 and "game over" in lines[6] and "no access" in lines[3]
    assert any(a in lines[1] for a in ("no double, take", "double, take", "double, pass", "too good, pass", "too good, take"))
    assert lines[8] == "package %s library %s" % (os.path.join(ROOT, "backgammon-engine_amd", "backgammon_env"),
                                                  os.path.join(ROOT, "backgammon-engine_amd", "libbgamd.so")), r.stdout
