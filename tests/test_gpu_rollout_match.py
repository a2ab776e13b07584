"""Match play on the cubeful rollouts on the MI355X (bgamd_env_rollout_match, VecGame.rollout(cube=..., match=...)):
  (1) replay: every trial's history and match-winning chance bit for bit against tests/match_model.py fed with the device's own
      pre-roll means (tests/test_gpu_rollout_cube.py's replay: lane j of a VecGame plays game id j, evaluate_preroll before every
      turn) and the device's own threshold entries, under greedy and 2-ply turns; the statistics against the fixed reduction order;
  (2) the classes of match history tests/test_match_model_cpu.py finds under the fp64 reference occur on the device too;
  (3) overlay: everything the rollout returned before is bit-identical with and without the match; a cleared match is no match;
  (4) independence of lanes, call order, position_offset splits, grouping and of what the env did before;
  (5) the paired read's which = 4, the threshold table, error codes, the intake's bad entries;
  (6) analysis.cube_action(match=...) end to end, and the example in a child process.
The configurations are those of tests/match_cases.py."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import cube_cases as CC
import cube_model as CM
import match_cases as MC
import match_model as MM
from test_gpu_rollout_cube import MARGIN, PLAIN, TOP_K, _args, _np, _replay, _same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CUBE = ("cubeful", "cubeful_stderr", "cube_counts", "trial_cubeful", "trial_cube", "trial_dropped")
MATCH = ("mwc", "mwc_stderr", "match_counts", "trial_mwc")
BY_NAME = {c[0]: c for c in MC.CONFIGS}


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


def _table(bg, tab):
    return bg.MatchTable(tab.met, tab.met_pc)


def _setting(bg, config, rows=slice(None)):
    """-> (Cube, Match) of a configuration of tests/match_cases.py, for the positions `rows`"""
    _, tab, ws, a1, a2, st, values, owners = config
    pick = lambda x: list(np.asarray(x)[rows])
    r = MC.RULE
    return (bg.Cube(r.double_at, r.pass_at, r.too_good_at, r.max_cube, False, r.hold_turn0, pick(values), pick(owners)),
            bg.Match(_table(bg, tab), pick(a1), pick(a2), pick(st), ws))


_THR = {}


def _device_thr(bg, env, config):
    """the threshold function of a configuration from the DEVICE's table: every entry read back once"""
    name, tab, ws = config[:3]
    if name not in _THR:
        one = torch.ones(1, dtype=torch.int32, device=env.device)
        env._set_match(_table(bg, tab), ws, one, one, one)
        _THR[name] = {key: env.rollout_match_thresholds(*key) for key in MM.threshold_table(tab, ws)}
        env._lib.bgamd_env_rollout_match(env._h, 0, 0, None, None, 0.0, None, None, None)
    return lambda s, c, a, b: _THR[name][(s, c, a, b)]


def _expect(trials, config, thr, hold=False):
    """the model on the replayed trials -> dict of the match and cube outputs"""
    P, T = len(trials), len(trials[0])
    tab, sc = config[1], MC.scores(config)
    rule = MC.RULE._replace(hold_turn0=hold)
    out = {"trial_mwc": np.zeros((P, T)), "trial_cube": np.zeros((P, T), np.int32), "trial_dropped": np.zeros((P, T), np.int32),
           "trial_cubeful": np.zeros((P, T)), "match_counts": np.zeros((P, 3), np.int64), "mwc": np.zeros(P), "mwc_stderr": np.zeros(P)}
    for p in range(P):
        res = [MM.trial(tab, turns, points, value, rule, sc[p], thr, config[6][p], config[7][p]) for turns, points, value, _ in trials[p]]
        for i, (played, mwc, _) in enumerate(res):
            out["trial_mwc"][p, i], out["trial_cube"][p, i], out["trial_dropped"][p, i] = mwc, played.rec.cube, played.rec.dropped
            out["trial_cubeful"][p, i] = CM.equity(played.rec, trials[p][i][1], trials[p][i][2], rule)
        out["match_counts"][p] = MM.counts(res)
        out["mwc"][p], out["mwc_stderr"][p] = MM.statistics(out["trial_mwc"][p])
    return out


def _check(r, want, trials):
    np.testing.assert_array_equal(r["trial_value"], np.array([[t[2] for t in row] for row in trials], np.float32))
    np.testing.assert_array_equal(r["trial_points"], np.array([[t[1] for t in row] for row in trials]))
    for k in ("trial_dropped", "trial_cube", "trial_cubeful", "trial_mwc", "match_counts", "mwc"):
        np.testing.assert_array_equal(r[k], want[k], err_msg=k)
    np.testing.assert_allclose(r["mwc_stderr"], want["mwc_stderr"], rtol=1e-12, atol=0.0)


# ---- (1) the replay ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [4, 0])
@pytest.mark.parametrize("rotate,T", CC.SHAPES)
def test_trials_against_the_model_on_the_devices_own_numbers(bg, weights, env, rotate, T, M):
    st, tu = CC.positions()
    trials = _replay(bg, weights, rotate, T, M)
    for config in MC.CONFIGS:
        cube, match = _setting(bg, config)
        r = _np(env.rollout(st, tu, T, position_offset=CC.OFFSET, cube=cube, match=match, **_args(rotate, M)))
        _check(r, _expect(trials, config, _device_thr(bg, env, config)), trials)
    assert (r["trial_turns"][0] == 4).all() if M else (r["truncated"] == 0).all()


@pytest.mark.parametrize("M", [4, 0])
@pytest.mark.parametrize("rotate,T", CC.SHAPES)
def test_trials_played_by_the_two_ply_search(bg, weights, env, rotate, T, M):
    st, tu = CC.positions()
    trials = _replay(bg, weights, rotate, T, M, plies=2)
    for name in ("5-5", "post", "gammon"):
        cube, match = _setting(bg, BY_NAME[name])
        r = _np(env.rollout(st, tu, T, position_offset=CC.OFFSET, cube=cube, match=match, plies=2, top_k=TOP_K, margin=MARGIN, **_args(rotate, M)))
        assert env.rollout_info()[3] == 1
        _check(r, _expect(trials, BY_NAME[name], _device_thr(bg, env, BY_NAME[name])), trials)


@pytest.mark.parametrize("lanes", [1, 2, 65, 256])
def test_any_number_of_lanes_also_fewer_than_positions(bg, weights, env, lanes):
    st, tu = CC.positions()
    rotate, T = CC.SHAPES[0]
    trials = _replay(bg, weights, rotate, T, CC.HORIZON)
    for name in ("5-5", "post 3-1"):
        cube, match = _setting(bg, BY_NAME[name])
        r = _np(env.rollout(st, tu, T, position_offset=CC.OFFSET, cube=cube, match=match, **{**_args(rotate, CC.HORIZON), "lanes": lanes}))
        assert env.rollout_info()[0] == lanes
        _check(r, _expect(trials, BY_NAME[name], _device_thr(bg, env, BY_NAME[name])), trials)


def test_hold_at_turn_0(bg, weights, env):
    st, tu = CC.positions()
    rotate, T = CC.SHAPES[0]
    trials = _replay(bg, weights, rotate, T, CC.HORIZON)
    config = BY_NAME["2-3"]
    cube, match = _setting(bg, config)
    cube.hold_turn0 = True
    r = _np(env.rollout(st, tu, T, position_offset=CC.OFFSET, cube=cube, match=match, **_args(rotate, CC.HORIZON)))
    _check(r, _expect(trials, config, _device_thr(bg, env, config), hold=True), trials)
    assert (r["trial_dropped"] != 0).all()


# ---- (2) the classes on the device ---------------------------------------------------------------------------------------------------------

def test_every_class_occurs_on_the_device(bg, weights, env):
    got = MC.full_census(lambda rotate, T: _replay(bg, weights, rotate, T, CC.HORIZON), thr_of=lambda config: _device_thr(bg, env, config))
    print(got)
    for c in MC.CLASSES:
        assert got.get(c, 0) >= 1, (c, got)
    # ... and in the device's own outputs, not only in the model's reading of its numbers
    st, tu = CC.positions()
    rotate, T = CC.SHAPES[0]
    run = lambda name: _np(env.rollout(st, tu, T, position_offset=CC.OFFSET, **dict(zip(("cube", "match"), _setting(bg, BY_NAME[name]))),
                                       **_args(rotate, CC.HORIZON)))
    craw = run("crawford")
    assert (craw["trial_cube"] == 1).all() and (craw["trial_dropped"] == -1).all() and (craw["match_counts"][:, 2] == 0).all()
    assert (craw["trial_mwc"][2] == MC.J7.met_pc[0]).all()                # over, PLAYER2 won a gammon at 3-away: 1-away / 1-away, post-Crawford
    dmp = run("dmp")
    assert (dmp["trial_cube"] == 1).all() and (dmp["trial_mwc"][2] == 0.0).all() and set(np.unique(dmp["trial_mwc"][1])) <= {0.0, 1.0}
    np.testing.assert_array_equal(dmp["trial_mwc"][0], dmp["trial_value"][0].astype(np.float64))       # truncated: x 1 + (1 - x) 0
    five = run("5-5")
    assert (five["trial_cube"][0] == 2).any() and (five["trial_cube"][0] == 4).any()                      # double / take; redouble
    post = run("post")
    assert (post["match_counts"][0, 2] == T) and (post["trial_dropped"][0] == 1).any() and (post["trial_cube"][0] == 2).any()
    assert (post["trial_cube"][1] == 1).all() and (post["trial_dropped"][1] == -1).all()                  # 3-away: the entry without thresholds
    gam = run("gammon")
    assert (gam["trial_cube"][1] == 2).all() and (gam["trial_mwc"][1][gam["trial_points"][1] == -2] == 0.0).all()
    assert gam["match_counts"][1, 1] == (gam["trial_points"][1] == -2).sum() > 0 and gam["match_counts"][2].tolist() == [0, T, 0]


# ---- (3) overlay ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rotate,T", CC.SHAPES)
def test_the_match_changes_nothing_else(bg, weights, env, rotate, T):
    st, tu = CC.positions()
    st, tu = np.concatenate([st, st[:1]]), np.concatenate([tu, tu[:1]])
    groups, ref = [2, 0, 2, 2], [3, 1, 0, 0]
    args = _args(rotate, CC.HORIZON, groups=groups, group_offset=1)
    cube = bg.Cube(CC.RULE.double_at, CC.RULE.pass_at, 1.0, 4, value=[1, 2, 1, 4], owner=[0, 1, 0, 2])
    a = _np(env.rollout(st, tu, T, cube=cube, **args))
    ia = env.rollout_info()
    pa = [[x.cpu().numpy() for x in env.rollout_paired(ref, w)] for w in ("value", "vr", "equity")]
    b = _np(env.rollout(st, tu, T, cube=cube, match=bg.Match(_table(bg, MC.J7), [5, 3, 5, 6], [5, 5, 2, 6], window_share=0.1), **args))
    assert env.rollout_info() == ia
    pb = [[x.cpu().numpy() for x in env.rollout_paired(ref, w)] for w in ("value", "vr", "equity")]
    assert set(a) == set(PLAIN) | set(CUBE) and set(b) == set(PLAIN) | set(CUBE) | set(MATCH)
    _same(a, b, PLAIN)
    for x, y in zip(pa, pb):
        np.testing.assert_array_equal(x[0], y[0])
        np.testing.assert_array_equal(x[1], y[1])
    assert not (np.array_equal(a["trial_cube"], b["trial_cube"]) and np.array_equal(a["trial_dropped"], b["trial_dropped"]))  # (other thresholds)
    # the cube's own read describes, in points, the records the match rule produced
    eq = np.where(b["trial_dropped"] >= 0, np.nan, b["trial_cube"] * np.where(b["trial_points"] != 0, b["trial_points"].astype(np.float64),
                                                                              2.0 * b["trial_value"].astype(np.float64) - 1.0))
    np.testing.assert_array_equal(b["trial_cubeful"][b["trial_dropped"] < 0], eq[b["trial_dropped"] < 0])
    assert (np.abs(b["trial_cubeful"][b["trial_dropped"] >= 0]) == b["trial_cube"][b["trial_dropped"] >= 0]).all()


def test_an_env_that_cleared_the_match_is_one_that_never_set_it(bg, weights):
    st, tu = CC.positions()
    out = []
    for setter in (False, True):
        e = bg.VecGame(64, seed=7)
        e.load_weights(weights)
        if setter:
            cube, match = _setting(bg, BY_NAME["5-5"])
            e.rollout(st, tu, 36, cube=cube, match=match, **_args(True, 2))        # a rollout under a match first: rollout() clears the setting
            one = torch.ones(3, dtype=torch.int32, device=e.device)
            e._set_match(_table(bg, MC.J1), 0.25, one, one, one)
            assert e._lib.bgamd_env_rollout_match(e._h, 0, 0, None, None, 0.0, None, None, None) == 0
        out.append((_np(e.rollout(st, tu, 72, cube=bg.Cube(0.52, 0.8, 1.0, 4), **{**_args(True, 9), "lanes": 0})),
                    _np(e.rollout(st, tu, 40, max_plies=3, rotate=False, seed=CC.SEED, per_trial=True)), e.rollout_info()))
        with pytest.raises(bg.BgamdError, match="-1"):                             # the last rollout ran under no match
            e.rollout_match_read()
        e.close()
    _same(out[0][0], out[1][0])
    _same(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and (out[0][0]["cube_counts"][:, 2] > 0).any()


# ---- (4) independence ----------------------------------------------------------------------------------------------------------------------

def test_independence_of_lanes_calls_offsets_groups_and_history(bg, weights, env):
    st, tu = CC.positions()
    st, tu = np.concatenate([st, st[:1]]), np.concatenate([tu, tu[:1]])
    P, T = 4, 144
    cube = bg.Cube(1.0, 0.0, 1.0, 4, value=[1, 2, 1, 1], owner=[0, 2, 0, 0])
    a1, a2, ms = [5, 3, 4, 1], [5, 4, 2, 4], [0, 0, 0, 2]
    table = _table(bg, MC.J7)
    match = lambda lo=0, hi=P: bg.Match(table, a1[lo:hi], a2[lo:hi], ms[lo:hi], 0.1)
    half = lambda lo, hi: bg.Cube(1.0, 0.0, 1.0, 4, value=cube.value[lo:hi], owner=cube.owner[lo:hi])
    args = dict(max_plies=5, rotate=True, seed=CC.SEED, per_trial=True, variance_reduction=True, outcomes=True)
    base = _np(env.rollout(st, tu, T, cube=cube, match=match(), **args))
    info = env.rollout_cube_info()
    assert (base["trial_cube"] > np.array(cube.value)[:, None]).any() and (base["trial_dropped"] >= 0).any()
    for lanes in (256, 512):
        _same(base, _np(env.rollout(st, tu, T, lanes=lanes, cube=cube, match=match(), **args)))
        assert env.rollout_info()[0] == lanes and env.rollout_cube_info() == info
    _same(base, _np(env.rollout(st, tu, T, cube=cube, match=match(), **args)))                  # twice on one env ...
    fresh = bg.VecGame(64, seed=3)
    fresh.load_weights(weights)
    _same(base, _np(fresh.rollout(st, tu, T, cube=cube, match=match(), **args)))                # ... as on an env that did nothing before
    fresh.close()
    a = _np(env.rollout(st[:2], tu[:2], T, position_offset=0, cube=half(0, 2), match=match(0, 2), **args))
    b = _np(env.rollout(st[2:], tu[2:], T, position_offset=2, cube=half(2, 4), match=match(2, 4), **args))
    _same(base, {k: np.concatenate([a[k], b[k]]) for k in base})
    assert not np.array_equal(base["trial_value"][0], base["trial_value"][3])                   # the same position under other trial ids
    groups = [4, 1, 4, 1]
    g = _np(env.rollout(st, tu, T, groups=groups, group_offset=2, cube=cube, match=match(), **args))
    for p in range(P):
        one = _np(env.rollout(st[p:p + 1], tu[p:p + 1], T, position_offset=2 + groups[p], cube=half(p, p + 1), match=match(p, p + 1), **args))
        _same({k: g[k][p:p + 1] for k in g}, one)


# ---- (5) the paired read, the table, errors --------------------------------------------------------------------------------------------------

def test_paired_read_of_the_mwc(bg, env):
    st, tu = CC.positions()
    st, tu = st[[0, 0, 1, 0]], tu[[0, 0, 1, 0]]
    groups, ref = [5, 5, 6, 5], [1, 0, 0, 7]
    T = 73
    # the contact position twice on the same dice at 5-away / 5-away: with a centred cube, which its roller turns to 2 at turn 0, and with
    # a 2-cube in the roller's hands, which it turns to 4
    cube = bg.Cube(1.0, 0.0, 1.0, 4, value=[1, 2, 1, 1], owner=[0, 1, 0, 0])
    match = bg.Match(_table(bg, MC.J7), 5, 5, window_share=0.1)
    r = _np(env.rollout(st, tu, T, groups=groups, cube=cube, match=match, max_plies=4, rotate=True, seed=CC.SEED, per_trial=True,
                        variance_reduction=True))
    dm, ds = (x.cpu().numpy() for x in env.rollout_paired(ref, "mwc"))
    q = r["trial_mwc"]
    for p in (0, 1):
        m, se = MM.paired(q[p], q[ref[p]])
        assert dm[p] == m and math.isclose(ds[p], se, rel_tol=1e-12)
    assert dm[0] == -dm[1] and dm[0] != 0.0 and ds[0] > 0.0
    assert np.isnan(dm[2]) and np.isnan(ds[2]) and np.isnan(dm[3]) and np.isnan(ds[3])       # another group; out of range
    same, zero = (x.cpu().numpy() for x in env.rollout_paired([0, 1, 2, 3], "mwc"))
    assert (same == 0.0).all() and (zero == 0.0).all()
    env.rollout_paired(ref, "cubeful")                                                        # the cube's own read is still there
    env.rollout(st, tu, T, groups=groups, cube=cube, max_plies=4, rotate=True, seed=CC.SEED, variance_reduction=True)
    with pytest.raises(bg.BgamdError, match="-1"):
        env.rollout_paired(ref, "mwc")
    env.rollout_paired(ref, "cubeful")


def test_threshold_table_against_the_model(bg, env):
    for config in (BY_NAME["2-2"], BY_NAME["5-5"]):
        tab, ws = config[1], config[2]
        thr = _device_thr(bg, env, config)
        want = MM.threshold_table(tab, ws)
        assert len(want) == 2 * 3 * 49
        for key, v in want.items():
            assert thr(*key) == v, key
    assert any(v[0] == float("inf") for v in want.values()) and any(v[0] < 1.0 for v in want.values())
    # what the table does not hold
    one = torch.ones(1, dtype=torch.int32, device=env.device)
    env._set_match(_table(bg, MC.J7), 0.5, one, one, one)
    for state, c, a, b in ((1, 1, 2, 2), (3, 1, 2, 2), (0, 3, 2, 2), (0, 0, 2, 2), (0, 8, 2, 2), (0, 1, 0, 2), (0, 1, 8, 2), (0, 1, 2, 0), (0, 1, 2, 8)):
        with pytest.raises(bg.BgamdError, match="-1"):
            env.rollout_match_thresholds(state, c, a, b)
    assert env.rollout_match_thresholds(2, 4, 7, 7) == MM.thresholds(MC.J7, 0.5, 2, 4, 7, 7)
    env._set_match(_table(bg, MC.J1), 0.5, one, one, one)                                     # one point: no cube is ever alive, the table is empty
    with pytest.raises(bg.BgamdError, match="-1"):
        env.rollout_match_thresholds(0, 1, 1, 1)
    assert env._lib.bgamd_env_rollout_match(env._h, 0, 0, None, None, 0.0, None, None, None) == 0


def test_error_codes(bg, weights):
    import ctypes
    from backgammon_env import _capi
    st, tu = CC.positions()
    e = bg.VecGame(64, seed=1)
    e.load_weights(weights)
    lib = e._lib
    config = BY_NAME["5-5"]
    cube, match = _setting(bg, config)
    good = _np(e.rollout(st, tu, 36, cube=cube, match=match, **_args(True, 4)))
    info, cinfo = e.rollout_info(), e.rollout_cube_info()
    e.rollout_match_read()
    met, pc = np.full((4, 4), 0.5), np.full(4, 0.5)
    dev = lambda x: torch.tensor(x, dtype=torch.int32, device=e.device)
    a1, a2, ms = dev(config[3]), dev(config[4]), dev(config[5])
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def setter(flags=1, M=4, met=met, pc=pc, ws=0.5, t=(a1, a2, ms)):
        return lib.bgamd_env_rollout_match(e._h, flags, M, None if met is None else ctypes.c_void_p(met.ctypes.data),
                                           None if pc is None else ctypes.c_void_p(pc.ctypes.data), ws, *(None if x is None else ptr(x) for x in t))
    # a setting in force, whose thresholds every refusal must leave in place
    e._set_match(_table(bg, config[1]), config[2], a1, a2, ms)
    held = e.rollout_match_thresholds(0, 1, 5, 5)
    nan, inf = float("nan"), float("inf")
    bad = lambda k, v: np.where(np.arange(16).reshape(4, 4) == k, v, 0.5)
    for kw in (dict(flags=2), dict(flags=3), dict(M=0), dict(M=65), dict(M=-3), dict(met=None), dict(pc=None), dict(met=bad(5, 1.5)),
               dict(met=bad(15, -0.5)), dict(met=bad(0, nan)), dict(met=bad(7, inf)), dict(pc=np.array([0.5, 0.5, 2.0, 0.5])),
               dict(pc=np.array([nan, 0.5, 0.5, 0.5])), dict(ws=nan), dict(ws=-0.1), dict(ws=1.1), dict(t=(None, a2, ms)), dict(t=(a1, None, ms)),
               dict(t=(a1, a2, None))):
        assert setter(**kw) == -1, kw
        assert e.rollout_match_thresholds(0, 1, 5, 5) == held, kw
    assert lib.bgamd_env_rollout_match(None, 1, 4, None, None, 0.5, None, None, None) == -1
    assert _np(e.rollout(st, tu, 36, cube=cube, **{**_args(True, 4), "outcomes": True}))["trial_cube"].tolist() == good["trial_cube"].tolist()
    # ... (the Python surface cleared nothing it did not set: the match is still in force, and that call ran under it)
    _same(good, {**good, **_np(e.rollout_match_read(per_trial=True))})
    # while a match is set: no cube, Jacoby, no luck pass -- refused before anything is played, and the read calls refuse afterwards
    with pytest.raises(bg.BgamdError, match="-1"):
        e.rollout(st, tu, 36, max_plies=4, seed=CC.SEED, variance_reduction=True)
    with pytest.raises(bg.BgamdError, match="-1"):
        e.rollout_match_read()
    cube_j = bg.Cube(1.0, 0.0, 1.0, 4, jacoby=True)
    with pytest.raises(bg.BgamdError, match="-1"):
        e.rollout(st, tu, 36, cube=cube_j, **_args(True, 4))
    with pytest.raises(bg.BgamdError, match="-1"):
        e.rollout(st, tu, 36, max_plies=4, seed=CC.SEED)
    assert setter(flags=0, M=-1, met=None, pc=None, ws=nan, t=(None, None, None)) == 0
    e.rollout(st, tu, 36, cube=cube_j, **_args(True, 4))                                       # cleared: Jacoby is the cube's again
    with pytest.raises(ValueError):
        e.rollout(st, tu, 36, match=match, **_args(True, 4))                                  # the Python surface: match without cube
    # a bad entry of the score tables: refused with the bad states, before anything is played
    for x1, x2, s in (([0, 5, 5], [5, 5, 5], [0, 0, 0]), ([5, 5, 8], [5, 5, 5], [0, 0, 0]), ([5, 5, 5], [5, -1, 5], [0, 0, 0]),
                      ([5, 5, 5], [5, 5, 5], [0, 3, 0]), ([5, 5, 5], [5, 5, 5], [0, 0, -1]), ([5, 5, 5], [5, 5, 5], [0, 1, 0]),
                      ([5, 1, 5], [5, 5, 5], [0, 0, 0]), ([5, 5, 5], [5, 5, 1], [0, 0, 0]), ([5, 5, 5], [5, 5, 5], [2, 0, 0])):
        with pytest.raises(bg.BgamdError, match="-1"):
            e.rollout(st, tu, 36, cube=cube, match=bg.Match(_table(bg, MC.J7), x1, x2, s), **_args(True, 4))
        with pytest.raises(bg.BgamdError, match="-1"):
            e.rollout_match_read()
    bad_st = st.copy()
    bad_st[0, 3] = 16
    with pytest.raises(bg.BgamdError, match="-5"):
        e.rollout(bad_st, tu, 36, cube=cube, match=match, **_args(True, 4))
    # ... and the env is as good as before
    again = _np(e.rollout(st, tu, 36, cube=cube, match=match, **_args(True, 4)))
    _same(good, again)
    assert e.rollout_info() == info and e.rollout_cube_info() == cinfo
    # new tables end the readability of the rollout that ran under the old ones; clearing does not
    assert setter(flags=0) == 0
    e.rollout_match_read()
    assert setter() == 0
    with pytest.raises(bg.BgamdError, match="-1"):
        e.rollout_match_read()
    with pytest.raises(bg.BgamdError, match="-1"):
        e.rollout_paired([0, 1, 2], "mwc")
    e.rollout_paired([0, 1, 2], "cubeful")
    assert _capi.MATCH_ON == 1
    e.close()


# ---- (6) analysis.cube_action ----------------------------------------------------------------------------------------------------------------

def test_cube_action_at_a_match_score(bg, weights, env):
    from backgammon_env import analysis
    from backgammon_env.analysis import cube_action
    cst, ctu = CC.positions()
    st = np.stack([cst[0], cst[1], cst[0], cst[0], cst[2], cst[0]]).astype(np.int32)
    tu = np.array([0, 1, 0, 0, 0, 0], np.int32)
    value, owner = [1, 1, 1, 2, 1, 1], [0, 0, 0, 0, 0, 2]
    a1, a2, ms = [5, 5, 1, 2, 5, 5], [5, 3, 4, 5, 5, 5], [0, 0, 1, 0, 0, 0]
    T, M, off = 72, 6, 3
    table = _table(bg, MC.J7)
    match = bg.Match(table, a1, a2, ms)
    res = cube_action(env, st, tu, cube_value=value, cube_owner=owner, trials=T, max_plies=M, seed=CC.SEED, group_offset=off, match=match)
    assert [r["action"] for r in res[2:]] == ["Crawford game", "dead cube", "game over", "no access"]
    assert all("dt" not in r for r in res[2:]) and res[4]["nd"] == MM.after(MC.J7, 5, 3, 0) == res[4]["mwc"]
    assert res[0]["action"] in analysis.CUBE_ACTIONS and res[1]["action"] in analysis.CUBE_ACTIONS
    assert res[0]["dp"] == MM.after(MC.J7, 4, 5, 0) and res[1]["dp"] == MM.after(MC.J7, 2, 5, 0)
    # nd and dt are the two single rollouts, bit for bit; dt - nd is the paired read
    for p in (0, 1):
        side = (lambda x: x) if tu[p] == 0 else (lambda x: 1.0 - x)
        sg = 1.0 if tu[p] == 0 else -1.0
        kw = dict(max_plies=M, rotate=True, seed=CC.SEED, position_offset=off + p, variance_reduction=True, per_trial=True,
                  match=bg.Match(table, a1[p], a2[p], ms[p]))
        nd = _np(env.rollout(st[p:p + 1], tu[p:p + 1], T, cube=bg.Cube(hold_turn0=True, value=[value[p]], owner=[owner[p]]), **kw))
        dt = _np(env.rollout(st[p:p + 1], tu[p:p + 1], T, cube=bg.Cube(hold_turn0=True, value=[2 * value[p]], owner=[2 - int(tu[p])]), **kw))
        assert res[p]["nd"] == side(nd["mwc"][0]) and res[p]["nd_stderr"] == nd["mwc_stderr"][0] and res[p]["mwc"] == nd["mwc"][0]
        assert res[p]["dt"] == side(dt["mwc"][0]) and res[p]["dt_stderr"] == dt["mwc_stderr"][0]
        m, se = MM.paired(dt["trial_mwc"][0], nd["trial_mwc"][0])
        assert res[p]["diff"] == sg * m and math.isclose(res[p]["diff_stderr"], se, rel_tol=1e-12, abs_tol=0.0)
        assert res[p]["action"] == analysis.cube_decision(res[p]["nd"], res[p]["dt"], res[p]["dp"])
        assert 0.0 <= res[p]["nd"] <= 1.0 and 0.0 <= res[p]["dt"] <= 1.0
    assert res[1]["nd"] > 0.5 and res[1]["shares"]["win"] > 0.9                 # the bear-off's roller stands at 0.98 and leads


def test_the_example_runs_at_a_match_score():
    site_flags = (["-s"] if sys.flags.no_user_site else []) + (["-E"] if sys.flags.ignore_environment else [])
    r = subprocess.run([sys.executable, *site_flags, os.path.join(ROOT, "examples", "cube_action.py"), "--trials", "72", "--max-plies", "6",
                        "--match-to", "5", "--score", "4,2", "--post-crawford"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    # PLAYER1 is 1-away: its cube is dead where it rolls; PLAYER2, 3-away after the Crawford game, has a decision where it rolls
    assert len(lines) == 9 and "dead cube" in lines[1] and "dead cube" in lines[2] and "game over" in lines[6] and "no access" in lines[3]
    assert any(a in lines[4] for a in ("no double, take", "double, take", "double, pass", "too good, pass", "too good, take"))
    assert lines[8] == "package %s library %s" % (os.path.join(ROOT, "backgammon-engine_amd", "backgammon_env"),
                                                  os.path.join(ROOT, "backgammon-engine_amd", "libbgamd.so")), r.stdout
