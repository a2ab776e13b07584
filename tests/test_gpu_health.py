"""The net health check and the choice spread on the MI355X (include/bgamd.h: bgamd_net_health, bgamd_env_choice_spread) against the
float64 references of tests/health_ref.py.

Counts are compared as intervals: the device forms a in fp32, so a (row, unit) pair whose exact |a| lies within the fp32 chain's error m
of the threshold may fall either way -- every count lies in [sure, sure + undecided], and tests/test_health_cpu.py checks that the
undecided pairs are at most 1 % of all pairs for every table, row set, size and threshold used here.  The spread is integer / min / max
work on stored values: it is compared exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

import health_ref as H
import nets as N

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


@pytest.fixture(scope="module")
def health():
    from backgammon_env import health
    return health


def _np(t):
    return t.detach().cpu().numpy()


# ---- 1. weights ------------------------------------------------------------------------------------------------------------------------

def test_weight_fields(bg, health):
    import ctypes
    from backgammon_env import _capi
    lib = _capi.load()
    tables = [(name, N.table(name)) for name in N.NAMES] + list(H.injected_tables())
    seen = set()
    for label, w in tables:
        ref = H.weights_ref(w)
        got = health.net_health(w)
        w32 = np.ascontiguousarray(w, dtype=np.float32)
        accepted = lib.bgamd_weights_check(w32.ctypes.data_as(ctypes.c_void_p)) == 0
        assert got["nonfinite"] == ref["nonfinite"] == int((~np.isfinite(w)).sum()), label
        gm = np.array([got["max_abs"][k] for k in health.TENSORS], np.float32)
        assert gm.tobytes() == ref["max_abs"].tobytes(), (label, gm, ref["max_abs"])
        assert got["fits_f16_split"] == accepted == ref["fits_f16_split"], label
        assert got["rows"] == 0 and got["saturated"] == 0 and got["dead_units"] == 0 and got["saturated_share"] == 0.0, label
        assert got["max_abs_preact"] == 0 and got["v_min"] == 0 and got["v_max"] == 0 and not _np(got["unit_saturated"]).any(), label
        seen.add((got["nonfinite"] > 0, got["fits_f16_split"]))
    assert seen == {(False, True), (False, False), (True, False)}


# ---- 2. rows ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", N.NAMES)
def test_row_fields(bg, health, family):
    w = N.table(family)
    theta = torch.from_numpy(w.copy()).cuda()
    for key, (st, tu, X) in H.row_sets().items():
        assert set(tu.tolist()) == {0, 1}
        rows = bg.pack_rows(st, tu)
        a, m, v, _ = H.pairs(family, key)
        for n in H.sizes(len(X)):
            vb = H.value_bound(w, X[:n], family)
            for thr in H.THRESHOLDS:
                ref = H.counts_ref(a[:n], m[:n], thr)
                got = health.net_health(theta, rows[:n], thr)
                unit = _np(got["unit_saturated"]).astype(np.int64)
                what = (family, key, n, thr)
                print("HEALTH %-13s %-5s n %5d thr %4g: saturated %7d in [%d, %d], max|a| %.6g (ref %.6g +- %.2g), v [%.7g, %.7g] (ref [%.7g, %.7g] +- %.2g)"
                      % (family, key, n, thr, got["saturated"], ref["sure"], ref["sure"] + ref["undecided"], got["max_abs_preact"],
                         ref["max_abs_preact"], ref["preact_bound"], got["v_min"], got["v_max"], v[:n].min(), v[:n].max(), vb))
                assert got["rows"] == n and got["nonfinite"] == 0 and got["fits_f16_split"], what
                assert ref["sure"] <= got["saturated"] <= ref["sure"] + ref["undecided"], what
                assert (ref["unit_sure"] <= unit).all() and (unit <= ref["unit_sure"] + ref["unit_undecided"]).all(), what
                assert got["saturated"] == unit.sum() and got["dead_units"] == int((unit == n).sum()), what
                assert ref["dead_sure"] <= got["dead_units"] <= ref["dead_max"], what
                assert abs(got["saturated_share"] - got["saturated"] / (n * 128.0)) < 1e-12, what
                assert abs(got["max_abs_preact"] - ref["max_abs_preact"]) <= ref["preact_bound"], what
                assert abs(got["v_min"] - v[:n].min()) <= vb and abs(got["v_max"] - v[:n].max()) <= vb, what


def test_dead_unit_and_constant_net(bg, health):
    st, tu, X = H.row_sets()["sweep"]
    rows = bg.pack_rows(st, tu)
    w = N.table("w1_x64").copy()
    w[N.O1 + 5] = 1e4                                       # saturated on every row, whatever x
    got = health.net_health(w, rows)
    ref = H.net_health_ref(w, X, 15.0)
    assert _np(got["unit_saturated"])[5] == len(X) and ref["dead_sure"] >= 1
    assert ref["dead_sure"] <= got["dead_units"] <= ref["dead_max"]
    assert got["saturated_share"] > 0.25
    z = health.net_health(N.table("zero_w1"), rows)
    assert z["saturated"] == 0 and z["dead_units"] == 0 and z["v_min"] == z["v_max"]
    assert abs(z["v_min"] - N.constant_value(N.table("zero_w1"))) <= 1e-6


# ---- 3. edge calls ---------------------------------------------------------------------------------------------------------------------

def test_edge_calls(bg, health):
    import ctypes as C
    from backgammon_env import _capi
    lib = _capi.load()
    st, tu, X = H.row_sets()["g5"]
    rows = bg.pack_rows(st, tu)
    w = torch.from_numpy(N.table("ckpt").copy()).cuda()
    out = torch.zeros(C.sizeof(_capi.NetHealth), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.bgamd_net_health(p(w), None, 0, 15.0, p(out), s) == 0                      # n_rows = 0, d_rows NULL
    assert lib.bgamd_net_health(p(w), p(rows), 0, 15.0, p(out), s) == 0
    for bad in (0.0, -1.0, float("nan")):
        assert lib.bgamd_net_health(p(w), p(rows), 4, bad, p(out), s) == _capi.E_INVALID
    assert lib.bgamd_net_health(p(w), p(rows), -1, 15.0, p(out), s) == _capi.E_INVALID
    assert lib.bgamd_net_health(p(w), None, 4, 15.0, p(out), s) == _capi.E_INVALID
    assert lib.bgamd_net_health(None, p(rows), 4, 15.0, p(out), s) == _capi.E_INVALID
    assert lib.bgamd_net_health(p(w), p(rows), 4, 15.0, None, s) == _capi.E_INVALID
    torch.cuda.synchronize()
    h0 = health.net_health(w, rows[:0])
    assert h0["rows"] == 0 and h0["saturated"] == 0 and h0["max_abs"]["fc1.weight"] > 0 and h0["v_min"] == 0 == h0["v_max"]
    # a table with NaN: the call completes and reports them
    bad = N.table("ckpt").copy()
    bad[[3, 25400, 25600]] = np.nan
    hb = health.net_health(bad, rows)
    assert hb["nonfinite"] == 3 and not hb["fits_f16_split"] and hb["rows"] == len(X)
    with pytest.raises(health.NetHealthError, match="3 of 25601 weights are not finite"):
        health.check(hb)
    health.check(health.net_health(w, rows))


# ---- 4. reproducible, and beside an env at play ---------------------------------------------------------------------------------------------

def _raw(health, theta, rows, thr=15.0):
    h = health.net_health(theta, rows, thr)
    return (h["nonfinite"], h["rows"], h["saturated"], h["dead_units"], tuple(sorted(h["max_abs"].items())),
            np.float32(h["max_abs_preact"]).tobytes(), np.float32(h["v_min"]).tobytes(), np.float32(h["v_max"]).tobytes(),
            h["fits_f16_split"], _np(h["unit_saturated"]).tobytes())


def test_bit_identical_and_no_side_effect(bg, health, weights):
    from backgammon_env.learner import DeviceTDLambdaLearner
    st, tu, X = H.row_sets()["sweep"]
    rows = bg.pack_rows(st, tu)
    theta = torch.from_numpy(N.table("w1_x16").copy()).cuda()
    assert _raw(health, theta, rows, 1.0) == _raw(health, theta, rows, 1.0)
    assert _raw(health, theta, rows[:65]) == _raw(health, theta, rows[:65])
    torch.cuda.synchronize()                            # theta and rows are complete before another stream reads them

    def play(with_health):
        env = bg.VecGame(256, seed=77)
        env.load_weights(weights)
        L = DeviceTDLambdaLearner(weights, max_games=256)
        before = _np(L.theta)
        env.run_greedy(6)
        if with_health:
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):               # on a side stream, the env's steps still in flight on the main one
                health.net_health(theta, rows)
                L.health(rows)
            env.run_greedy(2)
            env.choice_spread()
        else:
            env.run_greedy(2)
        torch.cuda.synchronize()
        snap, lc = _np(env.snapshot()), {k: _np(v) for k, v in env.last_choice().items()}
        assert _np(L.theta).tobytes() == before.tobytes()
        env.close()
        return snap, lc
    a, b = play(True), play(False)
    assert a[0].tobytes() == b[0].tobytes()
    assert all(a[1][k].tobytes() == b[1][k].tobytes() for k in a[1])


# ---- 5. the learner's own weights -----------------------------------------------------------------------------------------------------------

def test_learner_health(bg, health, weights):
    from backgammon_env.learner import DeviceTDLambdaLearner, play_round
    env = bg.VecGame(64, seed=5)
    env.load_weights(weights)
    traj, lengths, won = play_round(env, max_plies=256)
    L = DeviceTDLambdaLearner(weights, max_games=64, alpha=0.1, lam=0.7)
    L.replay_rows(traj, lengths, won, batch_scale=1.0 / 64)
    assert _np(L.theta).tobytes() != weights.tobytes()                     # a few replay steps have moved the weights
    rows = health.health_rows(traj, lengths, [0, 3, 10])
    assert len(rows) > 64
    a, b = L.health(rows), health.net_health(L.theta, rows)
    for k in a:
        if k == "unit_saturated":
            assert _np(a[k]).tobytes() == _np(b[k]).tobytes()
        else:
            assert a[k] == b[k], k
    assert a["rows"] == len(rows) and a["nonfinite"] == 0 and a["fits_f16_split"]
    env.close()


# ---- 6. choice spread ----------------------------------------------------------------------------------------------------------------------

def _positions(n):
    """n lanes from nets.py's position families: fixture G5's game positions (both movers), closed boards and stuck positions (no legal
    move for most rolls), single checkers, bear-offs, and finished games (15 borne off)."""
    g5s, g5t = N.g5_rows()
    fin = np.zeros((2, 28), np.int32)                      # (one side has borne off all fifteen: the other one is to move)
    fin[0, 26] = 15; fin[0, [3, 4]] = [-7, -8]
    fin[1, 27] = 15; fin[1, [20, 21]] = [7, 8]
    fams = [N.closed_board_positions(), N._stuck(), N._singles(), N._bearoffs(), (fin, np.array([1, 0], np.int32))]
    small_s, small_t = np.concatenate([f[0] for f in fams]), np.concatenate([f[1] for f in fams])
    fam_of = np.concatenate([np.full(len(f[0]), k) for k, f in enumerate(fams)])     # 0 closed, 1 stuck, 2 singles, 3 bear-offs, 4 finished
    st, tu, fam = [], [], []
    for i in range(n):
        if i % 3 == 2:
            j = (i // 3) % len(small_s)
            st.append(small_s[j]); tu.append(small_t[j]); fam.append(fam_of[j])
        else:
            st.append(g5s[(7 * i) % len(g5s)]); tu.append(g5t[(7 * i) % len(g5s)]); fam.append(-1)
    dice = np.array([[1 + i % 6, 1 + (i // 6) % 6] for i in range(n)], np.int32)             # all 36 ordered pairs, doubles included
    return np.array(st, np.int32), np.array(tu, np.int32), dice, np.array(fam)


def _check_spread(env, n, zero_w1=False, eps0=True):
    before = _np(env.snapshot())
    lc0 = {k: _np(v) for k, v in env.last_choice().items()}
    got = env.choice_spread()
    info, _, val = env.unique_rows(want_states=False)
    info, val = _np(info), _np(val)
    ref = H.spread_ref(info, val, n)
    for k in ("count", "tied"):
        assert (_np(got[k]) == ref[k]).all(), k
    for k in ("best", "worst"):
        assert _np(got[k]).tobytes() == ref[k].tobytes(), k
    assert [got["choice_lanes"], got["all_tied_lanes"], got["rows"], got["empty_lanes"]] == ref["summary"]
    assert got["rows"] == len(val)
    cnt, tied = ref["count"], ref["tied"]
    assert (tied[cnt >= 1] >= 1).all() and (tied <= cnt).all()
    if zero_w1:
        assert (tied[cnt >= 2] == cnt[cnt >= 2]).all() and got["all_tied_lanes"] == got["choice_lanes"]
    if eps0:
        lv = lc0["value"]
        assert _np(got["best"])[cnt >= 1].tobytes() == lv[cnt >= 1].tobytes()
    # no side effect
    assert _np(env.snapshot()).tobytes() == before.tobytes()
    assert all(_np(v).tobytes() == lc0[k].tobytes() for k, v in env.last_choice().items())
    return got, info


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_choice_spread(bg, weights, n):
    from backgammon_env import _capi
    st, tu, dice, fam = _positions(n)
    dbl = dice[:, 0] == dice[:, 1]
    movers, empties, choices = set(), 0, 0
    for name in ("ckpt", "zero_w1", "w1_x64"):
        env = bg.VecGame(n, seed=11)
        env.load_weights(N.table(name))
        with pytest.raises(bg.BgamdError) as e:                                           # before any greedy step
            env.choice_spread()
        assert e.value.code == _capi.E_INVALID
        env.set_states(st, tu)
        env.set_dice(dice)
        env.step_greedy(roll=False, auto_reset=False)
        got, info = _check_spread(env, n, zero_w1=name == "zero_w1")
        movers |= set(((info[:, 1] >> 31) & 1).tolist())
        empties += got["empty_lanes"]
        choices += got["choice_lanes"]
        if n >= 64:                                        # the cases the inputs were chosen for do occur, each on its own
            cnt = _np(got["count"])
            row_dbl, row_p2 = dbl[info[:, 0]], ((info[:, 1] >> 31) & 1) == 1
            # rows of doubles turns and of the other turns, from both movers: the two pairs of arenas the leaf stage fills
            # (non-doubles 0 / 1, doubles 2 / 3) both hold rows of this step
            for d in (False, True):
                for p2 in (False, True):
                    assert ((row_dbl == d) & (row_p2 == p2)).sum() > 0, (d, p2)
                assert (cnt[dbl == d] >= 2).any(), d
            assert (cnt[fam == 1] == 0).any(), cnt[fam == 1]                               # both on the bar against six made points: no move
            # a finished lane: the late bear-offs end with this step; without auto-reset those lanes stay finished and have no rows in the next
            done = (_np(env.flags()) & 4) != 0
            assert done.any() and not done.all()
            env.step_greedy(roll=True, auto_reset=False)
            got2, _ = _check_spread(env, n, zero_w1=name == "zero_w1")
            assert (_np(got2["count"])[done] == 0).all() and got2["empty_lanes"] >= int(done.sum())
        env.run_greedy(3, roll=True, auto_reset=True)                                      # ... then it describes the LAST step of a run
        _check_spread(env, n, zero_w1=name == "zero_w1")
        assert env.stats()["error_flags"] == 0
        env.close()
    if n >= 64:
        assert movers == {0, 1} and empties > 0 and choices > 0


def test_choice_spread_null_pointers(bg, weights):
    import ctypes as C
    env = bg.VecGame(64, seed=3)
    env.load_weights(weights)
    env.step_greedy()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert env._lib.bgamd_env_choice_spread(env._h, None, None, None, None, None, s) == 0
    tied = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert env._lib.bgamd_env_choice_spread(env._h, None, None, None, C.c_void_p(tied.data_ptr()), None, s) == 0
    assert (_np(tied) == _np(env.choice_spread()["tied"])).all()
    env.close()


# ---- 7. the example, end to end ----------------------------------------------------------------------------------------------------------------

def _example(args, tmp_path, rounds=2):
    env = dict(os.environ)
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", "selfplay_train.py"), "--games", "256", "--rounds", str(rounds),
                           "--max-plies", "200", "--arena", "64", "--health-rows", "2048", *args], capture_output=True, text=True, env=env,
                          cwd=str(tmp_path), timeout=300)


def test_example_prints_health_and_stops_on_a_diverged_table(tmp_path):
    r = _example([], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if " health: " in ln]
    assert len(lines) == 3 and lines[0].startswith("start") and lines[1].startswith("round 1 ") and lines[2].startswith("round 2 "), r.stdout
    for ln in lines[1:]:
        assert "nonfinite 0" in ln and "saturated share" in ln and "dead units" in ln and "all-tied share" in ln and "fc2.b" in ln
    # a NaN in the starting weights: a message naming the count, no traceback
    w = N.table("xavier").copy()
    w[[17, 25500]] = np.nan
    f = tmp_path / "nan.f32"
    w.tofile(str(f))
    r = _example(["--init-weights", str(f)], tmp_path)
    assert r.returncode != 0
    assert "2 of 25601 weights are not finite" in r.stderr and "STOPPED" in r.stderr and "Traceback" not in r.stderr, r.stderr


def test_example_health_lines_of_continuous_windows(tmp_path):
    """One classic round, then three pipelined windows: the health rows come out of the ring log (16 of a window's steps), the line follows
    the learner thread's join.  Every window measures the 2 048 rows asked for -- 256 lanes x 16 steps hold 4 096 -- and none of them is an
    unwritten (all-zero) slot: an empty board would show as the same value on every such row, and is filtered before the count."""
    r = _example(["--continuous", "--pipeline-rounds", "--classic-rounds", "1", "--slots", "64", "--window-steps", "40", "--ring-steps", "256",
                  "--verbose"], tmp_path, rounds=4)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if " health: " in ln]
    assert [ln.split(" (")[0] for ln in lines] == ["start", "round 1", "window 1", "window 2", "window 3"], r.stdout
    for ln in lines[2:]:
        assert "nonfinite 0" in ln and " on 2048 rows " in ln and "all-tied share" in ln and "after 16 turns" not in ln, ln
        assert int(ln.split(" of ")[-1].split(" lanes")[0]) >= 64, ln               # a window's last step: the lanes are live
