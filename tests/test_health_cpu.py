"""CPU side of the net health check (tests/health_ref.py, backgammon_env/health.py): the ABI is there, the float64 reference agrees with
the plain fp32 forward pass, the condition the GPU test's count intervals rest on holds for every table and row set it uses, the
reference's acceptance test is bgamd_weights_check's, check() names what failed and health_rows never measures padding."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import health_ref as H
import nets as N

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from backgammon_env import _capi
    return _capi.load()


def test_abi_declares_exports_and_binds_both_entries(lib):
    from backgammon_env import _capi
    header = open(os.path.join(ROOT, "include", "bgamd.h")).read()
    bound = {name for name, _, _ in _capi.SYMBOLS}
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("bgamd_net_health", "bgamd_env_choice_spread"):
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert re.search(r"\bT %s\b" % sym, exported), sym
        assert sym in bound and getattr(lib, sym).argtypes is not None, sym
    assert "bgamd_net_health_t" in header
    # the ctypes mirror is the header's struct: 4 x int64, 7 floats, int32, int32[128]
    assert ctypes.sizeof(_capi.NetHealth) == 576 and _capi.NetHealth.unit_saturated.offset == 64
    from backgammon_env import _srchash
    assert any(f.endswith("bg_health.h") for f in _srchash.source_files())


@pytest.mark.parametrize("family", N.NAMES)
def test_reference_against_the_fp32_forward_pass(family):
    """The reference's net output against nets.forward_np32 on the sweep (every value of every feature), within the bound the reference
    itself derives for any fp32 evaluation of that net (health_ref.preactivations) -- under all eleven tables."""
    w = N.table(family)
    X = H.row_sets()["sweep"][2]
    a, m, v, vb = H.pairs(family, "sweep")
    got = N.forward_np32(w, X).astype(np.float64)
    err = np.abs(got - v)
    print("%s: max |numpy fp32 - fp64| = %.3g, derived bound %.3g .. %.3g" % (family, err.max(), vb.min(), vb.max()))
    assert (err <= vb).all(), (family, float(err.max()))
    # ... and its pre-activations against the fp32 matrix product, within m
    W1, b1, _, _ = H.split(w)
    a32 = (X @ W1.T + b1).astype(np.float64)
    assert (np.abs(a32 - a) <= m).all(), family


@pytest.mark.parametrize("family", N.NAMES)
def test_undecided_pairs_are_at_most_one_per_cent(family):
    """The condition the GPU test rests on: for every table, row set, prefix size and threshold it uses, the (row, unit) pairs whose
    exact |a| lies within the fp32 chain's error of the threshold are at most 1 % of all pairs -- the count intervals [sure, sure +
    undecided] are tight.  A condition on the inputs, checked here; a row set that broke it would be replaced."""
    for key, (st, tu, X) in H.row_sets().items():
        a, m, _, _ = H.pairs(family, key)
        for thr in H.THRESHOLDS:
            for n in H.sizes(len(X)):
                c = H.counts_ref(a[:n], m[:n], thr)
                assert c["undecided"] <= 0.01 * n * N.N_HID, (family, key, thr, n, c["undecided"])
        assert set(tu.tolist()) == {0, 1}, key                  # both turn bits are present


def test_saturated_and_constant_nets():
    X = H.row_sets()["sweep"][2]
    r = H.net_health_ref(N.table("w1_x64"), X, 15.0)
    assert r["sure"] > 0.25 * len(X) * N.N_HID, r["sure"]              # the checkpoint's W1 x 64: a saturated hidden layer
    assert r["dead_sure"] == int((r["unit_sure"] == len(X)).sum()) and r["dead_sure"] <= r["dead_max"]
    w = N.table("w1_x64").copy()
    w[N.O1 + 5] = 1e4                                                   # a unit that is saturated on EVERY row, whatever x
    d = H.net_health_ref(w, X, 15.0)
    assert d["unit_sure"][5] == len(X) and d["dead_sure"] >= 1 and d["dead_sure"] >= r["dead_sure"]
    assert H.net_health_ref(w, X[:0], 15.0)["dead_sure"] == 0           # no rows: no dead units
    z = H.net_health_ref(N.table("zero_w1"), X, 15.0)
    c = N.constant_value(N.table("zero_w1"))
    assert z["sure"] == 0 and z["undecided"] == 0 and z["dead_max"] == 0
    assert z["v_min"] == z["v_max"] and abs(z["v_min"] - c) <= 1e-15


def test_reference_acceptance_is_weights_check(lib):
    def chk(w):
        w = np.ascontiguousarray(w, dtype=np.float32)
        return lib.bgamd_weights_check(w.ctypes.data_as(ctypes.c_void_p))
    for name in N.NAMES:
        r = H.weights_ref(N.table(name))
        assert r["fits_f16_split"] == (chk(N.table(name)) == 0) and r["fits_f16_split"] and r["nonfinite"] == 0, name
    seen = set()
    for label, w in H.injected_tables():
        r = H.weights_ref(w)
        assert r["fits_f16_split"] == (chk(w) == 0), label
        assert r["nonfinite"] == int((~np.isfinite(w)).sum()), label
        seen.add(r["fits_f16_split"])
    assert seen == {True, False}                                       # e.g. 65 504 in fc2.weight is accepted, in fc1.weight it is not


def _health(**kw):
    h = {"nonfinite": 0, "rows": 1000, "saturated": 0, "dead_units": 0, "saturated_share": 0.0, "fits_f16_split": True,
         "max_abs": {"fc1.weight": 1.0, "fc1.bias": 1.0, "fc2.weight": 1.0, "fc2.bias": 1.0}, "max_abs_preact": 3.0, "v_min": 0.4,
         "v_max": 0.6, "threshold": 15.0}
    h.update(kw)
    return h


def test_check_names_every_failed_condition():
    from backgammon_env import health
    spread = {"choice_lanes": 200, "all_tied_lanes": 150, "rows": 900, "empty_lanes": 3}
    health.check(_health())                                            # healthy: nothing raised
    health.check(_health(saturated_share=0.9), spread)                 # soft limits are off unless given
    with pytest.raises(health.NetHealthError, match=r"7 of 25601 weights are not finite"):
        health.check(_health(nonfinite=7))
    with pytest.raises(health.NetHealthError, match=r"f16 hi \+ lo planes.*70000"):
        health.check(_health(fits_f16_split=False, max_abs={"fc1.weight": 70000.0, "fc1.bias": 1, "fc2.weight": 1, "fc2.bias": 1}))
    with pytest.raises(health.NetHealthError, match=r"saturated share 0\.6250 .* limit 0\.5000; 3 dead units"):
        health.check(_health(saturated_share=0.625, dead_units=3), max_saturated_share=0.5)
    with pytest.raises(health.NetHealthError, match=r"150 of 200 lanes .*0\.7500.* limit 0\.7000"):
        health.check(_health(), spread, max_all_tied_share=0.7)
    health.check(_health(saturated_share=0.5), spread, max_saturated_share=0.5, max_all_tied_share=0.75)     # at the limit: allowed
    with pytest.raises(health.NetHealthError) as e:                    # everything at once: every condition is named
        health.check(_health(nonfinite=1, fits_f16_split=False, saturated_share=0.9), spread, 0.5, 0.1)
    assert len(e.value.failed) == 4 and [f[1] for f in e.value.failed][0] == 1
    for word in ("not finite", "f16 hi + lo", "saturated share 0.9000", "all candidates tie"):
        assert word in str(e.value)
    assert health.all_tied_share({"choice_lanes": 0, "all_tied_lanes": 0}) == 0.0


def test_health_rows_never_selects_padding():
    torch = pytest.importorskip("torch")
    from backgammon_env import health
    rng = np.random.RandomState(3)
    T, n = 12, 9
    lengths = np.array([0, 1, 5, 12, 12, 3, 0, 7, 11])
    traj = np.zeros((T, n, 8), np.int32)
    for g in range(n):                                                 # inside a game: (step, lane) stamped into the row; beyond: zeros
        for t in range(lengths[g]):
            traj[t, g] = [1000 * t + g + 1] + rng.randint(1, 99, 7).tolist()
    tj, ln = torch.from_numpy(traj), torch.from_numpy(lengths)
    for steps in ([0], [4], [0, 4, 11], [11, 11], list(range(T)), [12, -1, 40], []):
        got = health.health_rows(tj, ln, steps).numpy()
        want = sorted(1000 * t + g + 1 for t in steps if 0 <= t < T for g in range(n) if t < lengths[g])
        assert sorted(got[:, 0].tolist()) == want, steps
        assert got.shape[1:] == (8,) and (got != 0).all()              # never a padding row


def test_round_rows_cover_the_round_not_its_first_step():
    """round_rows(traj, lengths, n_rows): n_rows turns spread evenly over ALL the round's turns.  With n_rows = the lane count -- the
    training example's default -- the rows must come from many steps, not from step 0 alone."""
    torch = pytest.importorskip("torch")
    from backgammon_env import health
    rng = np.random.RandomState(5)
    T, n = 60, 257
    lengths = rng.randint(0, T + 1, n)
    lengths[:4] = [0, 1, T, T]
    traj = np.zeros((T, n, 8), np.int32)
    for g in range(n):
        for t in range(lengths[g]):
            traj[t, g] = [1000 * t + g + 1] * 8                        # (step, lane) stamped into the row; beyond the game: zeros
    tj, ln = torch.from_numpy(traj), torch.from_numpy(lengths)
    total = int(lengths.sum())
    every = sorted(1000 * t + g + 1 for g in range(n) for t in range(lengths[g]))
    for k in (1, 7, n, 1000, total - 1, total, total + 5):
        got = health.round_rows(tj, ln, k).numpy()
        stamps = got[:, 0].tolist()
        assert got.shape == (min(k, total), 8) and (got != 0).all(), k                       # never a padding row
        assert len(set(stamps)) == len(stamps) and set(stamps) <= set(every), k              # every row a turn of the round, once
        if k >= total:
            assert sorted(stamps) == every
    steps = {s // 1000 for s in health.round_rows(tj, ln, n).numpy()[:, 0].tolist()}
    # n rows of ~ n * T / 2 turns: one row per ~ T / 2 turns, so every step with at least that many lanes left gets one
    stride = -(-total // n)
    want = {t for t in range(T) if int((lengths > t).sum()) >= stride}
    assert want <= steps and len(steps) >= 16 and 0 in steps and max(steps) >= T // 2, sorted(steps)
    assert health.round_rows(tj, torch.zeros(n, dtype=torch.int64), 10).shape == (0, 8)      # no game inside the log: no rows
    assert health.round_rows(tj, ln, 0).shape == (0, 8)
    # thin(): evenly over all rows, not the head
    r = torch.arange(100)[:, None].repeat(1, 8)
    assert health.thin(r, 100) is r and health.thin(r, 500) is r
    assert health.thin(r, 10)[:, 0].tolist() == list(range(0, 100, 10)) and health.thin(r, 3)[:, 0].tolist() == [0, 33, 66]


def test_check_min_choice_lanes():
    from backgammon_env import health
    few = {"choice_lanes": 3, "all_tied_lanes": 3}
    health.check(_health(), few, max_all_tied_share=0.5, min_choice_lanes=64)                # a share of 3 lanes is not judged
    with pytest.raises(health.NetHealthError, match="3 of 3 lanes"):
        health.check(_health(), few, max_all_tied_share=0.5)
    with pytest.raises(health.NetHealthError, match="64 of 64 lanes"):
        health.check(_health(), {"choice_lanes": 64, "all_tied_lanes": 64}, max_all_tied_share=0.5, min_choice_lanes=64)
