"""The supervised step on the device (bgamd_td_fit_step, csrc/bg_fit.h) against the float64 reference of tests/fit_ref.py, parameter by
parameter within its bound (whose conditions tests/test_fit_cpu.py states): handed out and applied, at every tile edge of the kernel,
over several workgroups, several tiles per workgroup and several chunks, under the parity families and the edge nets of tests/nets.py,
with targets that are uniform, all 0, all 1, the net's own values, and not finite."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fit_ref as FR
import learner_ref as LR
import nets as N
from test_gpu_parity import _np

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_TD_VARS = ("BGAMD_TD_DIRECT_MIN", "BGAMD_TD_FUSE_STEP", "BGAMD_TD_MFMA_MIN", "BGAMD_TD_WIDE_MIN", "BGAMD_TD_PIPE", "BGAMD_TD_NT_MIN",
            "BGAMD_TD_FUSE_MIN", "BGAMD_TD_FUSE_G", "BGAMD_TD_LAZY", "BGAMD_TD_DENSE", "BGAMD_TD_NG", "BGAMD_TD_NO_WIDE_EVEN", "BGAMD_TD_FUSED")


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


_dev = {}


def _rows(bg, n):
    """the n rows of fit_ref.positions packed on the device; once, their encoding is held against the reference's features"""
    if n not in _dev:
        st, tu = FR.positions(n)
        rows = bg.pack_rows(st, tu).contiguous()
        if not _dev:
            assert np.array_equal(_np(bg.VecGame(1).encode_rows(rows)), FR.features(n))
        _dev[n] = rows
    return _dev[n]


def _learner(monkeypatch, net, config="default", max_games=64, env=None):
    from backgammon_env.learner import DeviceTDLambdaLearner
    for k in FR.VARS + _TD_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**FR.CONFIGS[config], **(env or {})}.items():
        monkeypatch.setenv(k, v)
    return DeviceTDLambdaLearner(N.table(net), max_games=max_games, alpha=LR.ALPHA)


def _step(L, rows, y, alpha=FR.ALPHA, hand_out=True):
    """bgamd_td_fit_step through the binding -> the update handed out (numpy) or None (applied)"""
    y = torch.as_tensor(y, dtype=torch.float32, device=L.device).contiguous()
    upd = torch.full((N.N_PARAMS,), 7.0, dtype=torch.float32, device=L.device) if hand_out else None
    L._capi.check(L._lib.bgamd_td_fit_step(L._h, L._p(rows), L._p(y), int(rows.shape[0]), alpha, L._p(upd) if hand_out else None, L._s()),
                  "td_fit_step")
    return _np(upd) if hand_out else None


def _within(got, want, bound, label):
    d = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d > 0, d / bound, 0.0)
    p = int(np.argmax(r))
    print("%s: worst device / bound = %.4f (%s)" % (label, float(r[p]), LR.where(p)))
    assert (d <= bound).all(), "%s: %d parameters outside the bound; the worst %s: |d| = %.3g = %.3g x the bound %.3g" % (
        label, int((d > bound).sum()), LR.where(p), d[p], float(r[p]), bound[p])


def _check(bg, monkeypatch, net, n, tset, config="default"):
    """handed out: within the bound, twice the same bits; applied: the weights within the bound (+ the rounding of θ + update); the
    statistics of the two counted steps"""
    label = "%s, %d rows, %s, %s" % (net, n, tset, config)
    ref = FR.reference(net, n, tset)
    bound = FR.bound(ref, n, config)
    L = _learner(monkeypatch, net, config)
    rows, y = _rows(bg, n), FR.targets(net, n, tset)
    L.fit_stats()
    upd = _step(L, rows, y)
    assert np.array_equal(_np(L.theta), N.table(net)), "a handed-out update was applied"
    _within(upd, ref.update, bound, label)
    again = _step(L, rows, y)
    assert np.array_equal(upd.view(np.uint32), again.view(np.uint32)), label + ": two calls, two results"
    sq, cnt, skipped = L.fit_stats()
    assert (cnt, skipped) == (2 * ref.rows, 2 * ref.skipped), label
    assert abs(sq - 2 * ref.sq) <= 2 * FR.sq_bound(ref), (label, sq, 2 * ref.sq)
    _step(L, rows, y, hand_out=False)
    th0, th1 = N.table(net).astype(np.float64), _np(L.theta)
    _within(th1, th0 + ref.update, bound + 2.0 ** -24 * np.maximum(np.abs(th0), np.abs(th1)), label + ", applied")
    assert L.fit_stats()[1:] == (ref.rows, ref.skipped)


@pytest.mark.parametrize("n", FR.FAMILY_SIZES)
@pytest.mark.parametrize("tset", FR.TARGET_SETS)
@pytest.mark.parametrize("net", [f for f in N.PARITY if f != "ckpt"])
def test_families(bg, monkeypatch, net, tset, n):
    """every parity family x every target set at 33, 257 and 1 061 rows, in every configuration that size runs in"""
    for config, sizes in FR.CONFIG_SIZES.items():
        if n in sizes:
            _check(bg, monkeypatch, net, n, tset, config)


@pytest.mark.parametrize("n", FR.SIZES)
@pytest.mark.parametrize("tset", FR.TARGET_SETS)
def test_checkpoint_at_every_size(bg, monkeypatch, tset, n):
    """the checkpoint at every tile edge: 1, 2, 31 .. 33, 63 .. 65, 255 .. 257, 1 061; several tiles per workgroup and several chunks
    where the size has them"""
    for config, sizes in FR.CONFIG_SIZES.items():
        if n in sizes:
            _check(bg, monkeypatch, "ckpt", n, tset, config)


def test_checkpoint_over_129_workgroups(bg, monkeypatch):
    _check(bg, monkeypatch, "ckpt", FR.LARGE, "uniform")


def test_edge_nets(bg, monkeypatch):
    """out_hi / out_lo: v is exactly 1 / 0, g exactly 0: the update is exactly zero and Σ δ² counts the rows the net denies.  zero_w1:
    under the bound.  w1_x64: finite only -- the hidden layer overflows, no bound is claimed (tests/test_gpu_learner_steps.py)."""
    n = 257
    rows = _rows(bg, n)
    for net, y, sq in (("out_hi", np.zeros(n, np.float32), float(n)), ("out_lo", np.ones(n, np.float32), float(n))):
        L = _learner(monkeypatch, net)
        L.fit_stats()
        assert not _step(L, rows, y).any()
        _step(L, rows, y, hand_out=False)
        assert np.array_equal(_np(L.theta), N.table(net)) and L.fit_stats() == (2 * sq, 2 * n, 0)
    for tset in FR.TARGET_SETS:
        _check(bg, monkeypatch, "zero_w1", n, tset)
    L = _learner(monkeypatch, "w1_x64")
    upd = _step(L, rows, FR.targets("w1_x64", n, "uniform"))
    assert np.isfinite(upd).all() and upd.any()


def test_rows_without_a_finite_target_add_nothing(bg, monkeypatch):
    """every target NaN or +-inf: an update of exact zeros, the weights to the bit, every row skipped, Σ δ² = 0 (mixed with finite
    targets: the `nonfinite` target set of the cases above, whose reference leaves those rows out)"""
    n = 65
    L = _learner(monkeypatch, "ckpt")
    y = np.full(n, np.nan, np.float32)
    y[1::3], y[2::3] = np.inf, -np.inf
    L.fit_stats()
    assert not _step(L, _rows(bg, n), y).any()
    _step(L, _rows(bg, n), y, hand_out=False)
    assert np.array_equal(_np(L.theta), N.table("ckpt")) and L.fit_stats() == (0.0, 0, 2 * n)


def test_no_rows(bg, monkeypatch):
    """n = 0 (d_rows and d_target may be NULL): an all-zero update, the weights bit-identical, nothing counted"""
    L = _learner(monkeypatch, "ckpt")
    L.fit_stats()
    upd = torch.full((N.N_PARAMS,), 7.0, dtype=torch.float32, device=L.device)
    assert L._lib.bgamd_td_fit_step(L._h, None, None, 0, FR.ALPHA, L._p(upd), L._s()) == 0
    assert not _np(upd).any()
    assert L._lib.bgamd_td_fit_step(L._h, None, None, 0, FR.ALPHA, None, L._s()) == 0
    L.fit_step(torch.zeros((0, 8), dtype=torch.int32), torch.zeros(0))
    assert np.array_equal(_np(L.theta), N.table("ckpt")) and L.fit_stats() == (0.0, 0, 0)


def test_error_codes(bg, monkeypatch):
    L = _learner(monkeypatch, "ckpt")
    rows = _rows(bg, 33)
    y = torch.zeros(33, dtype=torch.float32, device=L.device)
    f = L._lib.bgamd_td_fit_step
    assert f(L._h, L._p(rows), L._p(y), -1, FR.ALPHA, None, L._s()) == -1
    assert f(L._h, None, L._p(y), 33, FR.ALPHA, None, L._s()) == -1
    assert f(L._h, L._p(rows), None, 33, FR.ALPHA, None, L._s()) == -1
    assert f(None, L._p(rows), L._p(y), 33, FR.ALPHA, None, L._s()) == -1
    assert L._lib.bgamd_td_fit_stats(None, None, None, None) == -1
    assert L._lib.bgamd_td_fit_step_allreduce(L._h, L._p(rows), L._p(y), 33, FR.ALPHA, L._s()) == -1       # no communicator
    h = ctypes.c_void_p()
    assert L._lib.bgamd_td_create(ctypes.byref(h), 8, L.device.index or 0) == 0
    assert f(h, L._p(rows), L._p(y), 33, FR.ALPHA, None, L._s()) == -6                                       # BGAMD_E_NOWEIGHTS
    assert L._lib.bgamd_td_destroy(h) == 0
    assert np.array_equal(_np(L.theta), N.table("ckpt"))
    with pytest.raises(ValueError):
        L.fit_step(rows, y[:5])


@pytest.mark.parametrize("net", ("ckpt", "normal"))
def test_two_halves_then_apply(bg, monkeypatch, net):
    """The multi-rank route on one GPU: the two halves of a batch handed out, summed, bgamd_td_apply -- the whole batch's update in
    another order: one addition more than the longer half's chain."""
    n, tset = 257, "uniform"
    ref = FR.reference(net, n, tset)
    L = _learner(monkeypatch, net)
    rows, y = _rows(bg, n), FR.targets(net, n, tset)
    a, b = _step(L, rows[:128], y[:128]), _step(L, rows[128:].contiguous(), y[128:])
    s = torch.from_numpy(a + b).to(L.device)
    L._capi.check(L._lib.bgamd_td_apply(L._h, L._p(s), L._s()), "td_apply")
    bound = ref.base + (max(FR.chain(128), FR.chain(129)) + 1) * 2.0 ** -24 * ref.absterm
    th0, th1 = N.table(net).astype(np.float64), _np(L.theta)
    _within(th1, th0 + ref.update, bound + 2.0 ** -24 * np.maximum(np.abs(th0), np.abs(th1)), "%s, two halves" % net)


@pytest.mark.parametrize("net", ("ckpt", "normal"))
def test_binary_targets_are_the_td_route(bg, monkeypatch, net):
    """targets in {0, 1}: one fit step against one bgamd_td_step(t = 0) over a T = 1 log of the same rows with p1_won = the targets --
    the same update by the learner's trace kernels, within the two bounds summed (the TD route's batch sum: a chain of n at most)."""
    n = 257
    rows = _rows(bg, n)
    y = (np.arange(n) % 3 != 1).astype(np.float32)
    ref = FR.reference_at(N.reference_table(net), FR.features(n), y)
    L = _learner(monkeypatch, net, max_games=n)
    fit = _step(L, rows, y)
    log = rows.reshape(1, n, 8).contiguous()
    order = torch.arange(n, dtype=torch.int32, device=L.device)
    lengths = torch.ones(n, dtype=torch.int32, device=L.device)
    won = torch.as_tensor(y.astype(np.uint8), device=L.device)
    chk, lib = L._capi.check, L._lib
    chk(lib.bgamd_td_begin(L._h, L._p(log), 1, n, L._p(order), n, L._p(lengths), L._p(won), L._s()), "td_begin")
    upd = torch.zeros(N.N_PARAMS, dtype=torch.float32, device=L.device)
    chk(lib.bgamd_td_step(L._h, 0, n, FR.ALPHA, LR.LAM, L._p(upd), L._s()), "td_step")
    td = _np(upd)
    _within(fit, td.astype(np.float64), 2 * ref.base + (FR.chain(n) + n) * 2.0 ** -24 * ref.absterm, "%s, fit step against TD route" % net)


def _td_step0(net_theta64):
    """float64 reference of step 0 of the lock-step replay of learner_ref.log() from the given weights -> (update, bound)"""
    st, tu, ln, won = LR.log()
    X = LR.encode(st, tu)
    idx = np.nonzero(ln > 0)[0]
    ones = np.ones(len(idx), bool)
    u, _, _, b = LR.step_reference(net_theta64, LR.new_traces(len(idx)), X[0, idx], X[1, idx], ones, ln[idx] == 1, won[idx].astype(np.float64),
                                   ones, LR.ALPHA * LR.BATCH_SCALE, LR.LAM)
    return u, b, idx


@pytest.mark.parametrize("route", ("valu", "direct_slice"))
def test_td_replay_after_a_fit_step_runs_on_the_new_weights(bg, monkeypatch, route):
    """After an applied fit step, step 0 of a fresh lock-step replay matches the float64 reference evaluated from the UPDATED weights:
    the forward pass of route `valu` reads the transposed copy w1t, that of `direct_slice` the bf16 planes wl3 -- a stale copy leaves
    the bound (checked here on the reference: from the old weights it is more than 10 bounds away)."""
    env = {"valu": {}, "direct_slice": {"BGAMD_TD_DIRECT_MIN": "1", "BGAMD_TD_FUSE_STEP": "0"}}[route]
    L = _learner(monkeypatch, "ckpt", max_games=160, env=env)
    n = 257
    _step(L, _rows(bg, n), FR.targets("ckpt", n, "uniform"), alpha=0.1, hand_out=False)
    th1 = _np(L.theta)
    assert np.abs(th1 - N.table("ckpt")).max() > 1e-3
    want, bound, idx = _td_step0(th1.astype(np.float64))
    stale, _, _ = _td_step0(N.table("ckpt").astype(np.float64))
    assert (np.abs(stale - want) > 10 * bound).any()
    st, tu, ln, won = LR.log()
    rows = bg.pack_rows(st, tu).contiguous()
    lengths = torch.as_tensor(ln).to(torch.int32).to(L.device).contiguous()
    sl, order = torch.sort(lengths, descending=True, stable=True)
    order = order[:len(idx)].to(torch.int32).contiguous()
    p1 = torch.as_tensor(won).to(torch.uint8).to(L.device).contiguous()
    chk, lib = L._capi.check, L._lib
    chk(lib.bgamd_td_begin(L._h, L._p(rows), int(rows.shape[0]), int(rows.shape[1]), L._p(order), len(idx), L._p(lengths), L._p(p1), L._s()),
        "td_begin")
    upd = torch.zeros(N.N_PARAMS, dtype=torch.float32, device=L.device)
    chk(lib.bgamd_td_step(L._h, 0, len(idx), LR.ALPHA * LR.BATCH_SCALE, LR.LAM, L._p(upd), L._s()), "td_step")
    _within(_np(upd), want, bound, "TD step after a fit step, " + route)


def test_fit_step_leaves_a_finished_replay_as_it_was(bg, monkeypatch):
    """bgamd_td_stats, bgamd_td_slots and the column counters of a finished replay read the same before and after a fit step"""
    L = _learner(monkeypatch, "ckpt", max_games=160)
    st, tu, ln, won = LR.log()
    L.replay_rows(bg.pack_rows(st, tu).contiguous(), ln, won, batch_scale=LR.BATCH_SCALE, slots=LR.SLOTS)
    C, lib, chk = L._C, L._lib, L._capi.check

    def read():
        sq, cnt, a, w = C.c_double(), C.c_int64(), C.c_uint64(), C.c_uint64()
        slots = np.zeros((160, 6), np.int32)
        chk(lib.bgamd_td_stats(L._h, C.byref(sq), C.byref(cnt)), "td_stats")
        chk(lib.bgamd_td_slots(L._h, slots.ctypes.data), "td_slots")
        chk(lib.bgamd_td_active_columns(L._h, C.byref(a)), "td_active_columns")
        chk(lib.bgamd_td_written_columns(L._h, C.byref(w)), "td_written_columns")
        return sq.value, cnt.value, a.value, w.value, slots.tobytes()
    before = read()
    assert before[1] == int(ln.sum()) and before[2] > 0
    th = _np(L.theta)
    _step(L, _rows(bg, 257), FR.targets("ckpt", 257, "uniform"), hand_out=False)
    assert not np.array_equal(_np(L.theta), th)
    assert read() == before


def test_fit_against_the_host_learner(bg, monkeypatch):
    """DeviceTDLambdaLearner.fit, two epochs at batch 256 over 1 000 rows, against the float64 host learner driven with the same batches
    (fit_batches): the final weights within the bounds of the eight steps added up -- each step's bound from the float64 reference at the
    host learner's weights of that step, plus the rounding of each θ + update.  (The bound is first order in the errors of one step from
    the same weights; for the checkpoint plain float32 uses 0.5 % of it, tests/fit_ref.py RESTATED, which leaves the room the gathered
    difference of the weights needs.)"""
    from backgammon_env.learner import TDLambdaLearner, fit_batches
    n, batch, epochs, seed = 1000, 256, 2, 3
    st, tu = FR.positions(n)
    y = FR.targets("ckpt", n, "uniform")
    X = FR.features(n)
    L = _learner(monkeypatch, "ckpt")
    mse = L.fit(st, tu, y, epochs=epochs, batch=batch, seed=seed)
    H = TDLambdaLearner(N.table("ckpt"), dtype=torch.float64, alpha=LR.ALPHA)
    total, sq, sq_tol, k = np.zeros(N.N_PARAMS), [0.0] * epochs, [0.0] * epochs, 0
    for e, idx in fit_batches(n, epochs, batch, seed):
        i = idx.numpy()
        ref = FR.reference_at(H.theta.numpy(), X[i], y[i], LR.ALPHA * 24.0 / batch)
        total += FR.bound(ref, len(i)) + 2.0 ** -24 * (np.abs(H.theta.numpy()) + np.abs(ref.update))
        sq[e] += H.fit_step(torch.from_numpy(X[i]), torch.from_numpy(y[i]), batch_scale=24.0 / batch)[0]
        sq_tol[e] += FR.sq_bound(ref)
        k += 1
    assert k == 8 and len(mse) == epochs
    _within(_np(L.theta), H.theta.numpy(), total, "fit, two epochs of four batches")
    for e in range(epochs):
        assert abs(mse[e] - sq[e] / n) <= sq_tol[e] / n, (e, mse[e], sq[e] / n)       # Σ δ² of values within V = 1e-5, step by step
    assert mse[1] < mse[0]


def test_world_of_one_collective(bg, monkeypatch):
    """fit_step through the library's own all-reduce on a communicator of ONE rank (bgamd_td_fit_step_allreduce: fit step handed out ->
    ncclAllReduce -> bgamd_td_apply) ends on the weights of the local route, bit for bit"""
    n = 257
    rows, y = _rows(bg, n), FR.targets("ckpt", n, "uniform")
    A = _learner(monkeypatch, "ckpt")
    A.fit_step(rows, y, batch_scale=LR.BATCH_SCALE)
    B = _learner(monkeypatch, "ckpt")
    B.init_collective()
    monkeypatch.setenv("BGAMD_FORCE_COLLECTIVE", "1")
    B.fit_step(rows, y, batch_scale=LR.BATCH_SCALE)
    monkeypatch.delenv("BGAMD_FORCE_COLLECTIVE")
    assert torch.equal(A.theta, B.theta) and A.fit_stats() == B.fit_stats()
    assert not np.array_equal(_np(A.theta), N.table("ckpt"))


def test_example_runs_to_its_last_line():
    """examples/rollout_fit.py at a toy size in a child process: it prints `done`, and the held-out error after the fit is finite"""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "rollout_fit.py"), "--games", "256", "--positions", "48", "--trials", "36",
           "--turn-limit", "4", "--epochs", "2", "--batch", "16", "--arena", "64", "--max-plies", "200"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "done", out.stdout
    m = re.search(r"held-out mse after the fit: (\S+)", out.stdout)
    assert m and np.isfinite(float(m.group(1))) and float(m.group(1)) >= 0, out.stdout
    assert re.search(r"held-out mse before the fit: (\S+)", out.stdout) and "health:" in out.stdout
