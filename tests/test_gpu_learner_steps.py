"""EVERY update of the HIP TD(λ) learner against the float64 step reference of tests/learner_ref.py, within its per-parameter bound
(whose conditions tests/test_learner_steps_cpu.py states): the 25 601-float update bgamd_td_step hands out is read after every step, on
a 160-game log that reaches every value of every feature, under the seven parity families of tests/nets.py, on every kernel route of
bgamd_td_step, lock-step, streamed through 7 slots and over a ring log, at λ = 0, 2^-2, 0.7 and 1.

The device replays run free: every step's own update goes through bgamd_td_apply.  The bound is first order in the errors of one step
from the SAME weights and has no term for the rounding the float32 weights gather from step to step; for the (family, mode) pairs of
learner_ref.NARROWED, where that rounding alone leaves the bound for plain numpy float32 (tests/test_learner_steps_cpu.py), the float64
reference is evaluated AT the weights the device went through -- its traces, δ and updates remain its own, so nothing the device
computed in a step enters what that step is compared with."""
import numpy as np
import pytest

import learner_ref as LR
import nets as N
from learner_routes import ROUTES, _VARS
from test_gpu_parity import _np

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_FAMILY_ROUTE = [(f, r) for f in N.PARITY for r in ROUTES]     # family-major: the routes of a family share its cached reference


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


# ---- the log on the device --------------------------------------------------------------------------------------------------------

_dev = {}


def _rows(bg, ring):
    """-> the packed log [T, 160, 8] (or the ring [T + 5, 160, 8]); once, encode_rows(pack_rows(...)) is held against the oracle"""
    if ring not in _dev:
        if ring:
            st, tu, _, _ = LR.ring_layout()
        else:
            st, tu, _, _ = LR.log()
        rows = bg.pack_rows(st, tu).contiguous()
        X = _np(bg.VecGame(1).encode_rows(rows))
        assert np.array_equal(X, N.encode(st.reshape(-1, 28), tu.reshape(-1)).reshape(tu.shape + (N.N_IN,)))
        _dev[ring] = rows
    return _dev[ring]


def _learner(monkeypatch, route, family, lam=LR.LAM, alpha=LR.ALPHA, dense=False):
    from backgammon_env.learner import DeviceTDLambdaLearner
    for k in _VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    if dense:
        monkeypatch.setenv("BGAMD_TD_DENSE", "1")
    return DeviceTDLambdaLearner(N.table(family), max_games=160, alpha=alpha, lam=lam)


class Device:
    """updates [n_steps, 25601] float32, weights [n_steps, 25601] the weights every step started from, theta: after the last step"""


def stepwise(bg, L, mode, batch_scale=LR.BATCH_SCALE):
    """The replay of the 160-game log through the entry points DeviceTDLambdaLearner calls, one step at a time: bgamd_td_begin /
    bgamd_td_begin_stream / bgamd_td_begin_stream_games, then per step bgamd_td_step into a device buffer, a copy of it, and
    bgamd_td_apply of the same buffer."""
    C, lib, chk = L._C, L._lib, L._capi.check
    _, _, ln, p1 = LR.log()
    rows = _rows(bg, mode == "ring")
    T, n = int(rows.shape[0]), int(rows.shape[1])
    lengths = torch.as_tensor(ln).to(torch.int32).to(L.device).contiguous()
    won = torch.as_tensor(p1).to(torch.uint8).to(L.device).contiguous()
    if mode == "lockstep":
        sl, order = torch.sort(lengths, descending=True, stable=True)
        n_games = int((sl > 0).sum().item())
        order = order[:n_games].to(torch.int32).contiguous()
        n_steps = int(sl[0].item())
        n_active = [int((sl > t).sum().item()) for t in range(n_steps)]
        keep = (order,)
        chk(lib.bgamd_td_begin(L._h, L._p(rows), T, n, L._p(order), n_games, L._p(lengths), L._p(won), L._s()), "td_begin")
    else:
        game, _, queue, qoff = LR.schedule(ln, LR.SLOTS)
        h_len = np.ascontiguousarray(ln, np.int32)
        h_queue, h_qoff = np.zeros(n, np.int32), np.zeros(LR.SLOTS + 1, np.int32)
        ng, nst = C.c_int64(), C.c_int64()
        chk(lib.bgamd_td_stream_schedule(h_len.ctypes.data, n, LR.SLOTS, h_queue.ctypes.data, h_qoff.ctypes.data, C.byref(ng), C.byref(nst)),
            "td_stream_schedule")
        assert int(nst.value) == len(game) and np.array_equal(h_queue[:int(ng.value)], queue) and np.array_equal(h_qoff, qoff)
        n_steps, n_active = len(game), [LR.SLOTS] * len(game)
        dq, do = torch.from_numpy(h_queue[:int(ng.value)].copy()).to(L.device), torch.from_numpy(h_qoff).to(L.device)
        if mode == "streamed":
            keep = (dq, do)
            chk(lib.bgamd_td_begin_stream(L._h, L._p(rows), T, n, L._p(dq), L._p(do), LR.SLOTS, L._p(lengths), L._p(won), L._s()),
                "td_begin_stream")
        else:
            _, _, lane, start = LR.ring_layout()
            dl, ds = torch.from_numpy(lane.copy()).to(L.device), torch.from_numpy(start.copy()).to(L.device)
            keep = (dq, do, dl, ds)
            chk(lib.bgamd_td_begin_stream_games(L._h, L._p(rows), T, n, L._p(dq), L._p(do), LR.SLOTS, n, L._p(dl), L._p(ds), L._p(lengths),
                                                L._p(won), L._s()), "td_begin_stream_games")
    alpha, lam = float(L.learning_rate) * float(batch_scale), float(L.lambda_decay)
    upd = torch.zeros(N.N_PARAMS, dtype=torch.float32, device=L.device)
    ups = torch.empty((n_steps, N.N_PARAMS), dtype=torch.float32, device=L.device)
    ths = torch.empty((n_steps, N.N_PARAMS), dtype=torch.float32, device=L.device)
    for t in range(n_steps):
        chk(lib.bgamd_td_get_weights(L._h, L._p(ths[t]), L._s()), "td_get_weights")
        chk(lib.bgamd_td_step(L._h, t, n_active[t], alpha, lam, L._p(upd), L._s()), "td_step")
        ups[t].copy_(upd)
        chk(lib.bgamd_td_apply(L._h, L._p(upd), L._s()), "td_apply")
    sq, cnt = C.c_double(), C.c_int64()
    chk(lib.bgamd_td_stats(L._h, C.byref(sq), C.byref(cnt)), "td_stats")
    out = Device()
    out.updates, out.weights, out.theta, out.sq, out.count = _np(ups), _np(ths), _np(L.theta), float(sq.value), int(cnt.value)
    del keep
    return out


# ---- the comparison ---------------------------------------------------------------------------------------------------------------

def _ratio(dev_updates, ref_updates, bounds, label):
    """max |device - reference| / bound over every step and parameter; the assertion is elementwise |d| <= bound"""
    d = np.abs(dev_updates.astype(np.float64) - ref_updates)
    over = d > bounds
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d > 0, d / bounds, 0.0)
    s, p = np.unravel_index(int(np.argmax(r)), r.shape)
    worst = float(r[s, p])
    print("%s: worst device / bound = %.4f (step %d, %s)" % (label, worst, s, LR.where(p)))
    assert not over.any(), "%s: %d updates outside the bound; the worst at step %d, %s: |d| = %.3g = %.3g x the bound %.3g" % (
        label, int(over.sum()), s, LR.where(p), d[s, p], worst, bounds[s, p])
    return worst


def _against_fp64(family, route, mode, lam, dev, reset_every_step=False):
    label = "%s, %s, %s, lambda %g" % (family, route, mode, lam)
    mode = "streamed" if mode == "ring" else mode       # the ring holds the same replay (tests/test_learner_steps_cpu.py)
    ref = LR.replay(family, mode=mode, lam=lam)
    assert dev.updates.shape == ref.updates.shape
    upd_ref = ref.updates
    if (family, mode, lam) in LR.NARROWED:
        d = np.abs(dev.updates - ref.updates)
        print("%s: running free against the cached reference: %.4f of the bound" % (
            label, float((d / np.maximum(ref.bounds, np.float32(1e-37))).max())))
        upd_ref = LR.replay(family, mode=mode, lam=lam, weights=dev.weights, bound=False).updates
    _ratio(dev.updates, upd_ref, ref.bounds, label)
    if reset_every_step:         # λ = 0: also the replay whose traces are zeroed at every step
        _ratio(dev.updates, LR.replay(family, mode=mode, lam=lam, reset_every_step=True, bound=False).updates, ref.bounds, label + ", traces zeroed")
    _, _, ln, _ = LR.log()
    assert dev.count == ref.count == int(ln.sum())
    assert abs(dev.sq - ref.sq) <= 1e-4 * ref.sq, (label, dev.sq, ref.sq)
    # the final weights: θ0 + Σ reference updates, within the summed bounds -- and, the device's θ being float32, half an ulp of it
    # for every bgamd_td_apply that changed the parameter
    theta0 = N.table(family).astype(np.float64)
    d = np.abs(dev.theta - (theta0 + upd_ref.sum(0)))
    total = ref.bounds.sum(0, dtype=np.float64)
    rounding = (dev.updates != 0).sum(0) * 2.0 ** -24 * np.maximum(np.abs(theta0), np.abs(dev.theta))
    p = int(np.argmax(d / np.maximum(total + rounding, 1e-300)))
    print("%s: final weights: worst |d| / (summed bounds + rounding) = %.4f, / summed bounds alone = %.4g (%s)" % (
        label, d[p] / max(total[p] + rounding[p], 1e-300), float((d / np.maximum(total, 1e-300)).max()), LR.where(p)))
    assert (d <= total + rounding).all(), (label, LR.where(p), d[p], total[p], rounding[p])


@pytest.mark.parametrize("family,route", _FAMILY_ROUTE)
def test_every_step_against_fp64(bg, monkeypatch, family, route):
    """lock-step, α = 0.1, batch_scale = 0.25, λ = 0.7: every step's update within the bound of the float64 reference, elementwise; at
    the end the count, Σ δ² (1e-4 relative) and the final weights within the summed bounds."""
    L = _learner(monkeypatch, route, family)
    _against_fp64(family, route, "lockstep", LR.LAM, stepwise(bg, L, "lockstep"))


@pytest.mark.parametrize("family,route", _FAMILY_ROUTE)
def test_every_step_streamed(bg, monkeypatch, family, route):
    """the same through 7 slots (bgamd_td_begin_stream): slots take their next games while the lazy scale is away from 1"""
    L = _learner(monkeypatch, route, family)
    _against_fp64(family, route, "streamed", LR.LAM, stepwise(bg, L, "streamed"))


@pytest.mark.parametrize("family", ("ckpt", "normal"))
@pytest.mark.parametrize("route", ("valu", "direct_pipe", "fused_g16"))
def test_every_step_over_a_ring_log(bg, monkeypatch, family, route):
    """the games in a ring of T + 5 rows, more than a third of them wrapping, through a game table (bgamd_td_begin_stream_games)"""
    L = _learner(monkeypatch, route, family)
    _against_fp64(family, route, "ring", LR.LAM, stepwise(bg, L, "ring"))


@pytest.mark.parametrize("lam,family,route", [(l, f, r) for l in (0.0, 0.25, 1.0) for f in ("ckpt", "normal") for r in ROUTES])
def test_lambda_edges(bg, monkeypatch, lam, family, route):
    """λ = 0 (every step an ordinary pass with emul = 0), 2^-2 (the scale reaches 2^-40, the inclusive end of the lazy range, and folds
    back on the next step, twice within the log) and 1 (the scale never moves): ckpt and normal, lock-step and streamed, the same bound."""
    for mode in ("lockstep", "streamed"):
        L = _learner(monkeypatch, route, family, lam=lam)
        _against_fp64(family, route, mode, lam, stepwise(bg, L, mode), reset_every_step=lam == 0.0)


@pytest.mark.parametrize("route", tuple(ROUTES))
def test_sparse_equals_dense_at_every_step(bg, monkeypatch, route):
    """BGAMD_TD_DENSE=1 (every column active from the first step) against the column-sparse default: every step's update to the bit, on
    a log whose columns switch on late, off and on again."""
    for family in ("ckpt", "normal", "loguniform"):
        for mode in ("lockstep", "streamed"):
            a = stepwise(bg, _learner(monkeypatch, route, family), mode)
            b = stepwise(bg, _learner(monkeypatch, route, family, dense=True), mode)
            same = (a.updates == b.updates).all(1)
            assert same.all(), (family, mode, "first differing step", int(np.argmin(same)))
            assert np.array_equal(a.theta, b.theta) and a.sq == b.sq


@pytest.mark.parametrize("family", N.PARITY)
def test_split_route_is_the_fused_replay(bg, monkeypatch, family):
    """the step / apply route this file drives ends on the weights of replay_rows' one-call replay, bit for bit (default route)"""
    _, _, ln, p1 = LR.log()
    rows = _rows(bg, False)
    for mode, slots in (("lockstep", 0), ("streamed", LR.SLOTS)):
        dev = stepwise(bg, _learner(monkeypatch, "valu", family), mode)
        L = _learner(monkeypatch, "valu", family)
        sq, cnt = L.replay_rows(rows, ln, p1, batch_scale=LR.BATCH_SCALE, slots=slots)
        assert cnt == dev.count and np.array_equal(_np(L.theta), dev.theta), (family, mode)


def test_edge_nets(bg, monkeypatch):
    """out_hi / out_lo: v is exactly 1 / 0, so g = v(1 - v) is exactly 0: every update is exactly zero, the weights stay to the bit and
    Σ δ² counts the terminal steps whose winner the net denies.  zero_w1: under the bound.  w1_x64: finite only -- the hidden layer
    overflows there and the float32 condition of tests/test_learner_steps_cpu.py does not hold, so no bound is claimed.  α = 0: the
    weights stay to the bit."""
    _, _, ln, p1 = LR.log()
    for family, lost in (("out_hi", ~p1), ("out_lo", p1)):
        for mode in ("lockstep", "streamed"):
            dev = stepwise(bg, _learner(monkeypatch, "valu", family), mode)
            assert not dev.updates.any() and np.array_equal(dev.theta, N.table(family))
            assert dev.count == ln.sum() and dev.sq == float((lost & (ln > 0)).sum()), (family, mode, dev.sq)
    for mode in ("lockstep", "streamed"):
        _against_fp64("zero_w1", "valu", mode, LR.LAM, stepwise(bg, _learner(monkeypatch, "valu", "zero_w1"), mode))
        for route in ("valu", "matrix_pipe", "fused_g16"):
            dev = stepwise(bg, _learner(monkeypatch, route, "w1_x64"), mode)
            assert np.isfinite(dev.updates).all() and np.isfinite(dev.theta).all() and dev.updates.any()
        dev = stepwise(bg, _learner(monkeypatch, "valu", "ckpt", alpha=0.0), mode)
        assert np.array_equal(dev.theta, N.table("ckpt")) and dev.count == ln.sum()
