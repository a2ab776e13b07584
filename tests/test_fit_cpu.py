"""The supervised step (bgamd_td_fit_step) on the CPU: the closed form against autograd, the host learner against the float64 reference of
tests/fit_ref.py, the condition the device test rests on (plain numpy float32 in the kernel's order leaves three quarters of the bound),
the negative controls, and how DeviceTDLambdaLearner.fit packs, permutes and batches."""
import numpy as np
import pytest

import fit_ref as FR
import learner_ref as LR
import nets as N

torch = pytest.importorskip("torch")


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("net", N.PARITY)
def test_reference_is_the_squared_error_gradient_step(net):
    """The float64 reference update = -alpha ∂/∂θ ½ Σ (y - V)² by torch autograd in float64, 1e-12 of the largest entry; so is the
    vectorised closed form the negative controls are mutations of.  Rows with targets that are not finite are outside the sum."""
    n = 257
    X = FR.features(n)
    for tset in ("uniform", "nonfinite"):
        y = FR.targets(net, n, tset)
        ref = FR.reference(net, n, tset)
        th = torch.tensor(N.reference_table(net).astype(np.float64), requires_grad=True)
        fin = np.isfinite(y)
        x = torch.tensor(X[fin].astype(np.float64))
        h = torch.sigmoid(x @ th[:N.O1].reshape(N.N_HID, N.N_IN).T + th[N.O1:N.O2])
        v = torch.sigmoid(h @ th[N.O2:N.O3] + th[N.O3])
        loss = 0.5 * ((torch.tensor(y[fin].astype(np.float64)) - v) ** 2).sum()
        loss.backward()
        want = -FR.ALPHA * th.grad.numpy()
        assert _rel(ref.update, want) <= 1e-12, (net, tset, _rel(ref.update, want))
        assert _rel(FR.closed_form(N.reference_table(net), X, y), want) <= 1e-12
        assert ref.rows == fin.sum() and ref.skipped == (~fin).sum()


@pytest.mark.parametrize("net", N.PARITY)
def test_host_learner(net):
    """TDLambdaLearner.fit_step: float64 at 1e-12 of the reference, float32 within the bound; Σ δ² and the counts."""
    from backgammon_env.learner import TDLambdaLearner
    n = 257
    X = FR.features(n)
    for tset in FR.TARGET_SETS:
        y = FR.targets(net, n, tset)
        ref = FR.reference(net, n, tset)
        th0 = N.reference_table(net)
        L = TDLambdaLearner(th0, dtype=torch.float64, alpha=LR.ALPHA)
        sq, rows, skipped = L.fit_step(torch.from_numpy(X), torch.from_numpy(y), batch_scale=LR.BATCH_SCALE)
        got = L.theta.numpy() - th0.astype(np.float64)
        assert np.abs(got - ref.update).max() <= 1e-12 * max(np.abs(ref.update).max(), np.abs(th0).max()), (net, tset)
        assert (rows, skipped) == (ref.rows, ref.skipped) and abs(sq - ref.sq) <= 1e-12 * max(ref.sq, 1.0)
        L = TDLambdaLearner(th0, dtype=torch.float32, alpha=LR.ALPHA)
        sq, rows, skipped = L.fit_step(torch.from_numpy(X), torch.from_numpy(y), batch_scale=LR.BATCH_SCALE)
        th1 = L.theta.numpy().astype(np.float64)
        slack = 2.0 ** -24 * np.maximum(np.abs(th0), np.abs(th1))          # θ + update rounds once more
        d = np.abs(th1 - (th0.astype(np.float64) + ref.update))
        assert (d <= FR.bound(ref, n) + slack).all(), (net, tset, float((d / (FR.bound(ref, n) + slack + 1e-300)).max()))
        assert abs(sq - ref.sq) <= FR.sq_bound(ref) and (rows, skipped) == (ref.rows, ref.skipped)


def _cases(family):
    out = []
    for config, sizes in FR.CONFIG_SIZES.items():
        for n in sizes:
            if family != "ckpt" and n not in FR.FAMILY_SIZES:
                continue
            out += [(config, n, tset) for tset in FR.TARGET_SETS]
    if family == "ckpt":
        out.append(("default", FR.LARGE, "uniform"))
    return out


@pytest.mark.parametrize("family", N.PARITY + ("zero_w1",))
def test_float32_restatement_leaves_three_quarters_of_the_bound(family):
    """The condition tests/test_gpu_fit.py rests on: plain numpy float32, rows summed in the kernel's documented order, stays within a
    quarter of the bound for every (family, target set, size, configuration) the device test holds to the whole bound."""
    worst = 0.0
    for config, n, tset in _cases(family):
        ref = FR.reference(family, n, tset)
        upd, sq = FR.restated_f32(N.table(family), FR.features(n), FR.targets(family, n, tset), config=config)
        b = FR.bound(ref, n, config)
        d = np.abs(upd.astype(np.float64) - ref.update)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.where(d > 0, d / b, 0.0).max())
        assert (d <= 0.25 * b).all(), (family, config, n, tset, r)
        assert abs(sq - ref.sq) <= 0.25 * FR.sq_bound(ref) + 1e-300, (family, config, n, tset)
        worst = max(worst, r)
    print("%s: worst float32 restatement / bound = %.4f (recorded: %.4f)" % (family, worst, FR.RESTATED[family]))
    assert worst <= FR.RESTATED[family] * 1.05, "fit_ref.RESTATED no longer describes the code: record %.4f" % worst


def test_chain_rule():
    """C(n) as csrc/bg_fit.h states it"""
    assert FR.chain(1) == FR.chain(32) == 32 + 1 + 16
    assert FR.chain(33) == 32 + 1 + 16 and FR.chain(8192) == 32 + 16 + 16 and FR.chain(8193) == 64 + 16 + 16
    assert FR.chain(65536) == 256 + 16 + 16 and FR.chain(65537) == 256 + 16 + 16 + 1
    assert FR.chain(1061, "chunk512") == 32 + 1 + 16 + 2 and FR.chain(1061, "groups3") == 12 * 32 + 1 + 16
    assert FR.chain(1061, "chunk512_groups3") == 6 * 32 + 1 + 16 + 2 and FR.chain(0) == 0


@pytest.mark.parametrize("net", N.PARITY)
def test_negative_controls(net):
    """Every deliberately wrong reference differs from the true one by at least 10 x the bound in some parameter, on inputs of the device
    test (257 rows; the targets that are not finite for the control that is about them)."""
    n = 257
    th = N.reference_table(net)
    for mutate in FR.MUTATIONS:
        tset = "nonfinite" if mutate == "nonfinite_zero" else "uniform"
        y = FR.targets(net, n, tset)
        ref = FR.reference(net, n, tset)
        wrong = FR.closed_form(th, FR.features(n, "off16" if mutate == "off16" else None), y, mutate=mutate)
        d = np.abs(wrong - ref.update)
        b = FR.bound(ref, n)
        hit = (d >= 10 * b) & (d > 0)
        assert hit.any(), (net, mutate, float((d / np.maximum(b, 1e-300)).max()))


class _Recorder:
    """DeviceTDLambdaLearner.fit without a device: the three methods it calls record what they are handed"""
    def __new__(cls):
        from backgammon_env.learner import DeviceTDLambdaLearner

        class R(DeviceTDLambdaLearner):
            def __init__(self):
                self.device, self.learning_rate, self.steps, self.packed = torch.device("cpu"), 0.1, [], 0

            def __del__(self):
                pass

            def _pack_rows(self, states28, turn):
                self.packed += 1
                st = torch.as_tensor(states28, dtype=torch.int32)
                return torch.cat([st[:, :7], torch.as_tensor(turn, dtype=torch.int32)[:, None]], 1)

            def fit_step(self, rows, targets, alpha=None, batch_scale=1.0, group=None):
                self.steps.append((rows.clone(), targets.clone(), alpha, batch_scale))

            def fit_stats(self):
                done, self.seen = len(self.steps) - getattr(self, "seen", 0), len(self.steps)
                return 2.0 * done, 4 * done, 0
        return R()


def test_fit_packs_permutes_and_batches():
    from backgammon_env.learner import fit_batches
    n, batch, seed = 1000, 256, 5
    st = np.arange(n * 28, dtype=np.int32).reshape(n, 28)
    tu = (np.arange(n) % 2).astype(np.int32)
    y = np.linspace(0, 1, n).astype(np.float32)
    R = _Recorder()
    mse = R.fit(st, tu, y, epochs=2, batch=batch, seed=seed)
    assert R.packed == 1 and len(R.steps) == 8 and mse == [0.5, 0.5]
    packed = R._pack_rows(st, tu)
    for e in range(2):
        g = torch.Generator(device="cpu")
        g.manual_seed(seed + e)
        perm = torch.randperm(n, generator=g)
        assert sorted(perm.tolist()) == list(range(n))
        steps = R.steps[4 * e:4 * e + 4]
        assert [len(s[0]) for s in steps] == [256, 256, 256, 232]                 # the last batch is short
        assert torch.equal(torch.cat([s[0] for s in steps]), packed[perm])
        assert torch.equal(torch.cat([s[1] for s in steps]), torch.from_numpy(y)[perm])
        assert all(s[2] is None and s[3] == 24.0 / batch for s in steps)           # the default batch_scale
    assert [(e, i.tolist()) for e, i in fit_batches(5, 2, 2, 1)] == [
        (e, torch.randperm(5, generator=torch.Generator().manual_seed(1 + e))[b:b + 2].tolist()) for e in range(2) for b in (0, 2, 4)]
    R = _Recorder()
    R.fit(st, tu, y, epochs=1, batch=4096, seed=0, alpha=0.05, batch_scale=0.5)
    assert len(R.steps) == 1 and R.steps[0][2:] == (0.05, 0.5) and len(R.steps[0][0]) == n
