"""float64 numpy references for the net health check and the choice spread (tests/test_health_cpu.py, tests/test_gpu_health.py).
A helper module like tests/nets.py: functions of a table and a row set, nothing read from outside tests/golden.

The device forms a = fc1.weight x + fc1.bias as an fp32 FMA chain of 198 products plus one add.  Against the exact sum its error is at
most  m = 200 * 2^-24 * (|b1| + sum_i |w_i x_i|)  for that (row, unit) pair (199 roundings, (1 + u)^199 - 1 < 200 u; derived, not
tuned).  A pair whose exact |a| is further than m above the threshold is SURELY counted, one within m of it is UNDECIDED, so every
count of the device lies in [sure, sure + undecided]."""
import numpy as np

import nets as N

U = 2.0 ** -24
THRESHOLDS = (15.0, 1.0)             # the verdict's threshold, and one that the healthy nets cross too (so that their counts are not all 0)
W_INDICES = (0, 25343, 25344, 25471, 25472, 25599, 25600)       # first and last element of fc1.weight, fc1.bias, fc2.weight, fc2.bias
BELOW = float(np.nextafter(np.float32(65504.0), np.float32(0)))
SPECIALS = (np.nan, np.inf, -np.inf, 65504.0, -65504.0, BELOW, -BELOW)


def split(theta):
    w = np.asarray(theta)
    return w[:N.O1].reshape(N.N_HID, N.N_IN), w[N.O1:N.O2], w[N.O2:N.O3], w[N.O3]


def weights_ref(theta):
    """-> nonfinite, max_abs [4] float32 (largest finite |w| per tensor, 0 if none), fits_f16_split: the acceptance test of
    bgamd_weights_check restated -- every weight finite; fc1.weight (columns 196 / 197 divided by 15 in fp32, as the root pass folds
    the 1/15 of the borne-off features into them) below 65 504 in magnitude and reproduced by f16 hi + f16 lo to 2^-21 |w| + 2^-24."""
    w = np.asarray(theta, np.float32)
    fin = np.isfinite(w)
    mx = np.zeros(4, np.float32)
    for k, (a, b) in enumerate(((0, N.O1), (N.O1, N.O2), (N.O2, N.O3), (N.O3, N.N_PARAMS))):
        t = np.abs(w[a:b][fin[a:b]])
        mx[k] = t.max() if t.size else 0
    fits = bool(fin.all())
    if fits:
        W1 = w[:N.O1].reshape(N.N_HID, N.N_IN).copy()
        W1[:, 196:] = W1[:, 196:] / np.float32(15)
        aw = np.abs(W1)
        with np.errstate(over="ignore", invalid="ignore"):
            hi = W1.astype(np.float16)
            lo = (W1 - hi.astype(np.float32)).astype(np.float16)
            res = np.abs(W1 - (hi.astype(np.float32) + lo.astype(np.float32)))
            fits = bool((aw < np.float32(65504)).all() and (res <= aw * np.float32(4.76837158e-7) + np.float32(5.96046448e-8)).all())
    return {"nonfinite": int((~fin).sum()), "max_abs": mx, "fits_f16_split": fits}


def preactivations(theta, X198):
    """-> (a64 [n, 128], m [n, 128], v64 [n], vbound [n]): the exact pre-activations, the fp32 chain's error bound per pair, the fp64 net
    output and a bound on what ANY fp32 evaluation of the net may differ from it by:
      |dh_j| <= |da_j| / 4 + 4u  (sigmoid' <= 1/4; exp, add and divide of a value in [0, 1]),
      |dz|   <= sum_j |W2_j| |dh_j| + 130 u (sum_j |W2_j h_j| + |b2|),   |dv| <= |dz| / 4 + 4u."""
    W1, b1, W2, b2 = (np.asarray(t, np.float64) for t in split(theta))
    X = np.asarray(X198, np.float64)
    a = X @ W1.T + b1
    m = 200 * U * (np.abs(X) @ np.abs(W1).T + np.abs(b1))
    with np.errstate(over="ignore"):
        h = 1.0 / (1.0 + np.exp(-a))
        v = 1.0 / (1.0 + np.exp(-(h @ W2 + b2)))
    dz = (m / 4 + 4 * U) @ np.abs(W2) + 130 * U * (h @ np.abs(W2) + abs(b2))
    return a, m, v, dz / 4 + 4 * U


def counts_ref(a, m, threshold):
    """-> dict of the sure / undecided counts over the pairs given (total and per unit), the dead-unit range and max |a| with its bound"""
    absa = np.abs(a)
    sure = absa > threshold + m
    und = np.abs(absa - threshold) <= m
    us, uu = sure.sum(0), und.sum(0)
    n = a.shape[0]
    return {"rows": n, "sure": int(sure.sum()), "undecided": int(und.sum()), "unit_sure": us, "unit_undecided": uu,
            "dead_sure": int((us == n).sum()) if n else 0, "dead_max": int((us + uu == n).sum()) if n else 0,
            "max_abs_preact": float(absa.max()) if n else 0.0, "preact_bound": float(m.max()) if n else 0.0}


def net_health_ref(theta, X198, threshold):
    a, m, v, vb = preactivations(theta, X198)
    out = counts_ref(a, m, threshold)
    out.update(weights_ref(theta))
    out.update({"v_min": float(v.min()) if len(v) else 0.0, "v_max": float(v.max()) if len(v) else 0.0})
    return out


def value_bound(theta, X198, family):
    """What tests/test_gpu_nets.py asks of `evaluate` under that net: the flat 1e-5 for the parity families; for the edge nets
    max(1e-5, 4 e32), e32 = the numpy fp32 forward pass's own largest error on these rows (test_saturated_hidden_layer)."""
    if family in N.PARITY:
        return 1e-5
    _, _, v, _ = preactivations(theta, X198)
    e32 = float(np.abs(N.forward_np32(theta, X198).astype(np.float64) - v).max())
    return max(1e-5, 4 * e32)


def injected_tables():
    """(label, table): the checkpoint with each special value at each of the four tensors' first and last elements, and two tables with
    several at once"""
    ck = N.checkpoint()
    for i in W_INDICES:
        for s in SPECIALS:
            w = ck.copy()
            w[i] = s
            yield "ckpt[%d] = %r" % (i, s), w
    w = ck.copy()
    w[[0, 5000, 25344, 25600]] = [np.nan, np.inf, -np.inf, np.nan]
    yield "four non-finite", w
    w = ck.copy()
    w[:N.O1] = np.nan
    yield "fc1.weight all NaN", w


_rows = {}


def row_sets():
    """name -> (states, turn, X198): the feature sweep (every value of every feature) and fixture G5's rows"""
    if not _rows:
        for key, (st, tu) in (("sweep", N.sweep_rows()), ("g5", N.g5_rows())):
            _rows[key] = (st, tu, N.encode(st, tu))
    return _rows


def sizes(n):
    return (1, 63, 64, 65, 257, n)          # around the 32-row tile and the 8-wave workgroup, more than one workgroup, everything


_pre = {}


def pairs(family, key):
    """preactivations(table(family), row set `key`), computed once"""
    if (family, key) not in _pre:
        _pre[(family, key)] = preactivations(N.table(family), row_sets()[key][2])
    return _pre[(family, key)]


def spread_ref(info, values, n):
    """The choice spread from the unique_rows() list: info [U, 2] (game, key | turn << 31), values float32 [U].
    -> count, best, worst, tied [n] and the four summary numbers."""
    info = np.asarray(info, np.int64)
    val = np.asarray(values, np.float32)
    count, tied = np.zeros(n, np.int32), np.zeros(n, np.int32)
    best, worst = np.zeros(n, np.float32), np.zeros(n, np.float32)
    game, mover = info[:, 0], (info[:, 1] >> 31) & 1
    for g in np.unique(game):
        sel = game == g
        v, mv = val[sel], mover[sel]
        assert (mv == mv[0]).all()
        count[g] = len(v)
        best[g], worst[g] = (v.min(), v.max()) if mv[0] else (v.max(), v.min())
        tied[g] = int((v.view(np.uint32) == best[g:g + 1].view(np.uint32)[0]).sum())
    ch = count >= 2
    return {"count": count, "best": best, "worst": worst, "tied": tied,
            "summary": [int(ch.sum()), int((ch & (tied == count)).sum()), int(count.sum()), int((count == 0).sum())]}
