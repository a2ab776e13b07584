"""Rows, targets, a float64 reference and a per-parameter bound for the tests of the supervised step (bgamd_td_fit_step, csrc/bg_fit.h:
tests/test_fit_cpu.py on the CPU, tests/test_gpu_fit.py on the device).  A helper module in the style of tests/learner_ref.py, not a
conftest: everything is a function of a seed and of the fixtures under tests/golden.

The step (backgammon_env/learner.py, fit_step):
    h = σ(W1 x + b1), v = σ(W2·h + b2), g = v(1-v);  ∇b2 = g, ∇W2 = g h, ∇b1 = g W2 ⊙ h ⊙ (1-h), ∇W1 = ∇b1 ⊗ x
    δ_i = y_i - v_i, update = Σ_i fp(α δ_i) ∇_i; a row whose target is not finite adds nothing
-- learner_ref.step_reference with every slot running, terminal and first and z = the targets: that function IS the float64 reference
here, called in chunks of at most 256 rows (its traces are [slots, 25601] float64), updates and bounds added up in float64.

The bound of a batch = the sum of step_reference's first-order bounds (V = 1e-5 on a value, H = 1e-5 on a hidden unit, R = 4e-6
relative) + one term for the batch sum in float32,
    C · 2^-24 · Σ_i |α δ_i| |∇_i|,
C = chain(n): the longest chain of fp32 additions into one parameter that the order of csrc/bg_fit.h makes for n rows -- a worst-case
rounding term derived from the order of the additions, not a measured number."""
import collections

import numpy as np

import learner_ref as LR
import nets as N

N_IN, N_HID, O1, O2, O3, N_PARAMS = N.N_IN, N.N_HID, N.O1, N.O2, N.O3, N.N_PARAMS
ALPHA = LR.ALPHA * LR.BATCH_SCALE            # the step's alpha (batch scale included)
V = LR.V
REF_CHUNK = 256

# the kernel's tiling (csrc/bg_fit.h): 32-row tiles, at most 256 workgroups, chunks of 65 536 rows
TILE, MAX_GROUPS, CHUNK = 32, 256, 65536

# Sizes.  Tile edges +-1 (32), two tiles (64), eight tiles = the reference's own chunk (256); 1 061: a prime, 34 workgroups, the last
# tile 5 rows; 4 099: 129 workgroups.  CONFIGS: the BGAMD_FIT_* variables bgamd_td_create reads -> what the size then reaches.
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1061)
FAMILY_SIZES = (33, 257, 1061)               # every parity family x every target set runs at these
LARGE = 4099                                 # the checkpoint, uniform targets
CONFIGS = {
    "default": {},
    # 1 061 rows = chunks of 512 + 512 + 37: the sum over chunks, a last chunk of two tiles
    "chunk512": {"BGAMD_FIT_CHUNK": "512"},
    # three workgroups: 257 rows = 9 tiles, three per workgroup; 1 061 rows = 34 tiles, 12 | 11 | 11
    "groups3": {"BGAMD_FIT_GROUPS": "3"},
    # both: chunks of 16 tiles over three workgroups (6 | 5 | 5)
    "chunk512_groups3": {"BGAMD_FIT_CHUNK": "512", "BGAMD_FIT_GROUPS": "3"},
}
CONFIG_SIZES = {"default": SIZES, "chunk512": (257, 1061), "groups3": (257, 1061), "chunk512_groups3": (1061,)}
VARS = ("BGAMD_FIT_CHUNK", "BGAMD_FIT_GROUPS")

TARGET_SETS = ("uniform", "zeros", "ones", "exact", "nonfinite")

# plain numpy float32, rows summed in the kernel's documented order, against the float64 reference: the worst |difference| / bound per
# family over every (target set, size, configuration) the device test uses (tests/test_fit_cpu.py asserts <= 0.25 and prints them).
# No input had to be dropped.
RESTATED = {"ckpt": 0.0043, "xavier": 0.0040, "ckpt_x4": 0.0439, "w1_x16": 0.0338, "normal": 0.0210, "normal_w1_x8": 0.0652,
            "loguniform": 0.0161, "zero_w1": 0.0136}

MUTATIONS = ("sign", "no_g", "mean", "off16", "drop_last", "nonfinite_zero")


def chain(n, config="default"):
    """C(n) by the rule csrc/bg_fit.h states: per chunk of m rows, tiles = ceil(m / 32), G = min(tiles, groups), a workgroup takes at
    most tpw = ceil(tiles / G) tiles -> 32 tpw additions in the workgroup, ceil(G / 16) + 16 over the workgroups; one more per chunk
    after the first."""
    env = CONFIGS[config]
    chunk = int(env.get("BGAMD_FIT_CHUNK", CHUNK))
    chunk = -(-max(chunk, TILE) // TILE) * TILE
    groups = min(max(int(env.get("BGAMD_FIT_GROUPS", MAX_GROUPS)), 1), MAX_GROUPS)
    worst, chunks = 0, 0
    for r0 in range(0, n, chunk):
        tiles = -(-min(chunk, n - r0) // TILE)
        G = min(tiles, groups)
        worst = max(worst, TILE * -(-tiles // G) + -(-G // 16) + 16)
        chunks += 1
    return worst + max(chunks - 1, 0)


def layout(n, config="default"):
    """-> per chunk (first row, rows, workgroups): what chain() is derived from, for the restatement in the kernel's order"""
    env = CONFIGS[config]
    chunk = -(-max(int(env.get("BGAMD_FIT_CHUNK", CHUNK)), TILE) // TILE) * TILE
    groups = min(max(int(env.get("BGAMD_FIT_GROUPS", MAX_GROUPS)), 1), MAX_GROUPS)
    return [(r0, min(chunk, n - r0), min(-(-min(chunk, n - r0) // TILE), groups)) for r0 in range(0, n, chunk)]


# ---- rows and targets -------------------------------------------------------------------------------------------------------------

_pool = {}


def positions(n):
    """n rows of the pool nets.sweep_rows() (every value of every feature) + nets.g5_rows(), taken with a stride of 37 (coprime to the
    pool's 3 832 rows: a short batch still meets points, bars and borne-off counters under both turn bits) -> (states [n, 28], turn [n])"""
    if "pool" not in _pool:
        a, b = N.sweep_rows(), N.g5_rows()
        st, tu = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]).astype(np.int32)
        assert np.gcd(len(st), 37) == 1
        _pool["pool"] = (st, tu)
    st, tu = _pool["pool"]
    idx = (np.arange(n) * 37) % len(st)
    return st[idx], tu[idx]


def features(n, mutate=None):
    st, tu = positions(n)
    return LR.encode(st, tu, mutate)


def values64(net, n):
    w = N.reference_table(net).astype(np.float64)
    X = features(n).astype(np.float64)
    with np.errstate(over="ignore"):
        h = 1.0 / (1.0 + np.exp(-(X @ w[:O1].reshape(N_HID, N_IN).T + w[O1:O2])))
        return 1.0 / (1.0 + np.exp(-(h @ w[O2:O3] + w[O3])))


def targets(net, n, tset):
    """float32 [n].  uniform: in [0, 1] by seed; zeros / ones; exact: the float32 value of the float64 reference (coef = 0 up to that
    rounding); nonfinite: the uniform ones with NaN at row 0, +inf at row n - 1, -inf at row n / 2 (one row: NaN)."""
    rng = np.random.RandomState(N.SEED + 31 * n + TARGET_SETS.index(tset))
    y = rng.uniform(0.0, 1.0, n).astype(np.float32)
    if tset == "zeros":
        y[:] = 0
    elif tset == "ones":
        y[:] = 1
    elif tset == "exact":
        y = values64(net, n).astype(np.float32)
    elif tset == "nonfinite":
        y[n // 2], y[n - 1], y[0] = -np.inf, np.inf, np.nan
    return y


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------

Ref = collections.namedtuple("Ref", "update base absterm delta sq rows skipped")
_refs = collections.OrderedDict()


def reference_at(theta, X, y, alpha=ALPHA):
    """learner_ref.step_reference over the rows in chunks of 256 -> Ref: the update, the summed first-order bounds, Σ_i |α δ_i| |∇_i|
    (what the batch-sum term multiplies), δ per row (0 where the target is not finite), Σ δ², rows that counted, rows skipped."""
    theta = np.asarray(theta, np.float64)
    fin = np.isfinite(y)
    z = np.where(fin, y, 0).astype(np.float64)
    upd, base, absterm, deltas = np.zeros(N_PARAMS), np.zeros(N_PARAMS), np.zeros(N_PARAMS), []
    for c0 in range(0, len(y), REF_CHUNK):
        sl = slice(c0, min(c0 + REF_CHUNK, len(y)))
        S = sl.stop - sl.start
        ones = np.ones(S, bool)
        u, tr, d, b = LR.step_reference(theta, LR.new_traces(S), X[sl], X[sl], fin[sl], ones, z[sl], ones, alpha, LR.LAM)
        upd += u
        base += b
        absterm += np.abs(alpha * d) @ tr.mag
        deltas.append(d)
    delta = np.concatenate(deltas) if deltas else np.zeros(0)
    return Ref(upd, base, absterm, delta, float((delta ** 2).sum()), int(fin.sum()), int((~fin).sum()))


def reference(net, n, tset, alpha=ALPHA):
    """the reference of (net, n rows, target set) from the net's own table; kept (read-only), the least recently used dropped"""
    key = (net, n, tset, alpha)
    if key not in _refs:
        r = reference_at(N.reference_table(net), features(n), targets(net, n, tset), alpha)
        for a in (r.update, r.base, r.absterm, r.delta):
            a.setflags(write=False)
        _refs[key] = r
        while len(_refs) > 64:
            _refs.popitem(last=False)
    _refs.move_to_end(key)
    return _refs[key]


def bound(ref, n, config="default"):
    """per parameter: the summed first-order bounds + chain(n) · 2^-24 · Σ_i |α δ_i| |∇_i|"""
    return ref.base + chain(n, config) * 2.0 ** -24 * ref.absterm


def sq_bound(ref):
    """Σ δ² of an evaluator whose values are within V: 2 V Σ|δ| + n V²"""
    return 2 * V * float(np.abs(ref.delta).sum()) + len(ref.delta) * V * V


# ---- the closed form once more, vectorised: the negative controls, and the check that it IS step_reference's update -----------------

def closed_form(theta, X, y, alpha=ALPHA, mutate=None):
    """float64.  mutate: sign (δ with the wrong sign), no_g (the factor g left out), mean (the mean instead of the sum), drop_last (the
    last row dropped), nonfinite_zero (targets that are not finite taken as 0); off16 is the caller's X."""
    w = np.asarray(theta, np.float64)
    W1, b1, W2, b2 = w[:O1].reshape(N_HID, N_IN), w[O1:O2], w[O2:O3], w[O3]
    x = np.asarray(X, np.float64)
    y = np.asarray(y, np.float64)
    if mutate == "nonfinite_zero":
        y = np.where(np.isfinite(y), y, 0.0)
    fin = np.isfinite(y)
    with np.errstate(over="ignore"):
        h = 1.0 / (1.0 + np.exp(-(x @ W1.T + b1)))
        v = 1.0 / (1.0 + np.exp(-(h @ W2 + b2)))
    delta = np.where(fin, np.where(fin, y, 0.0) - v, 0.0)
    if mutate == "sign":
        delta = -delta
    g = (np.ones_like(v) if mutate == "no_g" else v * (1 - v)) * fin
    db1 = g[:, None] * W2[None, :] * h * (1 - h)
    coef = alpha * delta
    if mutate == "mean":
        coef = coef / max(int(fin.sum()), 1)
    if mutate == "drop_last":
        coef[-1] = 0.0
    return np.concatenate([((coef[:, None] * db1).T @ x).reshape(-1), coef @ db1, (coef * g) @ h, [(coef * g).sum()]])


# ---- plain numpy float32 in the kernel's documented order ---------------------------------------------------------------------------

def restated_f32(theta, X, y, alpha=ALPHA, config="default"):
    """The step in numpy float32: every row's term in float32, summed in the order of csrc/bg_fit.h -- a workgroup's rows one after
    another (tiles b, b + G, ...), the workgroups by 16 strided sums and then those in order, the chunks one after another.  (b1 | W2
    are two half-length chains on the device; one full-length chain here: the longer one.)  -> (update float32 [25601], Σ δ²)"""
    f = np.float32
    n = len(y)
    w = np.asarray(theta, f)
    W1, b1, W2, b2 = w[:O1].reshape(N_HID, N_IN), w[O1:O2], w[O2:O3], w[O3]
    x = np.asarray(X, f)
    one = f(1)
    with np.errstate(over="ignore"):
        h = one / (one + np.exp(-(x @ W1.T + b1)))
        v = one / (one + np.exp(-(h @ W2 + b2)))
    fin = np.isfinite(y)
    delta = np.where(fin, np.where(fin, y, f(0)).astype(f) - v, f(0)).astype(f)
    coef = (alpha * delta.astype(np.float64)).astype(f)
    g = (v * (one - v) * fin).astype(f)
    db1 = ((g[:, None] * W2[None, :]) * (one - h) * h).astype(f)
    D = (coef[:, None] * db1).astype(f)
    total = None
    for r0, m, G in layout(n, config):
        tiles = -(-m // TILE)
        parts = np.zeros((G, N_PARAMS), f)
        for b in range(G):
            acc = parts[b]
            for tile in range(b, tiles, G):
                for i in range(r0 + tile * TILE, r0 + min((tile + 1) * TILE, m)):
                    acc[:O1] += (D[i][:, None] * x[i][None, :]).reshape(-1)
                    acc[O1:O2] += coef[i] * db1[i]
                    acc[O2:O3] += coef[i] * (g[i] * h[i])
                    acc[O3] += coef[i] * g[i]
        lanes = np.zeros((16, N_PARAMS), f)
        for gl in range(16):
            for b in range(gl, G, 16):
                lanes[gl] += parts[b]
        u = np.zeros(N_PARAMS, f)
        for gl in range(16):
            u += lanes[gl]
        total = u if total is None else total + u
    if total is None:
        total = np.zeros(N_PARAMS, f)
    return total, float((delta.astype(np.float64) ** 2).sum())
