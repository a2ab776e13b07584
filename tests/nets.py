"""Weight tables, references and row sets for the tests that run the value net and the move choice under MANY nets
(tests/test_nets_cpu.py, tests/test_gpu_nets.py).  A helper module, not a conftest: everything is a function of a seed and the
checkpoint fixture, nothing is read from outside tests/golden.

A table is 25 601 float32 values in the usual order: W1[128][198] | b1[128] | W2[128] | b2."""
import contextlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_IN, N_HID = 198, 128
O1, O2, O3 = N_HID * N_IN, N_HID * N_IN + N_HID, N_HID * N_IN + 2 * N_HID
N_PARAMS = O3 + 1
SEED = 20250117

# the families the project's flat 1e-5 parity bound applies to (tests/test_nets_cpu.py checks the condition it rests on)
PARITY = ("ckpt", "xavier", "ckpt_x4", "w1_x16", "normal", "normal_w1_x8", "loguniform")
# edge nets: saturation / overflow of the hidden layer, every value equal, every value exactly 1.0 or 0.0
EDGE = ("w1_x64", "zero_w1", "out_hi", "out_lo")
NAMES = PARITY + EDGE


def checkpoint():
    w = np.fromfile(os.path.join(GOLDEN, "tdgammonNEW100k.f32"), dtype=np.float32)
    assert w.size == N_PARAMS
    return w


def _normal(rng):
    return rng.standard_normal(N_PARAMS).astype(np.float32)


def _ckpt(rng, ck):
    return ck.copy()


def _xavier(rng, ck):
    """A fresh reference net: 0.1 x Xavier-uniform over (fan_in + fan_out) for both layers, biases 0."""
    w = np.zeros(N_PARAMS, np.float32)
    a1, a2 = 0.1 * np.sqrt(6.0 / (N_IN + N_HID)), 0.1 * np.sqrt(6.0 / (N_HID + 1))
    w[:O1] = rng.uniform(-a1, a1, O1)
    w[O2:O3] = rng.uniform(-a2, a2, N_HID)
    return w


def _ckpt_x4(rng, ck):
    return ck * np.float32(4)


def _w1_scaled(scale):
    def f(rng, ck):
        w = ck.copy()
        w[:O1] *= np.float32(scale)
        return w
    return f


def _normal_net(rng, ck):
    return _normal(rng)


def _normal_w1_x8(rng, ck):
    w = _normal(rng)
    w[:O1] *= np.float32(8)
    return w


def _loguniform(rng, ck):
    """|W1| log-uniform in [1e-7, 8] with a random sign: many entries whose f16 `hi` is subnormal and whose `lo` is zero."""
    w = ck.copy()
    mag = np.exp(rng.uniform(np.log(1e-7), np.log(8.0), O1))
    w[:O1] = mag * rng.choice([-1.0, 1.0], O1)
    return w


def _zero_w1(rng, ck):
    w = _normal(rng)
    w[:O1] = 0
    return w


def _out(b2):
    def f(rng, ck):
        w = _normal(rng)
        w[O3] = b2
        return w
    return f


_MAKERS = {"ckpt": _ckpt, "xavier": _xavier, "ckpt_x4": _ckpt_x4, "w1_x16": _w1_scaled(16), "normal": _normal_net,
           "normal_w1_x8": _normal_w1_x8, "loguniform": _loguniform, "w1_x64": _w1_scaled(64), "zero_w1": _zero_w1,
           "out_hi": _out(200.0), "out_lo": _out(-200.0)}
_cache = {}


def table(name, seed=SEED):
    """The table `name` for `seed` (float32 [25601], read-only: shared between the tests)."""
    key = (name, seed)
    if key not in _cache:
        w = np.ascontiguousarray(_MAKERS[name](np.random.RandomState(seed), checkpoint()), dtype=np.float32)
        assert w.shape == (N_PARAMS,)
        w.setflags(write=False)
        _cache[key] = w
    return _cache[key]


def dyadic_table(seed, n_cols=16):
    """A table under which candidates tie EXACTLY, in float32 and in fp64, in any order of summation (tests/search_model.py, the search's
    tie rules): W1 is zero except on n_cols columns drawn from features 0..191 -- the point features, whose values are 0, 1/2, 1, ... --
    with entries k / 16, k an integer in [-8, 8]; b1 of the same kind; W2 = 0.3 x normal; b2 = 0.  Every hidden pre-activation is then a
    sum of multiples of 1/32 below 2^7: exact whatever the order, so two candidates that agree on the chosen columns get the same value
    bit for bit.  Not a member of PARITY / EDGE / NAMES.  (float32 [25601], read-only and cached like table().)"""
    key = ("dyadic", seed, n_cols)
    if key not in _cache:
        rng = np.random.RandomState(seed)
        cols = np.sort(rng.choice(192, n_cols, replace=False))
        W1 = np.zeros((N_HID, N_IN), np.float32)
        W1[:, cols] = rng.randint(-8, 9, (N_HID, n_cols)).astype(np.float32) / np.float32(16)
        w = np.zeros(N_PARAMS, np.float32)
        w[:O1] = W1.ravel()
        w[O1:O2] = rng.randint(-8, 9, N_HID).astype(np.float32) / np.float32(16)
        w[O2:O3] = (0.3 * rng.standard_normal(N_HID)).astype(np.float32)
        w.setflags(write=False)
        _cache[key] = w
    return _cache[key]


def reference_table(name):
    """The table the fp64 references play with.  out_lo's fp64 values are ~1e-90 apart instead of equal -- differences no float32
    evaluator can see, yet enough for an fp64 arg-min to prefer another candidate -- so its references run with b2 = -800, where
    the fp64 forward pass gives exactly 0.0 as well; every other table stands for itself."""
    if name != "out_lo":
        return table(name)
    if ("reference", name) not in _cache:
        w = table(name).copy()
        w[O3] = -800.0
        w.setflags(write=False)
        _cache[("reference", name)] = w
    return _cache[("reference", name)]


def constant_value(w):
    """The one value c a net with W1 = 0 gives every row, in fp64."""
    w = np.asarray(w, np.float64)
    h = 1.0 / (1.0 + np.exp(-w[O1:O2]))
    return float(1.0 / (1.0 + np.exp(-(h @ w[O2:O3] + w[O3]))))


# ---- references ---------------------------------------------------------------------------------------------------------------------

def forward_np32(w, X):
    """The plain numpy float32 forward pass (what a PyTorch fp32 CPU model computes, up to summation order)."""
    w = np.asarray(w, np.float32)
    one = np.float32(1)
    with np.errstate(over="ignore"):
        h = one / (one + np.exp(-(np.asarray(X, np.float32) @ w[:O1].reshape(N_HID, N_IN).T + w[O1:O2])))
        return one / (one + np.exp(-(h @ w[O2:O3] + w[O3])))


def bf16_round(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def forward_bf16_f64(w, X):
    """fp64 forward pass of the bf16-rounded W1 and features (b1, W2, b2 stay fp32): what the bf16 speed mode is held against."""
    w = np.asarray(w, np.float32)
    W1 = bf16_round(w[:O1].reshape(N_HID, N_IN)).astype(np.float64)
    b1, W2, b2 = w[O1:O2].astype(np.float64), w[O2:O3].astype(np.float64), float(w[O3])
    with np.errstate(over="ignore"):
        h = 1.0 / (1.0 + np.exp(-(bf16_round(X).astype(np.float64) @ W1.T + b1)))
        return 1.0 / (1.0 + np.exp(-(h @ W2 + b2)))


# ---- row sets -----------------------------------------------------------------------------------------------------------------------

def g5_rows():
    g = np.load(os.path.join(GOLDEN, "g5_values.npz"))
    return g["states"].astype(np.int32), g["turn"].astype(np.int32)


def fixture_pairs(name):
    """Fixture G7 ("g7_candidate_values") or G8 ("g8_bar_candidate_values"): -> (roots [R,28], turn [R], dice [R,2], rows [N,28],
    root index [N], off [R+1])"""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    roots, off = g["roots"].astype(np.int32), g["off"].astype(np.int64)
    ridx = np.repeat(np.arange(len(roots)), np.diff(off)).astype(np.int32)
    return roots[:, :28], roots[:, 28], roots[:, 29:31], g["states"].astype(np.int32), ridx, off


def _backgrounds(n, seed):
    """n boards for the sweeps to overwrite one entry of: arbitrary placements (sums are not 15: the encoder and
    planes_from_state28 check ranges only)."""
    rng = np.random.RandomState(seed)
    st = np.zeros((n, 28), np.int32)
    for i in range(n):
        pts = rng.choice(24, 10, replace=False)
        st[i, pts] = rng.randint(1, 7, 10) * rng.choice([-1, 1], 10)
        st[i, 24:28] = rng.randint(0, 5, 4)
    return st


def sweep_rows(seed=SEED):
    """Every value of every feature: for each of the 24 points, counts -15..15 (each side 0..15); bar and borne-off counts 0..15 for
    each side; two backgrounds; both turn bits.  -> (states [N,28], turn [N])"""
    out = []
    for b, bgd in enumerate(_backgrounds(2, seed)):
        for i in range(24):
            for c in range(-15, 16):
                s = bgd.copy(); s[i] = c
                out.append(s)
        for k in range(24, 28):
            for c in range(16):
                s = bgd.copy(); s[k] = c
                out.append(s)
    st = np.array(out, np.int32)
    return np.concatenate([st, st]), np.repeat([0, 1], len(st)).astype(np.int32)


_CROSS = (1, 2, 3, 4, 15)


def sweep_pairs(seed=SEED):
    """(root, row) pairs that differ in ONE entry of the state: per point every (c0 -> c1) with both counts on the same side (0..15 each,
    both sides) and a few changes of side; bar and borne-off counters every (c0 -> c1) in 0..15; each pair under both turn bits (the
    list builder walks the mover's side first).  One entry changes at most 8 features, so every pair is inside the incremental
    evaluator's 16-entry list.  -> (roots [R,28], root turn [R], rows [N,28], root index [N])"""
    bgd = _backgrounds(28, seed + 1)
    roots, rows, ridx = [], [], []

    def add(k, c0, targets):
        r = bgd[k].copy(); r[k] = c0
        roots.append(r)
        for c1 in targets:
            s = r.copy(); s[k] = c1
            rows.append(s); ridx.append(len(roots) - 1)

    for i in range(24):
        for c0 in range(-15, 16):
            same = [c for c in range(-15, 16) if c * c0 >= 0]
            cross = [-np.sign(c0) * c for c in _CROSS] if c0 and abs(c0) in _CROSS else []
            add(i, c0, same + cross)
    for k in range(24, 28):
        for c0 in range(16):
            add(k, c0, range(16))
    roots, rows, ridx = np.array(roots, np.int32), np.array(rows, np.int32), np.array(ridx, np.int32)
    R = len(roots)
    return (np.concatenate([roots, roots]), np.repeat([0, 1], R).astype(np.int32), np.concatenate([rows, rows]),
            np.concatenate([ridx, ridx + R]).astype(np.int32))


def encode(st, tu):
    """The oracle's encoder over rows with a turn bit each -> float32 [N, 198]"""
    from oracle import oracle as O
    st, tu = np.asarray(st, np.int32).reshape(-1, 28), np.asarray(tu)
    X = np.empty((len(st), N_IN), np.float32)
    for tb in (0, 1):
        m = tu == tb
        if m.any():
            X[m] = O.encode(st[m], tb)
    return X


_rows = {}


def value_rows():
    """What the dense evaluators are handed: fixture G5 + the sweep + 300 arbitrary boards under both turn bits."""
    if "dense" not in _rows:
        from helpers import random_boards
        g5s, g5t = g5_rows()
        sws, swt = sweep_rows()
        rb = random_boards(300, SEED % 1000)
        _rows["dense"] = (np.concatenate([g5s, sws, rb, rb]), np.concatenate([g5t, swt, np.repeat([0, 1], len(rb))]).astype(np.int32))
    return _rows["dense"]


def pair_sets():
    """What the incremental evaluator is handed: name -> (roots, root turn, rows, root index) for fixtures G7 and G8 and the sweep."""
    if "pairs" not in _rows:
        out = {}
        for key, name in (("g7", "g7_candidate_values"), ("g8", "g8_bar_candidate_values")):
            r, t, _, s, ri, _ = fixture_pairs(name)
            out[key] = (r, t, s, ri)
        out["sweep"] = sweep_pairs()
        _rows["pairs"] = out
    return _rows["pairs"]


@contextlib.contextmanager
def memoized(module, name):
    """module.name(weights, s28, side) -- search_ref.reply_values, rollout_vr_ref.preroll: pure functions of a table, a position and the
    side to roll -- answered from a cache while the block runs (rollout trials and the K = 0, 1, 3, 8 searches of one lane meet the same
    positions again and again).  The reference itself is untouched."""
    fn, cache = getattr(module, name), {}

    def cached(weights, s28, side):
        key = (weights.ctypes.data, np.asarray(s28, np.int32).tobytes(), int(side))
        if key not in cache:
            cache[key] = fn(weights, s28, side)
        return cache[key]
    setattr(module, name, cached)
    try:
        yield
    finally:
        setattr(module, name, fn)


@contextlib.contextmanager
def recorded_net_rows(search_ref):
    """Every (encoded) row the fp64 references hand to search_ref.net while the block runs -> list of float32 [n, 198] arrays: the rows a
    pre-roll evaluation or a rollout evaluates, for the numpy fp32 forward's own error "on those rows"."""
    fn, rows = search_ref.net, []

    def net(weights, states, turn):
        st = np.asarray(states, dtype=np.int32).reshape(-1, 28)
        if len(st):
            rows.append(encode(st, np.full(len(st), turn)))
        return fn(weights, states, turn)
    search_ref.net = net
    try:
        yield rows
    finally:
        search_ref.net = fn


def _bearoffs():
    """Late bear-offs: every trial ends within a few turns."""
    st = np.zeros((3, 28), np.int32)
    st[0, [18, 20, 23]] = [1, 2, 1]; st[0, [0, 2, 4]] = [-1, -1, -2]; st[0, 26], st[0, 27] = 11, 11
    st[1, [19, 22]] = [2, 1]; st[1, [1, 5]] = [-2, -1]; st[1, 26], st[1, 27] = 12, 12
    st[2, 23] = 1; st[2, [0, 1]] = [-1, -1]; st[2, 26], st[2, 27] = 14, 13
    return st, np.array([0, 1, 1], np.int32)


def _singles():
    """One checker a side, the other fourteen borne off (ranges are what the library checks, not reachability): three with contact
    ahead (a blot may be hit), three already past each other (every turn is forced)."""
    st = np.zeros((6, 28), np.int32)
    for k, (a, b) in enumerate(((2, 20), (0, 12), (6, 23), (14, 9), (12, 11), (16, 5))):
        st[k, a], st[k, b] = 1, -1
    st[:, 26] = st[:, 27] = 14
    return st, np.array([0, 1, 1, 0, 1, 0], np.int32)


def _stuck():
    """Both sides on the bar.  [0]: against six made points each -- nobody ever moves, every turn is a pass and a trial can only be
    cut; [1], [2]: five made points each -- a lone 6 (PLAYER1) / 6 (PLAYER2) enters, so trials stay put for a while and then race."""
    a = np.zeros(28, np.int32)
    a[0:6] = -2; a[6] = -2; a[25] = 1                    # PLAYER2: 12 on PLAYER1's entry points, 2 outside, 1 on the bar
    a[18:24] = 2; a[17] = 2; a[24] = 1                   # PLAYER1: the mirror image
    b = a.copy(); b[5] = 0; b[6] = -4; b[18] = 0; b[17] = 4
    return np.array([a, b, b], np.int32), np.array([0, 0, 1], np.int32)


def _cat(*parts):
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]).astype(np.int32)


def _pick(part, idx):
    return part[0][list(idx)], part[1][list(idx)]


def tie_rollout_positions():
    """Eight positions for the all-values-equal rollouts of 16 turns: bear-offs that end, positions that can only be cut, and in
    between.  Few checkers (or no moves) keep the reference's 21-roll pre-roll evaluation of every turn cheap."""
    return _cat(_bearoffs(), _pick(_stuck(), (0,)), _pick(_singles(), (1, 3, 4, 5)))


def family_rollout_positions():
    """Eight positions for the 3-turn rollouts under every parity family.  Under a net whose values differ by less than the near-tie
    margin between most candidates (xavier: every value is 0.5 +- 1e-4) any real decision is a near tie that the comparison with the
    reference leaves out, so most of these have forced turns: what the test is after is the truncation value, not the choice."""
    return _cat(_singles(), _pick(_stuck(), (0, 1)))


def preroll_positions():
    """Closed boards (rolls without a legal move), stuck positions, single checkers and bear-offs."""
    return _cat(closed_board_positions(), _stuck(), _pick(_singles(), (0, 1, 2)), _pick(_bearoffs(), (0, 1)))


def closed_board_positions():
    """Positions whose mover sits on the bar against a home board with five or six points made: most (or all) rolls have no legal move,
    so the pre-roll evaluator scores them with its own hidden-to-value loop.  -> (states [4,28], turn [4])"""
    a = np.zeros(28, np.int32)                           # PLAYER1 on the bar enters on points 1..6: all six held by PLAYER2
    a[0:6] = -2; a[7] = -3; a[18:24] = 2; a[17] = 2; a[24] = 1
    b = a.copy(); b[5] = 0; b[7] = -5                    # ... five held: only a 6 enters
    c = np.zeros(28, np.int32)                           # PLAYER2 on the bar enters on points 24..19
    c[18:24] = 2; c[16] = 3; c[0:6] = -2; c[6] = -2; c[25] = 1
    d = c.copy(); d[18] = 0; d[16] = 5
    return np.array([a, b, c, d], np.int32), np.array([0, 0, 1, 1], np.int32)
