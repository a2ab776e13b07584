"""Logs, a step-by-step float64 reference and a per-parameter error bound for the tests that look at EVERY update of the TD(λ)
learner (tests/test_learner_steps_cpu.py on the CPU, tests/test_gpu_learner_steps.py on the device).  A helper module in the style of
tests/nets.py, not a conftest: everything is a function of a seed and of fixture G3, nothing is read from outside tests/golden.

A log is (states int32 [T, G, 28], turn int32 [T, G], lengths int64 [G], p1_won bool [G]): turn t of game g is states[t, g] with
turn[t, g] to move; rows past a game's length repeat its last turn and are never part of a replay.

One training step in closed form (backgammon_env/learner.py):
    h = σ(W1 x + b1), v = σ(W2·h + b2), g = v(1-v);  ∇b2 = g, ∇W2 = g h, ∇b1 = g W2 ⊙ h ⊙ (1-h), ∇W1 = ∇b1 ⊗ x
    e ← λ e + ∇ (e ← ∇ on a game's first step);  δ = V(s_{t+1}) - V(s_t), terminal: z - V(s_t);  update = Σ_g fp(α δ_g) e_g"""
import collections
import os

import numpy as np

import nets as N

N_IN, N_HID, O1, O2, O3, N_PARAMS = N.N_IN, N.N_HID, N.O1, N.O2, N.O3, N.N_PARAMS
SEED = N.SEED
ALPHA, BATCH_SCALE, LAM, SLOTS = 0.1, 0.25, 0.7, 7

# The bound's constants.  V: the project's value parity bound (what tests/test_nets_cpu.py rests on); H: the absolute error allowed on
# a hidden unit; R: relative rounding.  (A change to any of them is recorded here with the measured ratio that made it necessary: none.)
V, H, R = 1e-5, 1e-5, 4e-6

# (family, mode, λ) whose free-running float32 replay leaves a quarter of the bound, with the worst ratio measured for plain numpy float32
# (tests/test_learner_steps_cpu.py): the rounding the float32 weights gather from step to step, which the bound -- first order in the
# errors of ONE step from the SAME weights -- has no term for.  xavier: fc2.weight[86] passes through zero in mid-replay (-0.0155 ...
# +1.2e-5), where the 8e-9 its float32 copy has gathered is 7e-4 of it, and every gradient of that hidden unit is off by as much.  The
# streamed replays take 695 steps instead of 48: fifteen times the additions to every weight; at λ = 1 nothing of it decays.  These
# cases are held against the reference evaluated AT the weights the replay under test went through (replay(weights=...)).
NARROWED = {("xavier", "lockstep", 0.7): 1.32, ("xavier", "streamed", 0.7): 40.5, ("loguniform", "streamed", 0.7): 2.2,
            ("ckpt", "streamed", 0.7): 0.91, ("normal", "streamed", 0.7): 0.27, ("ckpt", "streamed", 1.0): 2.34,
            ("normal", "streamed", 0.25): 3.73, ("normal", "lockstep", 1.0): 4.37, ("normal", "streamed", 1.0): 5.89,
            ("zero_w1", "streamed", 0.7): 1.69}      # (an edge net: W1 starts at exactly 0 and its first additions are all rounding)

# the deliberately wrong references (negative controls) and the replay mode each exists in
MUTATIONS = {"plane3": "lockstep", "off16": "lockstep", "bar_swap": "lockstep", "lam": "lockstep", "z": "lockstep",
             "no_restart": "streamed", "stale_new": "streamed", "ring_wrap": "ring"}

_PATTERN = (0, 4, 0, 8, -8, 0, 15, -15, 3, 0, -1, 1, 0, 7, -12, 0)
T_ZIGZAG = 48
# per log: the game of length 1, the game of length 0, a game of full length (every 9th game, from game 0, is cut to a third)
_ONE, _ZERO, _FULL = 5, 7, 1


# ---- the encoder (model.py:111-144), with the wrong decodes the negative controls need ---------------------------------------------

def encode(states, turn, mutate=None):
    """[..., 28] states + [...] turn bits -> float32 [..., 198]; mutate=None is the oracle's encoder to the bit
    (tests/test_learner_steps_cpu.py)."""
    st = np.asarray(states, np.int64)
    tu = np.asarray(turn)
    lead = st.shape[:-1]
    F = np.zeros(lead + (24, 8), np.float64)
    for side, cnt in ((0, np.maximum(st[..., :24], 0)), (1, np.maximum(-st[..., :24], 0))):
        if mutate == "plane3":
            cnt = np.where(cnt >= 8, cnt & 7, cnt)
        for k in range(3):
            F[..., 4 * side + k] = cnt > k
        F[..., 4 * side + 3] = np.where(cnt >= 4, (cnt - 3) / 2.0, 0.0)
    bar = st[..., [25, 24]] if mutate == "bar_swap" else st[..., 24:26]
    tail = np.stack([tu == 0, tu != 0, bar[..., 0] / 2.0, bar[..., 1] / 2.0, st[..., 26] / (16.0 if mutate == "off16" else 15.0),
                     st[..., 27] / (16.0 if mutate == "off16" else 15.0)], axis=-1)
    return np.concatenate([F.reshape(lead + (192,)), tail], axis=-1).astype(np.float32)


# ---- logs -----------------------------------------------------------------------------------------------------------------------------

def _ragged(natural, T):
    ln = np.asarray(natural, np.int64).copy()
    ln[::9] //= 3
    ln[_ONE], ln[_ZERO] = 1, 0
    assert ln[_FULL] == T and ln.max() == T
    return ln


def _pad(games, T):
    """list of ([len, 28], [len]) -> [T, G, 28], [T, G], natural lengths: rows past the end repeat the last turn"""
    st = np.zeros((T, len(games), 28), np.int32)
    tu = np.zeros((T, len(games)), np.int32)
    for g, (s, t) in enumerate(games):
        n = len(s)
        st[:n, g], tu[:n, g] = s, t
        st[n:, g], tu[n:, g] = s[-1], t[-1]
    return st, tu, np.array([len(s) for s, _ in games], np.int64)


def sweep_log():
    """Every value of every feature, as s_t and as s_{t+1}: per background (2), starting turn bit and point one game whose turn t has
    t - 15 checkers on the point (t = 0..30: columns of the second side become active after step 0), and one game per counter with
    0..15; the turn bit alternates.  112 games, T = 31."""
    games = []
    for bgd in N._backgrounds(2, SEED):
        for tb in (0, 1):
            for i in range(24):
                s = np.repeat(bgd[None], 31, 0)
                s[:, i] = np.arange(31) - 15
                games.append((s, (tb + np.arange(31)) % 2))
            for k in range(24, 28):
                s = np.repeat(bgd[None], 16, 0)
                s[:, k] = np.arange(16)
                games.append((s, (tb + np.arange(16)) % 2))
    st, tu, natural = _pad(games, 31)
    return st, tu, _ragged(natural, 31), np.arange(len(games)) % 3 != 1


def zigzag_log():
    """Counts that leave and re-enter values -- the not-written-then-written-again path of the lazily scaled traces: game i runs point
    i through a fixed pattern (period 16), point i + 12 through its negative (so every point has two games: the ragged lengths cost no
    column its coverage) and counter 24 + i % 4 through its magnitude, on a third background; T = 48, so that λ = 2^-2 folds its
    scale back twice."""
    bgd = N._backgrounds(3, SEED)[2]
    pat = np.array(_PATTERN * (T_ZIGZAG // len(_PATTERN)), np.int32)
    games = []
    for i in range(24):
        s = np.repeat(bgd[None], T_ZIGZAG, 0)
        s[:, i], s[:, (i + 12) % 24], s[:, 24 + i % 4] = pat, -pat, np.abs(pat)
        games.append((s, (i + np.arange(T_ZIGZAG)) % 2))
    st, tu, natural = _pad(games, T_ZIGZAG)
    return st, tu, _ragged(natural, T_ZIGZAG), np.arange(24) % 2 == 0


def g3_log():
    """The first 24 games of fixture G3 (random play: real bar entries and bear-offs), cut to their first 48 turns."""
    rows = np.load(os.path.join(N.GOLDEN, "g3_random_trajectories.npz"))["rows"]
    games, won = [], []
    for lane in range(24):
        rr = rows[rows[:, 0] == lane]
        assert (rr[:, 1] == np.arange(len(rr))).all() and rr[-1, 35] == 1
        games.append((rr[:T_ZIGZAG, 2:30].astype(np.int32), rr[:T_ZIGZAG, 30].astype(np.int32)))
        won.append(rr[-1, 36] == 0)
    st, tu, natural = _pad(games, T_ZIGZAG)
    return st, tu, _ragged(natural, T_ZIGZAG), np.array(won)


_LOGS = {}


def log(name="all"):
    """"sweep", "zigzag", "g3", or "all": the three side by side along G, padded to T = 48 -- 160 games of which 157 have turns (not a
    multiple of 2, 4, 8 or 16).  Read-only: shared between the tests."""
    if name not in _LOGS:
        if name == "all":
            parts = [log(k) for k in ("sweep", "zigzag", "g3")]
            T = max(p[0].shape[0] for p in parts)
            st = np.concatenate([np.concatenate([p[0], np.repeat(p[0][-1:], T - len(p[0]), 0)]) for p in parts], axis=1)
            tu = np.concatenate([np.concatenate([p[1], np.repeat(p[1][-1:], T - len(p[1]), 0)]) for p in parts], axis=1)
            out = (st, tu, np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts]))
            assert (out[2] > 0).sum() % 2 == 1
        else:
            out = {"sweep": sweep_log, "zigzag": zigzag_log, "g3": g3_log}[name]()
        for a in out:
            a.setflags(write=False)
        _LOGS[name] = out
    return _LOGS[name]


def register_log(name, states, turn, lengths, p1_won):
    """another log for the replays below (fixture G6's single game in tests/test_learner_steps_cpu.py)"""
    _LOGS[name] = (np.asarray(states, np.int32), np.asarray(turn, np.int32), np.asarray(lengths, np.int64), np.asarray(p1_won, bool))


def ring_layout(name="all"):
    """The log laid into a ring of R = T + 5 rows with a game table: game i sits in lane G - 1 - i, its turn k in ring row
    (game_start[i] + k) % R; the starts make more than a third of the games wrap.  Rows no game owns hold the lane's first turn under the other turn bit.
    -> (ring states [R, G, 28], ring turn [R, G], game_lane [G], game_start [G])"""
    st, tu, ln, _ = log(name)
    T, G = tu.shape
    Rr = T + 5
    lane = (G - 1 - np.arange(G)).astype(np.int32)
    start = ((np.arange(G) * 11 + 3) % Rr).astype(np.int32)
    rs = np.repeat(st[:1, ::-1], Rr, 0).copy()
    rt = np.repeat(1 - tu[:1, ::-1], Rr, 0).copy()
    for i in range(G):
        r = (start[i] + np.arange(ln[i])) % Rr
        rs[r, lane[i]], rt[r, lane[i]] = st[:ln[i], i], tu[:ln[i], i]
    return rs, rt, lane, start


# ---- one step -------------------------------------------------------------------------------------------------------------------------

Traces = collections.namedtuple("Traces", "e err mag")      # the trace, the error trace ẽ, the magnitude trace ē: [slots, 25601] each


def new_traces(slots, dtype=np.float64, bound=True):
    z = lambda: np.zeros((slots, N_PARAMS), dtype)
    return Traces(z(), z() if bound else None, z() if bound else None)


def _outer_add(E, a, x):
    """E[:, :O1] (as [S, 128, 198]) += a ⊗ x"""
    E[:, :O1] += (a[:, :, None] * x[:, None, :]).reshape(len(E), O1)


def step_reference(theta, tr, X_t, X_t1, running, terminal, z, first, alpha, lam, mutate=None):
    """One training step in plain numpy, in theta's dtype (float64: the reference; float32: the plain fp32 restatement the bound is
    measured on).  theta [25601]; tr: Traces of the slots, UPDATED IN PLACE; X_t, X_t1 [S, 198] features of s_t and s_{t+1}; running,
    terminal, first: bool [S] (first: the slot's game starts here, its trace restarts); z [S] the terminal targets; alpha includes the
    batch scale.  -> (update [25601], tr, δ [S], bound [25601] or None).

    The bound, first order in the errors a float32 evaluator is allowed -- V on a value, H on a hidden unit, R relative rounding --
    per running game, with ḡ = g + V, q̄ = h(1-h) + H, h̄ = h + H:
        inflated gradient magnitudes m_b2 = ḡ, m_W2 = ḡ h̄, m_b1 = ḡ |W2| q̄, m_W1 = m_b1 ⊗ |x|;  d = m - (1 - R) |∇|
        ẽ ← λ ẽ + d, ē ← λ ē + |∇|  (both restart with `first`)
        bound = Σ_g [ |α δ_g| ẽ_g + 2 α V (ē_g + ẽ_g) + R |α δ_g| ē_g ]"""
    dt = theta.dtype
    one = dt.type(1)
    if mutate == "lam":
        lam = lam * (1 + 1e-3)
    W1, b1, W2, b2 = theta[:O1].reshape(N_HID, N_IN), theta[O1:O2], theta[O2:O3], theta[O3]
    run = running.astype(dt)

    def fwd(x):
        with np.errstate(over="ignore"):
            h = one / (one + np.exp(-(x @ W1.T + b1)))
            return one / (one + np.exp(-(h @ W2 + b2))), h

    x = X_t.astype(dt) * run[:, None]
    v, h = fwd(x)
    vn, _ = fwd(X_t1.astype(dt))
    delta = np.where(terminal, z.astype(dt) - v, vn - v) * run
    g = v * (one - v) * run
    q = h * (one - h)
    db1 = g[:, None] * W2[None, :] * q
    e = tr.e
    e[first] = 0
    e *= dt.type(lam)
    _outer_add(e, db1, x)
    e[:, O1:O2] += db1
    e[:, O2:O3] += g[:, None] * h
    e[:, O3] += g
    coef = (alpha * delta.astype(np.float64)).astype(dt)          # α·δ is formed in float64 (python floats in the reference learner)
    upd = coef @ e
    bound = None
    if tr.err is not None:
        gb = (g + V) * run
        mb1 = gb[:, None] * np.abs(W2)[None, :] * (q + H)
        adb1 = np.abs(db1)
        for E, fb1, fW2, fb2 in ((tr.err, mb1 - (1 - R) * adb1, gb[:, None] * (h + H) - (1 - R) * g[:, None] * h, gb - (1 - R) * g),
                                 (tr.mag, adb1, g[:, None] * h, g)):
            E[first] = 0
            E *= lam
            _outer_add(E, fb1, np.abs(x))
            E[:, O1:O2] += fb1
            E[:, O2:O3] += fW2
            E[:, O3] += fb2
        ad = np.abs(alpha * delta)
        bound = (ad + 2 * alpha * V * run) @ tr.err + (2 * alpha * V * run + R * ad) @ tr.mag
    return upd, tr, delta, bound


# ---- whole replays --------------------------------------------------------------------------------------------------------------------

class Run:
    """updates [n_steps, 25601] (the replay's dtype), bounds [n_steps, 25601] float64 or None, theta: the weights after the last step,
    sq = Σ δ², count = (game, step) updates, n_active: running slots per step, resolved: see `against`, weights: [n_steps, 25601] the
    weights every step started from (keep_weights=True only).  The bounds are kept as float32, rounded up."""
    def __init__(self, keep_weights=False):
        self.updates, self.bounds, self.n_active = [], [], []
        self.sq, self.count, self.resolved, self.theta = 0.0, 0, None, None
        self.weights = [] if keep_weights else None

    def close(self, theta):
        self.theta = theta
        self.updates = np.array(self.updates)
        self.bounds = np.nextafter(np.array(self.bounds, np.float32), np.float32(np.inf)) if self.bounds and self.bounds[0] is not None else None
        if self.weights is not None:
            self.weights = np.array(self.weights)
        return self


def _record(run, upd, bound, delta, n_run, against, factor):
    """-> True when the replay is a negative control that has just been told from the true one: the first (step, parameter) at which it
    differs from `against` by at least `factor` x the bound"""
    s = len(run.updates)
    run.updates.append(upd)
    run.bounds.append(bound)
    run.n_active.append(n_run)
    run.sq += float((delta.astype(np.float64) ** 2).sum())
    run.count += n_run
    if against is not None and s < len(against.updates):
        d = np.abs(upd - against.updates[s])
        hit = (d >= factor * against.bounds[s]) & (d > 0)
        if hit.any():
            with np.errstate(divide="ignore"):
                ratio = np.where(hit, d / against.bounds[s], 0)
            p = int(np.argmax(ratio))
            run.resolved = (s, p, float(ratio[p]), float(d[p]))     # (ratio inf: the reference update is exactly 0 there, its bound too)
            return True
    return False


def _advance(theta, upd, weights, s):
    """the weights of the next step: the replay's own update is added, or (weights given) the next row of that trajectory is taken"""
    if weights is None:
        theta += upd
    elif s + 1 < len(weights):
        theta = weights[s + 1].astype(theta.dtype)
    return theta


def _flip(won, mutate):
    z = np.asarray(won).astype(np.float64).copy()
    if mutate == "z":
        z[_ONE] = 1 - z[_ONE]                                   # the sweep's one-turn game: its only step is terminal, at step 0
    return z


def _lockstep(theta0, logname, lam, dtype, mutate, bound, alpha, against, factor, reset_every_step, weights=None, keep_weights=False):
    st, tu, ln, won = log(logname)
    T = tu.shape[0]
    X = encode(st, tu, mutate)
    theta = np.asarray(theta0 if weights is None else weights[0], dtype).copy()
    idx = np.nonzero(ln > 0)[0]                                 # games drop out of the arrays when they end
    tr = new_traces(len(idx), dtype, bound)
    z = _flip(won, mutate)
    run = Run(keep_weights)
    for t in range(int(ln.max())):
        keep = ln[idx] > t
        if not keep.all():
            idx, tr = idx[keep], Traces(*(None if a is None else a[keep] for a in tr))
        first = np.full(len(idx), t == 0 or reset_every_step)
        if keep_weights:
            run.weights.append(theta.copy())
        upd, tr, delta, b = step_reference(theta, tr, X[t, idx], X[min(t + 1, T - 1), idx], np.ones(len(idx), bool), ln[idx] == t + 1,
                                           z[idx], first, alpha, lam, mutate)
        theta = _advance(theta, upd, weights, len(run.updates))
        if _record(run, upd, b, delta, len(idx), against, factor):
            break
    return run.close(theta)


def schedule(lengths, slots):
    """backgammon_env.learner.stream_schedule as tables: -> (game [n_steps, k] the game a slot replays at a step or -1, tl [n_steps, k]
    that game's own step, queue, qoff)"""
    from backgammon_env.learner import stream_schedule
    import torch
    queue, qoff, n_steps, k = stream_schedule(torch.as_tensor(np.array(lengths)), slots)
    queue, qoff = queue.numpy(), qoff.numpy()
    game = np.full((n_steps, k), -1, np.int64)
    tl = np.zeros((n_steps, k), np.int64)
    for i in range(k):
        s0 = 0
        for q in queue[qoff[i]:qoff[i + 1]]:
            n = int(lengths[q])
            game[s0:s0 + n, i], tl[s0:s0 + n, i] = q, np.arange(n)
            s0 += n
    return game, tl, queue.astype(np.int32), qoff.astype(np.int32)


def _streamed(theta0, logname, lam, slots, ring, dtype, mutate, bound, alpha, against, factor, reset_every_step=False, weights=None,
              keep_weights=False):
    st, tu, ln, won = log(logname)
    T = tu.shape[0]
    X = encode(st, tu, mutate)
    if ring:
        rs, rt, lane, start = ring_layout(logname)
        XR = encode(rs, rt, mutate)
    theta = np.asarray(theta0 if weights is None else weights[0], dtype).copy()
    game, tl, _, _ = schedule(ln, slots)
    k = game.shape[1]
    tr = new_traces(k, dtype, bound)
    z = _flip(won, mutate)
    stale, seen = np.zeros((k, N_HID, N_IN), dtype), np.zeros((k, N_IN), bool)
    run = Run(keep_weights)
    for s in range(len(game)):
        gm, t = game[s], tl[s]
        if keep_weights:
            run.weights.append(theta.copy())
        running = gm >= 0
        gi = np.maximum(gm, 0)
        first = running & ((t == 0) | reset_every_step)
        X_t, X_t1 = X[t, gi], X[np.minimum(t + 1, T - 1), gi]
        if mutate == "ring_wrap":                               # s_{t+1} read from the ring without wrapping at its end
            X_t1 = XR[np.minimum(start[gi] + t + 1, len(XR) - 1), lane[gi]]
        if mutate == "stale_new":                               # a column that becomes active after a game's first step starts from
            eW1 = tr.e[:, :O1].reshape(k, N_HID, N_IN)          # what the slot's previous game left there
            stale[first] = eW1[first]
            seen[first] = False
            new = (X_t != 0) & ~seen & running[:, None]
            seen |= new
            new &= ~first[:, None]
        upd, tr, delta, b = step_reference(theta, tr, X_t, X_t1, running, running & (ln[gi] == t + 1), z[gi],
                                           first if mutate != "no_restart" else first & (s == 0), alpha, lam, mutate)
        if mutate == "stale_new" and new.any():
            add = lam * stale * new[:, None, :]
            eW1 += add
            upd = upd + np.concatenate([((alpha * delta)[:, None, None] * add).sum(0).reshape(-1), np.zeros(N_PARAMS - O1, dtype)])
        theta = _advance(theta, upd, weights, len(run.updates))
        if _record(run, upd, b, delta, int(running.sum()), against, factor):
            break
    return run.close(theta)


def scale_passes(lam, n):
    """The scale c of the lazily stored traces over n steps, as bgamd_td_step keeps it (td_scale_step of csrc/bg_td_plan.h: `if (t == 0) scale = 1.0`,
    then c = λ·scale is kept while `c >= 0x1p-40 && c <= 0x1p40`, else an ordinary pass folds it back and the scale returns to 1)
    -> (the steps that are ordinary passes, the scales reached in between)"""
    c, full, reached = 1.0, [], []
    for t in range(n):
        x = lam * c
        if t > 0 and 2.0 ** -40 <= x <= 2.0 ** 40:
            c = x
            reached.append(c)
        else:
            c = 1.0
            full.append(t)
    return full, reached


_CACHE = collections.OrderedDict()
_CACHE_BYTES = 3 << 28


def replay(net, logname="all", mode="lockstep", lam=LAM, dtype=np.float64, mutate=None, against=None, factor=10.0,
           reset_every_step=False, slots=SLOTS, alpha=ALPHA, batch_scale=BATCH_SCALE, weights=None, keep_weights=False, bound=None):
    """The whole replay of `logname` under table `net` (a name of tests/nets.py) -> Run; mode: "lockstep", "streamed" (through `slots`
    slots) or "ring" (the same schedule over ring_layout's game table).  Plain replays are kept per (net, log, mode, λ, dtype, ...), the
    least recently used dropped above 768 MiB.  against: the true Run -- the (mutated) replay stops at the first step that differs from
    it by at least factor x its bound somewhere, .resolved = (step, parameter, ratio, |difference|).  weights [n_steps, 25601]: step s is
    taken from weights[s] instead of from what the replay's own updates add up to -- the reference AT the weights another replay (a
    float32 one, the device's) went through: its traces are the reference's own, its updates owe nothing to that replay's.
    bound=False: no bounds (a float64 replay has them by default)."""
    key = (net, logname, mode, float(lam), np.dtype(dtype).name, reset_every_step, slots, alpha, batch_scale, bound)
    plain = mutate is None and weights is None and not keep_weights
    if plain and key in _CACHE:
        _CACHE.move_to_end(key)
        return _CACHE[key]
    theta0 = N.reference_table(net)
    if bound is None:
        bound = mutate is None and np.dtype(dtype) == np.float64
    if mode == "lockstep":
        run = _lockstep(theta0, logname, lam, dtype, mutate, bound, alpha * batch_scale, against, factor, reset_every_step, weights,
                        keep_weights)
    else:
        run = _streamed(theta0, logname, lam, slots, mode == "ring", dtype, mutate, bound, alpha * batch_scale, against, factor,
                        reset_every_step, weights, keep_weights)
    if plain:
        _CACHE[key] = run
        size = lambda r: r.updates.nbytes + (0 if r.bounds is None else r.bounds.nbytes)
        while len(_CACHE) > 1 and sum(size(r) for r in _CACHE.values()) > _CACHE_BYTES:
            _CACHE.popitem(last=False)
    return run


def lockstep(net, logname="all", lam=LAM, **kw):
    return replay(net, logname, "lockstep", lam, **kw)


def streamed(net, logname="all", lam=LAM, slots=SLOTS, ring=False, **kw):
    return replay(net, logname, "ring" if ring else "streamed", lam, slots=slots, **kw)


def where(p):
    """parameter index -> "W1[n=.., j=..]" / "b1[n]" / "W2[n]" / "b2": the block, the hidden unit and the feature column"""
    p = int(p)
    if p < O1:
        return "W1[hidden unit %d, feature column %d]" % (p // N_IN, p % N_IN)
    if p < O2:
        return "b1[hidden unit %d]" % (p - O1)
    return "W2[hidden unit %d]" % (p - O2) if p < O3 else "b2"
