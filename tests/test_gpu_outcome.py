"""Gammons and backgammons on the MI355X (bgamd_outcomes, bgamd_env_outcomes, bgamd_env_rollout_outcomes_read; VecGame.outcomes,
VecGame.rollout(outcomes=True), arena.head_to_head, analysis.rollout_moves): the operator and the env call against the numpy rule
(tests/outcome_ref.py), the rollout's per-trial points trial for trial against the greedy step's own final boards and against the fp64
CPU reference, the counts and the equity against the per-trial outputs, invariance to lanes / calls / offsets / luck adjustment, errors
and side effects, and the points the arena and the move analysis report.  That the forced positions end the way these tests assume is
checked on the CPU (tests/test_outcome_cpu.py)."""
import os

import numpy as np
import pytest

import outcome_ref as OR
import rollout_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SEED = 4242
CLASSES = (1, 2, 3, -1, -2, -3)          # the order of counts [P, 6]
PLAIN = ("mean", "stderr", "turns", "truncated", "trial_value", "trial_turns")
OUT = ("counts", "equity", "equity_stderr", "trial_points")


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


@pytest.fixture(scope="module")
def W():
    return np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)


@pytest.fixture(scope="module")
def env(bg, W):
    e = bg.VecGame(64, seed=7)
    e.load_weights(W)
    yield e
    e.close()


def _greedy_positions(bg, W, n, seed, skip=0):
    """n positions reached by seeded greedy play from the start position (lane k stopped after skip + k + 1 turns, so plies differ)."""
    e = bg.VecGame(max(n, 64), seed=seed)
    e.load_weights(W)
    if skip:
        e.run_greedy(skip)
    st, tu = [], []
    for k in range(n):
        e.step_greedy()
        st.append(e.states()[k].cpu().numpy()); tu.append(int(e.turns()[k]))
    e.close()
    return np.array(st, np.int32), np.array(tu, np.int32)


@pytest.fixture(scope="module")
def positions(bg, W):
    """P = 18: the ten forced positions, six late-game positions of greedy play, two boards that are already over."""
    fst, ftu, _, _ = OR.forced_positions()
    gst, gtu = _greedy_positions(bg, W, 6, 13, skip=40)
    assert (OR.points_many(gst) == 0).all()
    ost, _ = OR.over_boards()
    return (np.concatenate([fst, gst, ost]).astype(np.int32), np.concatenate([ftu, gtu, [0, 1]]).astype(np.int32))


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _assert_same(a, b, keys=None):
    for k in (keys or a):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_operator_against_the_rule(bg):
    fam, want = OR.probe_family()
    g10 = np.load(os.path.join(ROOT, "tests", "golden", "g10_arbitrary_boards.npz"))["boards"].astype(np.int32)
    assert len(g10) >= 1000
    ost, owant = OR.over_boards()
    st = np.concatenate([fam, ost, OR.START[None], g10]).astype(np.int32)
    ref = OR.points_many(st)
    np.testing.assert_array_equal(ref[:102], np.concatenate([want, owant]))
    for n in (1, 63, 257, len(st)):                          # (257: one thread in the second workgroup)
        got = bg.outcomes(st[:n])
        assert got.dtype == torch.int32 and tuple(got.shape) == (n,)
        np.testing.assert_array_equal(got.cpu().numpy(), ref[:n], err_msg=str(n))
    assert int(bg.outcomes(OR.START)) == 0 and tuple(bg.outcomes(st[:6].reshape(2, 3, 28)).shape) == (2, 3)
    bad = st[:300].copy()
    bad[7, 3] = 16
    bad[299, 24] = 16
    got = bg.outcomes(bad).cpu().numpy()
    assert got[7] == got[299] == -2 ** 31 == bg._capi.OUTCOME_BAD
    keep = np.ones(300, bool)
    keep[[7, 299]] = False
    np.testing.assert_array_equal(got[keep], ref[:300][keep])
    with pytest.raises(bg.BgamdError):
        bg.outcomes(st[:0])


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_env_outcomes(bg, W):
    fst, ftu, fwant, _ = OR.forced_positions()
    ost, _ = OR.over_boards()
    mix = np.concatenate([fst, ost, OR.START[None]]).astype(np.int32)
    mtu = np.concatenate([ftu, [0, 1], [0]]).astype(np.int32)
    n = 300                                                  # (a second workgroup with a tail)
    idx = np.arange(n) % len(mix)
    st, tu = mix[idx], mtu[idx]
    before = OR.points_many(st)
    assert ((before != 0) == ((idx == 10) | (idx == 11))).all()

    def fresh():
        e = bg.VecGame(n, seed=21)
        e.load_weights(W)
        e.set_states(st, tu)
        return e
    e = fresh()
    got = e.outcomes()
    assert got.dtype == torch.int32 and tuple(got.shape) == (n,)
    np.testing.assert_array_equal(got.cpu().numpy(), before)
    e.step_greedy(auto_reset=False)
    after = e.outcomes().cpu().numpy()
    np.testing.assert_array_equal(after, OR.points_many(e.states().cpu().numpy()))
    frozen = (e.flags().cpu().numpy() & 4) != 0
    for p in range(9):                                       # positions 1a .. 7 end with any roll
        assert frozen[idx == p].all() and (after[idx == p] == fwant[p]).all(), p
    assert set(after[idx == 9]) == {0, -3}                   # position 8: the rolls holding a 1
    assert (after[idx == 12] == 0).all() and not frozen[idx == 12].any()
    assert (after[~frozen] == 0).all()
    e.close()
    e = fresh()                                              # the same step with auto-reset: the finished lanes are on the start position
    e.step_greedy(auto_reset=True)
    reset = e.outcomes().cpu().numpy()
    assert (reset[frozen] == 0).all() and (reset[idx < 10] == 0).all()
    np.testing.assert_array_equal(reset, OR.points_many(e.states().cpu().numpy()))
    e.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rotate,M", [(False, 0), (True, 6)])
def test_trial_for_trial_against_the_greedy_step(bg, W, env, positions, rotate, M):
    """Trial jl = p T + i is game id jl: lane jl of a fresh env with lane_offset 0 (position p's lanes have lane_offset p T) plays it
    with the same dice.  Both sides run the device's own play, so no trial is left out."""
    st, tu = positions
    P, T = len(st), 72
    assert P == 18
    r = _np(env.rollout(st, tu, T, max_plies=M, rotate=rotate, seed=SEED, per_trial=True, outcomes=True))
    tp = r["trial_points"]
    assert tp.dtype == np.int8 and tp.shape == (P, T)
    e = bg.VecGame(P * T, seed=SEED)
    e.load_weights(W)
    e.set_states(np.repeat(st, T, axis=0), np.repeat(tu, T))
    k = 0
    if rotate:
        i = np.tile(np.arange(T), P)
        e.set_dice(np.stack([1 + (i % 36) // 6, 1 + (i % 36) % 6], 1).astype(np.int32))
        e.step_greedy(roll=False, auto_reset=False)
        k = 1
    while k < (M or 100000):
        e.step_greedy(auto_reset=False)
        k += 1
        if k % 16 == 0 and bool(((e.flags() & 4) != 0).all()):
            break
    frozen = ((e.flags().cpu().numpy() & 4) != 0).reshape(P, T)
    want = np.where(frozen, OR.points_many(e.states().cpu().numpy()).reshape(P, T), 0)
    e.close()
    over = OR.points_many(st)                                # a position that is already over is scored at 0 turns, from its own board
    want[over != 0] = over[over != 0][:, None]
    if not M:
        assert frozen.all()
    np.testing.assert_array_equal(tp, want)
    assert (tp == 0).sum() == r["truncated"].sum() and ((tp > 0) == (r["trial_value"] == 1))[tp != 0].all()
    for c in CLASSES:
        assert (tp == c).any(), c
    assert (tp == 0).any() == bool(M)                        # (without a turn limit no trial is truncated)
    np.testing.assert_array_equal(r["counts"], np.stack([(tp == c).sum(1) for c in CLASSES], 1))


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_statistics_match_the_per_trial_outputs(env, positions):
    st, tu = positions
    for T, M in ((100, 0), (72, 4), (1, 0)):
        r = _np(env.rollout(st, tu, T, max_plies=M, rotate=False, seed=SEED + T, per_trial=True, outcomes=True))
        tp, tv = r["trial_points"].astype(np.int64), r["trial_value"]
        assert r["counts"].dtype == np.int64 and r["counts"].shape == (len(st), 6)
        np.testing.assert_array_equal(r["counts"], np.stack([(tp == c).sum(1) for c in CLASSES], 1))
        np.testing.assert_array_equal(r["counts"].sum(1), T - r["truncated"])
        fin = tp != 0
        assert ((tp > 0) == (tv == 1))[fin].all() and ((tp < 0) == (tv == 0))[fin].all()
        assert (np.abs(tp) <= 3).all()
        e = np.where(fin, tp.astype(np.float64), 2.0 * tv.astype(np.float64) - 1.0)
        mean = e.sum(1) / T
        se = np.sqrt(((e - mean[:, None]) ** 2).sum(1) / (T * (T - 1))) if T > 1 else np.zeros(len(e))
        np.testing.assert_allclose(r["equity"], mean, rtol=1e-12, atol=0)
        np.testing.assert_allclose(r["equity_stderr"], se, rtol=1e-12, atol=0)
        if M:
            assert r["truncated"].sum() > 0 and (~fin).sum() == r["truncated"].sum()
        else:
            assert fin.all()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_invariance(env, positions):
    st, tu = positions
    sel = [0, 2, 5, 9, 10, 12, 14, 17]                       # forced, late-game and finished positions
    st, tu = st[sel], tu[sel]
    P, T = len(sel), 108
    args = dict(max_plies=0, rotate=True, seed=SEED, per_trial=True)
    base = _np(env.rollout(st, tu, T, outcomes=True, **args))
    assert set(base) == set(PLAIN) | set(OUT)
    assert env.rollout_info()[0] == 1024
    plain = _np(env.rollout(st, tu, T, **args))
    assert set(plain) == set(PLAIN)                          # without the keyword: exactly the keys it always had
    _assert_same(plain, base)
    again = _np(env.rollout_outcomes_read(per_trial=True))   # the read after a call that did not ask for outcomes
    _assert_same(again, base, OUT)
    for lanes in (64, 4096):
        _assert_same(base, _np(env.rollout(st, tu, T, lanes=lanes, outcomes=True, **args)))
        assert env.rollout_info()[0] == lanes
    _assert_same(base, _np(env.rollout(st, tu, T, outcomes=True, **args)))
    a = _np(env.rollout(st[:P // 2], tu[:P // 2], T, position_offset=0, outcomes=True, **args))
    b = _np(env.rollout(st[P // 2:], tu[P // 2:], T, position_offset=P // 2, outcomes=True, **args))
    _assert_same(base, {k: np.concatenate([a[k], b[k]]) for k in base})
    vr = _np(env.rollout(st, tu, T, outcomes=True, variance_reduction=True, **args))
    _assert_same(base, vr, PLAIN + OUT)
    # truncated trials too
    targs = dict(max_plies=5, rotate=True, seed=SEED, per_trial=True, outcomes=True)
    tb = _np(env.rollout(st, tu, T, **targs))
    assert tb["truncated"].sum() > 0 and (tb["trial_points"] == 0).sum() == tb["truncated"].sum()
    _assert_same(tb, _np(env.rollout(st, tu, T, lanes=64, **targs)))
    _assert_same(tb, _np(env.rollout(st, tu, T, variance_reduction=True, **targs)), PLAIN + OUT)
    _assert_same(tb, _np(env.rollout(st, tu, T, max_plies=5, rotate=True, seed=SEED, per_trial=True)), PLAIN)


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_plies", [0, 6])
def test_parity_with_the_fp64_reference(env, W, positions, max_plies):
    st, tu = positions[0][:16], positions[1][:16]
    T = 36
    r = _np(env.rollout(st, tu, T, max_plies=max_plies, rotate=True, seed=SEED, per_trial=True, outcomes=True))
    ref = np.zeros((16, T), np.int64)
    near = np.zeros((16, T), bool)
    for p in range(16):
        for i in range(T):
            ref[p, i], near[p, i] = OR.trial_points(W, st[p], tu[p], SEED, p * T + i, i, max_plies, True)
    cmp = ~near
    assert R.TIE_EPS == 2e-5
    assert cmp.mean() >= (0.9 if max_plies else 0.8), cmp.mean()
    # Positions 1a .. 7 (indices 0 .. 8) end on their first turn with a single candidate, or none: always compared.  Position 8 (index 9)
    # is forced only for the rolls holding a 1; after any other roll it plays on with real choices, so its trials may hold a near tie.
    assert cmp[:9].all()
    np.testing.assert_array_equal(r["trial_points"][cmp], ref[cmp])
    for c in CLASSES:
        assert (ref[cmp] == c).any(), c


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_and_side_effects(bg, W, positions):
    st, tu = positions
    a = bg.VecGame(64, seed=5)
    a.load_weights(W)
    with pytest.raises(bg.BgamdError):
        a.rollout_outcomes_read()
    a.run_greedy(7)
    snap, dice, stats, lc = a.snapshot().clone(), a.dice().clone(), a.stats(), a.last_choice()
    prog = [x.clone() for x in a.progress()]

    def unchanged():
        assert torch.equal(a.snapshot(), snap) and torch.equal(a.dice(), dice)
        assert all(torch.equal(x, y) for x, y in zip(a.progress(), prog))
        assert a.stats() == stats
        lc2 = a.last_choice()
        assert all(torch.equal(lc[k], lc2[k]) for k in lc)
    o = a.outcomes()
    np.testing.assert_array_equal(o.cpu().numpy(), OR.points_many(snap[:, :28].cpu().numpy()))
    unchanged()
    a.rollout(st[:4], tu[:4], 72, max_plies=7, seed=SEED, per_trial=True, outcomes=True)
    unchanged()
    bad = st[:2].copy()
    bad[1, 3] = 16
    with pytest.raises(bg.BgamdError, match="-5"):
        a.rollout(bad, tu[:2], 8, outcomes=True)
    with pytest.raises(bg.BgamdError):                       # a rollout that failed leaves nothing to read
        a.rollout_outcomes_read()
    a.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_arena_points(bg, W):
    from backgammon_env.arena import head_to_head
    e = bg.VecGame(256, seed=9)
    r = head_to_head(e, W, None)
    assert r["games"] == 512 and r["a_wins"] == r["a_as_p1"][1] + r["a_as_p2"][1] and r["a_as_p1"][0] + r["a_as_p2"][0] == r["games"]
    assert r["win_rate"] == r["a_wins"] / r["games"] and r["win_rate"] > 0.9
    for k in ("a_gammons", "a_backgammons", "b_gammons", "b_backgammons", "a_points"):
        assert isinstance(r[k], int) and (k == "a_points" or r[k] >= 0), k
    b_wins = r["games"] - r["a_wins"]
    a_single = r["a_wins"] - r["a_gammons"] - r["a_backgammons"]
    b_single = b_wins - r["b_gammons"] - r["b_backgammons"]
    assert a_single >= 0 and b_single >= 0
    assert r["a_points"] == a_single + 2 * r["a_gammons"] + 3 * r["a_backgammons"] - b_single - 2 * r["b_gammons"] - 3 * r["b_backgammons"]
    assert r["ppg"] == r["a_points"] / r["games"] and abs(r["ppg"]) <= 3
    assert r["ppg"] >= r["win_rate"] - 3 * (1 - r["win_rate"]) and r["a_gammons"] > 0               # (a net gammons a random mover)
    # the lanes are still frozen on the second pass's final boards (A was PLAYER2 there)
    o = e.outcomes().cpu().numpy()
    assert (o != 0).all() and int((o < 0).sum()) == r["a_as_p2"][1]
    e.close()


def test_rollout_moves_outcomes(bg, W, positions):
    from backgammon_env.analysis import rollout_moves
    st, tu = positions
    one = bg.VecGame(1, seed=3)
    one.load_weights(W)
    rng = np.random.RandomState(5)
    for p in (10, 13):
        dice = rng.randint(1, 7, 2)
        kw = dict(top_k=4, trials=72, max_plies=8, seed=SEED)
        plain = rollout_moves(one, st[p], int(tu[p]), dice, **kw)
        res = rollout_moves(one, st[p], int(tu[p]), dice, outcomes=True, **kw)
        assert len(res) == len(plain) >= 1
        for c, d in zip(res, plain):                         # the same ranking, the same plain numbers
            assert not {"equity", "equity_stderr", "counts"} & set(d)
            assert set(c) == set(d) | {"equity", "equity_stderr", "counts"}
            assert all(np.array_equal(c[k], d[k]) for k in d)
            q = _np(one.rollout(c["state"][None], [1 - int(tu[p])], 72, max_plies=8, rotate=True, seed=SEED, outcomes=True))
            assert c["equity"] == float(q["equity"][0]) and c["equity_stderr"] == float(q["equity_stderr"][0])
            assert c["counts"] == q["counts"][0].tolist() and len(c["counts"]) == 6 and sum(c["counts"]) == 72 - int(q["truncated"][0])
            assert abs(c["equity"]) <= 3
    one.close()
