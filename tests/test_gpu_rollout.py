"""Monte Carlo rollouts on the MI355X (bgamd_env_rollout, VecGame.rollout): trial for trial against the greedy step itself (plain, and
rotated + truncated), parity with the fp64 CPU reference (tests/rollout_ref.py), invariance to the lane count / repeated calls /
position_offset splits, the statistics, weight slots and the absence of side effects, the errors, and analysis.rollout_moves."""
import os

import numpy as np
import pytest

import rollout_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SEED = 4242


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
    return _greedy_positions(bg, W, 40, 11)


def _play_lanes(bg, W, state, turn, T, lane_offset, first_dice=None, max_plies=0):
    """T lanes of a fresh env with game ids lane_offset + lane, set to the position and stepped greedily without auto-reset until every
    lane is frozen (or max_plies turns).  -> (value [T] float64 (NaN: still running), turns [T], env)"""
    e = bg.VecGame(T, seed=SEED, lane_offset=lane_offset)
    e.load_weights(W)
    e.set_states(np.tile(state, (T, 1)), np.full(T, turn))
    k = 0
    if first_dice is not None:
        e.set_dice(first_dice)
        e.step_greedy(roll=False, auto_reset=False)
        k = 1
    limit = max_plies or 100000
    while k < limit:
        e.step_greedy(auto_reset=False)
        k += 1
        if k % 16 == 0 and bool(((e.flags() & 4) != 0).all()):
            break
    f = e.flags().cpu().numpy()
    ply = e.progress()[0].cpu().numpy()
    frozen = (f & 4) != 0
    value = np.where(frozen, np.where((f >> 1) & 1, 0.0, 1.0), np.nan)
    turns = np.where(frozen, ply + 1, ply)
    return value, turns, e


def test_trial_for_trial_against_the_greedy_step(bg, W, env, positions):
    st, tu = positions
    P, T = 8, 512
    r = env.rollout(st[:P], tu[:P], T, max_plies=0, rotate=False, seed=SEED, per_trial=True)
    tv, tt = r["trial_value"].cpu().numpy(), r["trial_turns"].cpu().numpy()
    assert (r["truncated"].cpu().numpy() == 0).all()
    for p in range(P):
        value, turns, e = _play_lanes(bg, W, st[p], int(tu[p]), T, p * T)
        e.close()
        assert not np.isnan(value).any()
        np.testing.assert_array_equal(tv[p], value.astype(np.float32), err_msg=f"position {p}")
        np.testing.assert_array_equal(tt[p], turns, err_msg=f"position {p}")


def test_rotation_and_truncation_against_the_greedy_step(bg, W, env, positions):
    st, tu = positions
    P, T, M = 4, 360, 9
    r = env.rollout(st[8:8 + P], tu[8:8 + P], T, max_plies=M, rotate=True, seed=SEED, position_offset=3, per_trial=True)
    tv, tt = r["trial_value"].cpu().numpy(), r["trial_turns"].cpu().numpy()
    i = np.arange(T)
    dice = np.stack([1 + (i % 36) // 6, 1 + (i % 36) % 6], 1).astype(np.int32)
    n_trunc = 0
    for p in range(P):
        value, turns, e = _play_lanes(bg, W, st[8 + p], int(tu[8 + p]), T, (3 + p) * T, first_dice=dice, max_plies=M)
        running = np.isnan(value)
        if running.any():
            ev = e.evaluate(e.states(), e.turns()).cpu().numpy()
            value = np.where(running, ev, value)
        e.close()
        n_trunc += int(running.sum())
        assert int(r["truncated"][p]) == int(running.sum())
        assert (turns[running] == M).all()
        np.testing.assert_array_equal(tv[p], value.astype(np.float32), err_msg=f"position {p}")
        np.testing.assert_array_equal(tt[p], turns, err_msg=f"position {p}")
    assert n_trunc > 0


@pytest.mark.parametrize("max_plies", [0, 6])
def test_parity_with_the_fp64_reference(bg, W, env, max_plies):
    # positions from later in the game: every decision of a trial risks a near tie (2e-5), and whole games from early positions have
    # so many decisions that fewer than 90 % of the trials would be compared
    st1, tu1 = _greedy_positions(bg, W, 40, 13, skip=40)
    g10 = np.load(os.path.join(ROOT, "tests", "golden", "g10_arbitrary_boards.npz"))
    idx = np.arange(24) * (len(g10["boards"]) // 24)
    st = np.concatenate([st1, g10["boards"][idx]]).astype(np.int32)
    tu = np.concatenate([tu1, g10["dice"][idx, 0]]).astype(np.int32)
    if max_plies == 0:                                 # (whole games cost the CPU reference ~20 ms each: every other position)
        st, tu = st[::2], tu[::2]
    T = 36
    r = env.rollout(st, tu, T, max_plies=max_plies, rotate=True, seed=SEED, per_trial=True)
    tv, tt = r["trial_value"].cpu().numpy(), r["trial_turns"].cpu().numpy()
    ref = R.rollout(W, st, tu, T, SEED, max_plies=max_plies, rotate=True)
    cmp = ~ref["near_tie"]
    # a whole game has ~40-80 decisions, each a chance of a near tie: 85 % of these trials are compared (measured), 96 % at M = 6
    assert cmp.mean() >= (0.9 if max_plies else 0.8), cmp.mean()
    trunc = ref["truncated"] & cmp
    full = ~ref["truncated"] & cmp
    np.testing.assert_array_equal(tt[cmp], ref["turns"][cmp])
    np.testing.assert_array_equal(tv[full], ref["value"][full])
    if max_plies:
        assert trunc.sum() > 0
        np.testing.assert_allclose(tv[trunc], ref["value"][trunc], atol=1e-5, rtol=0)


def _stats(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _assert_same(a, b):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_invariance_to_lanes_calls_and_offsets(env, positions):
    st, tu = positions
    P, T = 8, 256
    args = dict(max_plies=0, rotate=True, seed=SEED, per_trial=True)
    base = _stats(env.rollout(st[:P], tu[:P], T, **args))
    assert env.rollout_info()[0] == 2048
    for lanes in (64, 4096):
        _assert_same(base, _stats(env.rollout(st[:P], tu[:P], T, lanes=lanes, **args)))
        assert env.rollout_info()[0] == lanes
    _assert_same(base, _stats(env.rollout(st[:P], tu[:P], T, **args)))
    a = _stats(env.rollout(st[:P // 2], tu[:P // 2], T, position_offset=0, **args))
    b = _stats(env.rollout(st[P // 2:P], tu[P // 2:P], T, position_offset=P // 2, **args))
    _assert_same(base, {k: np.concatenate([a[k], b[k]]) for k in base})
    # truncated trials too
    tb = _stats(env.rollout(st[:P], tu[:P], T, max_plies=5, rotate=True, seed=SEED, per_trial=True))
    _assert_same(tb, _stats(env.rollout(st[:P], tu[:P], T, max_plies=5, rotate=True, seed=SEED, per_trial=True, lanes=64)))


def test_statistics_match_the_per_trial_outputs(env, positions):
    st, tu = positions
    for T, M in ((100, 0), (72, 4), (1, 0)):
        r = _stats(env.rollout(st[:6], tu[:6], T, max_plies=M, rotate=False, seed=SEED + T, per_trial=True))
        x = r["trial_value"].astype(np.float64)
        mean = x.sum(1) / T
        se = np.sqrt(((x - mean[:, None]) ** 2).sum(1) / (T * (T - 1))) if T > 1 else np.zeros(len(x))
        np.testing.assert_allclose(r["mean"], mean, rtol=1e-12, atol=0)
        np.testing.assert_allclose(r["stderr"], se, rtol=1e-12, atol=0)
        np.testing.assert_array_equal(r["turns"], r["trial_turns"].astype(np.int64).sum(1))
        if M:                                          # (a game may also end on its M-th turn)
            assert (r["truncated"] <= (r["trial_turns"] == M).sum(1)).all() and r["truncated"].sum() > 0
        else:
            assert (r["truncated"] == 0).all()


def test_weight_slots_and_no_side_effects(bg, W, positions):
    st, tu = positions
    Wb = (W * np.float32(0.97)).astype(np.float32)
    a, twin = bg.VecGame(64, seed=5), bg.VecGame(64, seed=5)
    for e in (a, twin):
        e.load_weights(W)
        e.run_greedy(7)
    a.load_weights(Wb, slot=1)
    twin.load_weights(Wb, slot=1)
    snap, dice, stats, lc = a.snapshot().clone(), a.dice().clone(), a.stats(), a.last_choice()
    prog = [x.clone() for x in a.progress()]
    r1 = _stats(a.rollout(st[:4], tu[:4], 72, max_plies=7, seed=SEED, slot=1, per_trial=True))
    assert torch.equal(a.snapshot(), snap) and torch.equal(a.dice(), dice)
    assert all(torch.equal(x, y) for x, y in zip(a.progress(), prog))
    assert a.stats() == stats
    lc2 = a.last_choice()
    assert all(torch.equal(lc[k], lc2[k]) for k in lc)
    a.step_greedy()
    twin.step_greedy()
    assert torch.equal(a.snapshot(), twin.snapshot())
    b = bg.VecGame(64, seed=5)
    b.load_weights(Wb)
    r0 = _stats(b.rollout(st[:4], tu[:4], 72, max_plies=7, seed=SEED, slot=0, per_trial=True))
    _assert_same(r1, r0)
    rW = _stats(a.rollout(st[:4], tu[:4], 72, max_plies=7, seed=SEED, slot=0, per_trial=True))
    assert not np.array_equal(rW["trial_value"], r1["trial_value"])
    for e in (a, twin, b):
        e.close()


def test_errors(bg, W, env, positions):
    st, tu = positions
    with pytest.raises(bg.BgamdError):
        env.rollout(st[:0], tu[:0], 8)
    for kw in (dict(trials=0), dict(trials=8, max_plies=-1), dict(trials=8, lanes=-1), dict(trials=1 << 31)):
        with pytest.raises(bg.BgamdError):
            env.rollout(st[:1], tu[:1], **kw)
    bad = st[:2].copy()
    bad[1, 3] = 16
    with pytest.raises(bg.BgamdError, match="-5"):
        env.rollout(bad, tu[:2], 8)
    e = bg.VecGame(64, seed=1)
    with pytest.raises(bg.BgamdError, match="-6"):
        e.rollout(st[:1], tu[:1], 8)
    e.load_weights(W)
    with pytest.raises(bg.BgamdError, match="-6"):
        e.rollout(st[:1], tu[:1], 8, slot=1)
    e.close()


def test_rollout_moves(bg, W, positions):
    from backgammon_env.analysis import rollout_moves
    st, tu = positions
    one = bg.VecGame(1, seed=3)
    one.load_weights(W)
    ref = bg.VecGame(1, seed=3)
    ref.load_weights(W)
    rng = np.random.RandomState(5)
    for p in (2, 9, 17):
        dice = rng.randint(1, 7, 2)
        res = rollout_moves(one, st[p], int(tu[p]), dice, top_k=4, trials=72, max_plies=0, seed=SEED)
        ref.set_states(st[p][None], [int(tu[p])])
        ref.set_dice(dice[None])
        ref.step_search(top_k=4, roll=False, auto_reset=False, no_flip=True)
        cst, v1, v2, kept = (x.cpu().numpy() for x in ref.search_candidates())
        assert len(res) == int(kept[0])
        got = {tuple(c["state"]): c for c in res}
        assert set(got) == {tuple(cst[0, k]) for k in range(int(kept[0]))}
        for k in range(int(kept[0])):
            c = got[tuple(cst[0, k])]
            assert c["v1"] == float(v1[0, k]) and c["v2"] == float(v2[0, k])
            d = ref.rollout(cst[0, k][None], [1 - int(tu[p])], 72, max_plies=0, rotate=True, seed=SEED)
            assert c["mean"] == float(d["mean"][0]) and c["stderr"] == float(d["stderr"][0]) and c["turns"] == int(d["turns"][0])
        means = [c["mean"] for c in res]
        assert means == sorted(means, reverse=int(tu[p]) == 0)
        ref.set_states(st[p][None], [int(tu[p])])
        _, _, est, _, _ = ref.enumerate(player=[int(tu[p])], dice=dice[None])
        for c in res:
            assert (est[c["index"]].cpu().numpy() == c["state"]).all()
    one.close()
    ref.close()
