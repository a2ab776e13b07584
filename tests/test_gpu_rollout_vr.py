"""The 1-ply pre-roll evaluation and the luck-adjusted rollouts on the MI355X (bgamd_env_evaluate_preroll, BGAMD_ROLLOUT_VR): f against
the greedy step itself, the fp64 reference (tests/rollout_vr_ref.py) and the 2-ply search's V2; luck-adjusted rollouts leave the played
trials unchanged, match a lane-by-lane replay bit for bit, do not depend on the lane count / repeated calls / position_offset splits,
reduce to the per-trial outputs, agree with the reference, are unbiased and shrink the variance; side effects, errors, rollout_moves."""
import os

import numpy as np
import pytest

import rollout_ref as R
import rollout_vr_ref as V
import search_ref as S
from test_gpu_rollout import SEED, _greedy_positions

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
W21 = np.array(S.ROLL_W)
IDX = np.zeros((7, 7), np.int64)                     # IDX[d1, d2] = index of the unordered roll in ROLLS
for _a in range(1, 7):
    for _b in range(1, 7):
        IDX[_a, _b] = V.roll_index(_a, _b)


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


@pytest.fixture(scope="module")
def positions(bg, W):
    return _greedy_positions(bg, W, 40, 11)


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _assert_same(a, b, keys=None):
    for k in keys or a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_roll_order(bg):
    assert bg.ROLLS == S.ROLLS


def test_preroll_against_the_greedy_step(bg, W, env, positions):
    st, tu = positions
    P = len(st)
    f, m = (x.cpu().numpy() for x in env.evaluate_preroll(st, tu))
    assert f.shape == (P, 21) and f.dtype == np.float32 and m.dtype == np.float64
    # every (position, roll) as a lane of an env stepped greedily with the roll's dice injected
    e = bg.VecGame(P * 21, seed=3)
    e.load_weights(W)
    e.set_states(np.repeat(st, 21, 0), np.repeat(tu, 21))
    e.set_dice(np.tile(np.array(S.ROLLS, np.int32), (P, 1)))
    e.step_greedy(roll=False, auto_reset=False, no_flip=True)
    lc = {k: v.cpu().numpy() for k, v in e.last_choice().items()}
    e.close()
    moved = (lc["seq_len"] > 0).reshape(P, 21)
    assert moved.mean() > 0.5
    np.testing.assert_array_equal(f[moved], lc["value"].reshape(P, 21)[moved])
    if (~moved).any():
        p = np.nonzero(~moved)[0]
        ev = env.evaluate(st[p], tu[p]).cpu().numpy()
        np.testing.assert_allclose(f[~moved], ev, atol=1e-6, rtol=0)
    np.testing.assert_allclose(m, f.astype(np.float64) @ W21, atol=1e-12, rtol=0)


def _ties(W, s, turn):
    """[21] bool: the roll's greedy choice has its best two distinct values within rollout_ref.TIE_EPS."""
    out = []
    for a, b in S.ROLLS:
        cand = S.distinct_afterstates(s, turn, a, b)
        u = np.unique(S.net(W, cand, turn)) if len(cand) else np.zeros(0)
        out.append(len(u) > 1 and abs(float(u[-1] - u[-2]) if turn == 0 else float(u[1] - u[0])) < R.TIE_EPS)
    return np.array(out)


def test_preroll_against_the_fp64_reference(bg, W, env, positions):
    st, tu = positions
    g10 = np.load(os.path.join(ROOT, "tests", "golden", "g10_arbitrary_boards.npz"))
    idx = np.arange(12) * (len(g10["boards"]) // 12)
    s_all = np.concatenate([st[::2], g10["boards"][idx]]).astype(np.int32)
    t_all = np.concatenate([tu[::2], g10["dice"][idx, 0]]).astype(np.int32)
    # a position that is over: its outcome for every roll
    over = np.zeros(28, np.int32)
    over[27] = 15; over[19:24] = 3
    s_all = np.concatenate([s_all, over[None]])
    t_all = np.concatenate([t_all, [0]]).astype(np.int32)
    f, m = (x.cpu().numpy() for x in env.evaluate_preroll(s_all, t_all))
    n_cmp = 0
    for q in range(len(s_all)):
        rf, rm = V.preroll(W, s_all[q], int(t_all[q]))
        ok = ~_ties(W, s_all[q], int(t_all[q])) if R.over_code(s_all[q]) == 0 else np.ones(21, bool)
        n_cmp += int(ok.sum())
        np.testing.assert_allclose(f[q][ok], rf[ok], atol=1e-5, rtol=0, err_msg=f"position {q}")
        if ok.all():
            assert abs(m[q] - rm) < 1e-5
    assert (f[-1] == 0.0).all() and m[-1] == 0.0
    assert n_cmp >= 0.9 * 21 * len(s_all)


def test_preroll_against_the_search(bg, W, positions):
    st, tu = positions
    n = len(st)
    e = bg.VecGame(n, seed=9)
    e.load_weights(W)
    e.set_states(st, tu)
    dice = np.random.RandomState(2).randint(1, 7, (n, 2))
    e.set_dice(dice)
    e.step_search(top_k=8, roll=False, auto_reset=False, no_flip=True)
    cst, v1, v2, kept = (x.cpu().numpy() for x in e.search_candidates())
    rows, opp, want = [], [], []
    for g in range(n):
        for k in range(int(kept[g])):
            if R.over_code(cst[g, k]):                 # a terminal candidate scores its outcome, not a pre-roll mean
                continue
            rows.append(cst[g, k]); opp.append(1 - int(tu[g])); want.append(v2[g, k])
    _, m = e.evaluate_preroll(np.array(rows), np.array(opp, np.int32))
    e.close()
    assert len(rows) > 100
    np.testing.assert_allclose(m.cpu().numpy(), np.array(want, np.float64), atol=1e-6, rtol=0)


PLAIN = ("mean", "stderr", "turns", "truncated", "trial_value", "trial_turns")
VR = ("vr_mean", "vr_stderr", "trial_luck")


@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("max_plies", [0, 7])
def test_played_trials_are_unchanged(env, positions, rotate, max_plies):
    st, tu = positions
    args = dict(max_plies=max_plies, rotate=rotate, seed=SEED, per_trial=True)
    a = _np(env.rollout(st[:4], tu[:4], 144, **args))
    ia = env.rollout_info()
    b = _np(env.rollout(st[:4], tu[:4], 144, variance_reduction=True, **args))
    assert env.rollout_info() == ia
    _assert_same(a, b, PLAIN)
    assert set(b) == set(PLAIN) | set(VR)


def _replay(bg, W, state, turn, T, lane_offset, first_dice=None, max_plies=0):
    """The _play_lanes pattern of test_gpu_rollout.py with the luck: before every step_greedy the live lanes' positions go through
    evaluate_preroll, and after it the dice the step played give each live lane's luck, summed in fp64 in turn order.
    -> (value [T] (NaN: still running), luck [T])"""
    e = bg.VecGame(T, seed=SEED, lane_offset=lane_offset)
    e.load_weights(W)
    e.set_states(np.tile(state, (T, 1)), np.full(T, turn))
    luck = np.zeros(T)
    ar = np.arange(T)
    k = 0
    limit = max_plies or 100000
    while k < limit:
        live = (e.flags().cpu().numpy() & 4) == 0
        if not live.any():
            break
        f, m = (x.cpu().numpy() for x in e.evaluate_preroll(e.states(), e.turns()))
        if k == 0 and first_dice is not None:
            e.set_dice(first_dice)
            e.step_greedy(roll=False, auto_reset=False)
        else:
            e.step_greedy(auto_reset=False)
        d = e.dice().cpu().numpy()
        lk = f[ar, IDX[d[:, 0], d[:, 1]]].astype(np.float64) - m
        luck[live] = luck[live] + lk[live]
        k += 1
    fl = e.flags().cpu().numpy()
    frozen = (fl & 4) != 0
    value = np.where(frozen, np.where((fl >> 1) & 1, 0.0, 1.0), np.nan)
    running = np.isnan(value)
    if running.any():
        value = np.where(running, e.evaluate(e.states(), e.turns()).cpu().numpy(), value)
    e.close()
    return value, luck


@pytest.mark.parametrize("rotate,max_plies", [(False, 0), (True, 9)])
def test_luck_against_a_lane_by_lane_replay(bg, W, env, positions, rotate, max_plies):
    st, tu = positions
    P, T, off = 3, 144, 5
    r = _np(env.rollout(st[20:20 + P], tu[20:20 + P], T, max_plies=max_plies, rotate=rotate, seed=SEED, position_offset=off,
                        per_trial=True, variance_reduction=True))
    i = np.arange(T)
    first = np.stack([1 + (i % 36) // 6, 1 + (i % 36) % 6], 1).astype(np.int32) if rotate else None
    for p in range(P):
        value, luck = _replay(bg, W, st[20 + p], int(tu[20 + p]), T, (off + p) * T, first, max_plies)
        np.testing.assert_array_equal(r["trial_value"][p], value.astype(np.float32), err_msg=f"position {p}")
        np.testing.assert_array_equal(r["trial_luck"][p], luck, err_msg=f"position {p}")
        assert np.count_nonzero(luck) > T // 2


def test_invariance_to_lanes_calls_and_offsets(env, positions):
    st, tu = positions
    P, T = 8, 256
    args = dict(max_plies=0, rotate=True, seed=SEED, per_trial=True, variance_reduction=True)
    base = _np(env.rollout(st[:P], tu[:P], T, **args))
    for lanes in (256, 4096):
        _assert_same(base, _np(env.rollout(st[:P], tu[:P], T, lanes=lanes, **args)))
    _assert_same(base, _np(env.rollout(st[:P], tu[:P], T, **args)))
    a = _np(env.rollout(st[:P // 2], tu[:P // 2], T, position_offset=0, **args))
    b = _np(env.rollout(st[P // 2:P], tu[P // 2:P], T, position_offset=P // 2, **args))
    _assert_same(base, {k: np.concatenate([a[k], b[k]]) for k in base})


def test_statistics_match_the_per_trial_outputs(env, positions):
    st, tu = positions
    for T, M, rot in ((100, 0, False), (72, 4, True), (1, 0, False)):
        r = _np(env.rollout(st[:6], tu[:6], T, max_plies=M, rotate=rot, seed=SEED + T, per_trial=True, variance_reduction=True))
        y = r["trial_value"].astype(np.float64) - r["trial_luck"]
        mean = y.sum(1) / T
        se = np.sqrt(((y - mean[:, None]) ** 2).sum(1) / (T * (T - 1))) if T > 1 else np.zeros(len(y))
        np.testing.assert_allclose(r["vr_mean"], mean, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(r["vr_stderr"], se, rtol=1e-12, atol=1e-15)
        # without per_trial: the same statistics
        q = _np(env.rollout(st[:6], tu[:6], T, max_plies=M, rotate=rot, seed=SEED + T, variance_reduction=True))
        _assert_same(r, q, ("vr_mean", "vr_stderr"))


@pytest.mark.parametrize("max_plies", [0, 6])
def test_luck_parity_with_the_fp64_reference(bg, W, env, max_plies):
    # (the reference scores 21 rolls per turn, ~20 ms each, so few whole games: from fixture boards, whose games have fewer near ties
    # than those from greedy-play positions -- 81 % of these 32 trials are compared, against 71 % of 48 from greedy play)
    if max_plies == 0:
        g10 = np.load(os.path.join(ROOT, "tests", "golden", "g10_arbitrary_boards.npz"))
        idx = np.arange(8) * (len(g10["boards"]) // 24)
        st, tu, T = g10["boards"][idx].astype(np.int32), g10["dice"][idx, 0].astype(np.int32), 4
    else:
        st, tu = _greedy_positions(bg, W, 12, 13, skip=40)
        T = 8
    r = _np(env.rollout(st, tu, T, max_plies=max_plies, rotate=True, seed=SEED, per_trial=True, variance_reduction=True))
    ref = V.rollout(W, st, tu, T, SEED, max_plies=max_plies, rotate=True)
    cmp = ~ref["near_tie"]
    print(f"M={max_plies}: {cmp.mean():.3f} of {cmp.size} trials compared")
    assert cmp.mean() >= (0.9 if max_plies else 0.8), cmp.mean()
    np.testing.assert_array_equal(r["trial_turns"][cmp], ref["turns"][cmp])
    np.testing.assert_allclose(r["trial_luck"][cmp], ref["luck"][cmp], atol=1e-4, rtol=0)


def test_unbiased_and_variance_reduced(bg, W, env):
    g10 = np.load(os.path.join(ROOT, "tests", "golden", "g10_arbitrary_boards.npz"))
    idx = np.arange(16) * (len(g10["boards"]) // 16)
    st, tu = g10["boards"][idx].astype(np.int32), g10["dice"][idx, 0].astype(np.int32)
    T = 2592
    r = _np(env.rollout(st, tu, T, max_plies=7, rotate=True, seed=SEED, per_trial=True, variance_reduction=True))
    L = r["trial_luck"]
    se_L = L.std(1, ddof=1) / np.sqrt(T)
    assert (np.abs(L.mean(1)) <= 4 * se_L).all(), (L.mean(1), se_L)
    live = r["stderr"] > 0
    ratio = float((r["stderr"][live] ** 2).sum() / (r["vr_stderr"][live] ** 2).sum())
    print(f"pooled variance ratio (stderr / vr_stderr)^2 at M = 7: {ratio:.3f}; per position: "
          f"{np.round(r['stderr'][live] ** 2 / r['vr_stderr'][live] ** 2, 2).tolist()}")
    assert ratio > 1.0


def test_no_side_effects(bg, W, positions):
    st, tu = positions
    a = bg.VecGame(64, seed=5)
    a.load_weights(W)
    a.run_greedy(7)
    a.step_search(top_k=4)
    snap, dice, stats, lc = a.snapshot().clone(), a.dice().clone(), a.stats(), a.last_choice()
    prog = [x.clone() for x in a.progress()]
    sc = a.search_candidates()
    a.evaluate_preroll(st[:8], tu[:8])
    a.rollout(st[:4], tu[:4], 72, max_plies=5, seed=SEED, variance_reduction=True)
    assert torch.equal(a.snapshot(), snap) and torch.equal(a.dice(), dice)
    assert all(torch.equal(x, y) for x, y in zip(a.progress(), prog))
    assert a.stats() == stats
    lc2 = a.last_choice()
    assert all(torch.equal(lc[k], lc2[k]) for k in lc)
    assert all(torch.equal(x, y) for x, y in zip(a.search_candidates(), sc))
    a.close()


def test_errors(bg, W, env, positions):
    from backgammon_env import _capi
    st, tu = positions

    def vr_read(e):
        _capi.check(e._lib.bgamd_env_rollout_vr_read(e._h, None, None, None, None), "rollout_vr_read")
    e = bg.VecGame(64, seed=1)
    with pytest.raises(bg.BgamdError, match="-6"):
        e.evaluate_preroll(st[:1], tu[:1])
    with pytest.raises(bg.BgamdError, match="-6"):
        e.rollout(st[:1], tu[:1], 8, variance_reduction=True)
    e.load_weights(W)
    with pytest.raises(bg.BgamdError, match="-6"):
        e.evaluate_preroll(st[:1], tu[:1], slot=1)
    with pytest.raises(bg.BgamdError, match="-1"):
        vr_read(e)                                     # before any rollout
    e.rollout(st[:1], tu[:1], 8, variance_reduction=True)
    vr_read(e)
    e.rollout(st[:1], tu[:1], 8)
    with pytest.raises(bg.BgamdError, match="-1"):
        vr_read(e)                                     # after a plain one
    bad = st[:2].copy()
    bad[1, 3] = 16
    with pytest.raises(bg.BgamdError, match="-5"):
        e.evaluate_preroll(bad, tu[:2])
    with pytest.raises(bg.BgamdError, match="-5"):
        e.rollout(bad, tu[:2], 8, variance_reduction=True)
    with pytest.raises(bg.BgamdError):
        e.evaluate_preroll(st[:0], tu[:0])
    s1 = torch.as_tensor(st[:1]).cuda()
    for fl in (2, 128, 256):
        assert e._lib.bgamd_env_evaluate_preroll(e._h, fl, s1.data_ptr(), None, 1, None, None, None) == -1
    assert e._lib.bgamd_env_rollout(e._h, 512, s1.data_ptr(), None, 1, 0, 8, 0, 1, 0, *([None] * 7)) == -1
    e.close()


def test_rollout_moves(bg, W, positions):
    from backgammon_env.analysis import rollout_moves
    st, tu = positions
    one = bg.VecGame(1, seed=3)
    one.load_weights(W)
    ref = bg.VecGame(1, seed=3)
    ref.load_weights(W)
    rng = np.random.RandomState(6)
    for p in (4, 23):
        dice = rng.randint(1, 7, 2)
        args = dict(top_k=4, trials=72, max_plies=0, seed=SEED)
        plain = rollout_moves(one, st[p], int(tu[p]), dice, **args)
        res = rollout_moves(one, st[p], int(tu[p]), dice, variance_reduction=True, **args)
        by_state = {tuple(c["state"]): c for c in plain}
        assert set(by_state) == {tuple(c["state"]) for c in res}
        for c in res:
            pc = by_state[tuple(c["state"])]
            assert {k: v for k, v in c.items() if k not in ("vr_mean", "vr_stderr", "state")} == \
                   {k: v for k, v in pc.items() if k != "state"}
            d = ref.rollout(c["state"][None], [1 - int(tu[p])], 72, max_plies=0, rotate=True, seed=SEED, variance_reduction=True)
            assert c["vr_mean"] == float(d["vr_mean"][0]) and c["vr_stderr"] == float(d["vr_stderr"][0])
        vm = [c["vr_mean"] for c in res]
        assert vm == sorted(vm, reverse=int(tu[p]) == 0)
    one.close()
    ref.close()
