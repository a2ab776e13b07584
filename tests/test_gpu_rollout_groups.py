"""Rollouts on shared dice on the MI355X (bgamd_env_rollout_grouped, bgamd_env_rollout_paired_read; VecGame.rollout(groups=...),
VecGame.rollout_paired, analysis.rollout_decisions).  The yardstick everywhere is the plain rollout of ONE position at
position_offset = group_offset + group[p] -- the path tests/test_gpu_rollout*.py verify trial by trial -- and every comparison with it
is bit for bit.  The paired statistics are compared with exactly rounded sums over the per-trial outputs, inside the bounds
tests/test_rollout_groups_cpu.py derives for the device's order.  The tables (tests/rollout_group_model.py) and the conditions they
meet are checked on the CPU there."""
import math

import numpy as np
import pytest

import outcome_ref as OR
import rollout_cases as RC
import rollout_group_model as GM

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = RC.SEED
PLAIN = ("mean", "stderr", "turns", "truncated", "trial_value", "trial_turns", "counts", "equity", "equity_stderr", "trial_points")
LUCK = ("vr_mean", "vr_stderr", "trial_luck")
POLICY = dict(plies=2, top_k=2, margin=0.04)
_REF = {}                                              # the singles of a case, computed once per session


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


@pytest.fixture(scope="module")
def W():
    return RC.weights()


@pytest.fixture(scope="module")
def env(bg, W):
    e = bg.VecGame(64, seed=7)
    e.load_weights(W)
    yield e
    assert e.stats()["error_flags"] == 0
    e.close()


@pytest.fixture(scope="module")
def single(bg, W):
    """the env of the yardstick's single-position calls (its own, so that neither env re-creates its trial lanes call after call)"""
    e = bg.VecGame(64, seed=9)
    e.load_weights(W)
    yield e
    assert e.stats()["error_flags"] == 0
    e.close()


@pytest.fixture(scope="module")
def main():
    st, tu, _ = GM.main_positions()
    return st, tu


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _assert_same(a, b, keys=None):
    for k in keys or sorted(set(a) | set(b)):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _call(e, st, tu, T, rotate, M, **kw):
    return _np(e.rollout(st, tu, T, max_plies=M, rotate=rotate, seed=SEED, per_trial=True, outcomes=True, **kw))


def _singles(single, tag, st, tu, groups, offset, T, rotate, M, **kw):
    """position p alone at position_offset = offset + groups[p], for every p, stacked"""
    key = (tag, tuple(groups), offset, T, rotate, M, tuple(sorted(kw.items())))
    if key not in _REF:
        rows = [_call(single, st[p:p + 1], tu[p:p + 1], T, rotate, M, position_offset=offset + int(groups[p]), **kw) for p in range(len(st))]
        _REF[key] = {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}
        for v in _REF[key].values():
            v.setflags(write=False)
    return _REF[key]


# ---- grouped against singles; any lane count ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [64, 256, 0])
@pytest.mark.parametrize("T,rotate,M", GM.CASES)
def test_grouped_against_singles(env, single, main, T, rotate, M, lanes):
    st, tu = main
    ref = _singles(single, "main", st, tu, GM.GROUPS, GM.GROUP_OFFSET, T, rotate, M)
    r = _call(env, st, tu, T, rotate, M, groups=GM.GROUPS, group_offset=GM.GROUP_OFFSET, lanes=lanes)
    assert env.rollout_info()[0] == (lanes or RC.default_lanes(len(st) * T))
    if lanes == 64:
        assert len(st) * T > 3 * lanes                   # several times more trials than lanes: the refill seats grouped trials too
    assert set(r) == set(PLAIN)
    _assert_same(r, ref, PLAIN)
    over = list(GM.main_positions()[2]).index("over")
    assert (r["trial_turns"][over] == 0).all() and r["stderr"][over] == 0.0
    if M:
        assert r["truncated"].sum() > 0


def test_identity_groups_and_none_are_the_plain_rollout(env, main):
    st, tu = main
    P = len(st)
    for T, rotate, M in GM.CASES[1:]:
        plain = _call(env, st, tu, T, rotate, M, position_offset=GM.GROUP_OFFSET)
        _assert_same(_call(env, st, tu, T, rotate, M, groups=np.arange(P), group_offset=GM.GROUP_OFFSET), plain, PLAIN)
        _assert_same(_call(env, st, tu, T, rotate, M, groups=torch.arange(P) + GM.GROUP_OFFSET), plain, PLAIN)
        _assert_same(_call(env, st, tu, T, rotate, M, groups=None, position_offset=GM.GROUP_OFFSET), plain, PLAIN)


def test_twins(env):
    st, tu = GM.twin_positions()
    T = 36
    r = _np(env.rollout(st, tu, T, max_plies=6, rotate=True, seed=SEED, per_trial=True, outcomes=True, variance_reduction=True,
                        groups=GM.TWIN_GROUPS))
    for k in PLAIN + LUCK:                                # the same position on the same dice: the same trials
        np.testing.assert_array_equal(r[k][0], r[k][1], err_msg=k)
    # ... and on other dice other trials (rotation fixes turn 0 only)
    assert (r["trial_value"][0] != r["trial_value"][2]).any()
    for which in ("value", "vr", "equity"):
        dm, ds = (x.cpu().numpy() for x in env.rollout_paired([1, 0, 2], which))
        assert (dm == 0.0).all() and (ds == 0.0).all() and not np.signbit(dm).any(), which
        dm, ds = (x.cpu().numpy() for x in env.rollout_paired([2, 2, 0], which))
        assert np.isnan(dm).all() and np.isnan(ds).all(), which


# ---- the paired read ---------------------------------------------------------------------------------------------------------------------

def _quantities(r):
    """fp64 per-trial quantities [P][T] by `which`, from the per-trial outputs"""
    x = r["trial_value"].astype(np.float64)
    q = {"value": x, "equity": np.where(r["trial_points"] != 0, r["trial_points"].astype(np.float64), 2.0 * x - 1.0)}
    if "trial_luck" in r:
        q["vr"] = x - r["trial_luck"]
    return q


def _check_paired(env, r, groups, ref, T):
    q = _quantities(r)
    out = {}
    for which in q:
        dm, ds = (x.cpu().numpy() for x in env.rollout_paired(ref, which))
        for p in range(len(groups)):
            m, se = GM.paired_fsum(q[which].tolist(), groups, p, int(ref[p]))
            assert GM.close(float(dm[p]), m, T), (which, p, dm[p], m)
            assert GM.close(float(ds[p]), se, T, stderr=True), (which, p, ds[p], se)
            if int(ref[p]) == p:
                assert dm[p] == 0.0 and ds[p] == 0.0
        out[which] = (dm, ds)
    return out


def test_paired_read(env, main):
    st, tu = main
    g, P = GM.GROUPS, len(GM.GROUPS)
    T, rotate, M = GM.CASES[2]
    r = _call(env, st, tu, T, rotate, M, groups=g, group_offset=GM.GROUP_OFFSET, variance_reduction=True, lanes=256)
    first = [g.index(x) for x in g]                       # every position against its group's first member
    last = [P - 1 - g[::-1].index(x) for x in g]
    base = _check_paired(env, r, g, first, T)
    _check_paired(env, r, g, last, T)
    _check_paired(env, r, g, list(range(P)), T)
    assert all(np.isfinite(base[w][0]).all() and (base[w][1][[2, 4, 5]] > 0).all() for w in base)
    # references that pair nothing: out of range on either side, and in another group -- NaN there, the other rows as before
    bad = list(first)
    bad[0], bad[2], bad[4], bad[6] = -1, P, 2 ** 31 - 1, 0
    got = _check_paired(env, r, g, bad, T)
    for w in got:
        for k in (0, 1):
            assert np.isnan(got[w][k][[0, 2, 4, 6]]).all()
            np.testing.assert_array_equal(got[w][k][[1, 3, 5]], base[w][k][[1, 3, 5]])
    # the paired error of a live pair credits the shared dice: it is not the unpaired one
    x = _quantities(r)["value"].tolist()
    assert not GM.close(GM.unpaired_stderr(x, 2, 0), float(base["value"][1][2]), T, stderr=True)
    # the read changes nothing that the rollout or the other reads return
    again = _np(env.rollout_outcomes_read(per_trial=True))
    _assert_same(again, {k: r[k] for k in again})


def test_paired_read_one_trial_and_ungrouped(bg, env, main):
    st, tu = main
    g, P = GM.GROUPS, len(GM.GROUPS)
    first = [g.index(x) for x in g]
    r = _call(env, st, tu, 1, True, 3, groups=g, group_offset=GM.GROUP_OFFSET)
    got = _check_paired(env, r, g, first, 1)
    assert all((got[w][1] == 0.0).all() for w in got)
    # an ungrouped rollout: the table is the identity, only p itself shares p's dice
    r = _call(env, st, tu, 36, True, 2, position_offset=1)
    for which in ("value", "equity"):
        dm, ds = (x.cpu().numpy() for x in env.rollout_paired(list(range(P)), which))
        assert (dm == 0.0).all() and (ds == 0.0).all()
        for shift in range(1, P):
            dm, ds = (x.cpu().numpy() for x in env.rollout_paired([(p + shift) % P for p in range(P)], which))
            assert np.isnan(dm).all() and np.isnan(ds).all()
    _check_paired(env, r, list(range(P)), first, 36)


# ---- the other routes: luck adjustment, the 2-ply policy ----------------------------------------------------------------------------------

def test_luck_adjusted(env, single, main):
    st, tu = main
    T, M = 36, 2
    ref = _singles(single, "vr", st, tu, GM.GROUPS, GM.GROUP_OFFSET, T, True, M, variance_reduction=True, lanes=64)
    r = _call(env, st, tu, T, True, M, groups=GM.GROUPS, group_offset=GM.GROUP_OFFSET, variance_reduction=True, lanes=64)
    _assert_same(r, ref, PLAIN + LUCK)
    assert np.abs(r["trial_luck"]).max() > 0
    plain = _call(env, st, tu, T, True, M, groups=GM.GROUPS, group_offset=GM.GROUP_OFFSET, lanes=64)
    _assert_same(plain, r, PLAIN)


def test_two_ply_policy(env, single, main):
    st, tu = main
    T, M = 36, 2
    ref = _singles(single, "2ply", st, tu, GM.GROUPS, GM.GROUP_OFFSET, T, True, M, lanes=64, **POLICY)
    r = _call(env, st, tu, T, True, M, groups=GM.GROUPS, group_offset=GM.GROUP_OFFSET, lanes=64, **POLICY)
    assert env.rollout_info()[3] == 1
    _assert_same(r, ref, PLAIN)


# ---- independence ----------------------------------------------------------------------------------------------------------------------

def test_call_order_splits_and_alternation(env, main):
    st, tu = main
    T, rotate, M = GM.CASES[2]
    kw = dict(groups=GM.GROUPS, group_offset=GM.GROUP_OFFSET)
    plain0 = _call(env, st, tu, T, rotate, M, position_offset=5)
    a = _call(env, st, tu, T, rotate, M, **kw)
    _assert_same(_call(env, st, tu, T, rotate, M, **kw), a, PLAIN)                     # from call to call
    _assert_same(_call(env, st, tu, T, rotate, M, position_offset=5), plain0, PLAIN)   # a plain call after grouped ones
    _assert_same(_call(env, st, tu, T, rotate, M, **kw), a, PLAIN)                     # ... and a grouped one after it
    parts = GM.split_tables()                                                          # the groups split over two calls
    got = {k: np.empty_like(a[k]) for k in PLAIN}
    for idx, groups, off in parts:
        r = _call(env, st[idx], tu[idx], T, rotate, M, groups=groups, group_offset=off)
        for k in PLAIN:
            got[k][idx] = r[k]
    _assert_same(got, a, PLAIN)


def test_no_side_effect_on_the_env(bg, W, main):
    st, tu = main
    a, twin = bg.VecGame(64, seed=5), bg.VecGame(64, seed=5)
    for e in (a, twin):
        e.load_weights(W)
        e.run_greedy(7)
    snap, dice, stats, lc = a.snapshot().clone(), a.dice().clone(), a.stats(), a.last_choice()
    prog = [x.clone() for x in a.progress()]
    a.rollout(st, tu, 36, max_plies=3, seed=SEED, groups=GM.GROUPS, group_offset=GM.GROUP_OFFSET, variance_reduction=True)
    a.rollout_paired([GM.GROUPS.index(x) for x in GM.GROUPS], "vr")
    assert torch.equal(a.snapshot(), snap) and torch.equal(a.dice(), dice)
    assert all(torch.equal(x, y) for x, y in zip(a.progress(), prog))
    assert a.stats() == stats
    lc2 = a.last_choice()
    assert all(torch.equal(lc[k], lc2[k]) for k in lc)
    a.step_greedy()
    twin.step_greedy()
    assert torch.equal(a.snapshot(), twin.snapshot())
    for e in (a, twin):
        e.close()


# ---- errors, and the largest table -------------------------------------------------------------------------------------------------------

def test_errors_and_the_last_valid_group(bg, env, single, main):
    st, tu = main
    T = 36
    top = 2 ** 31 // T - 1                               # (top + 1) T < 2^31 <= (top + 2) T
    assert (top + 1) * T < 2 ** 31 <= (top + 2) * T
    with pytest.raises(bg.BgamdError, match="-1"):
        env.rollout(st[:2], tu[:2], T, groups=[0, -1])
    with pytest.raises(bg.BgamdError, match="-1"):
        env.rollout(st[:2], tu[:2], T, groups=[top + 1, 0])
    with pytest.raises(bg.BgamdError, match="-1"):
        env.rollout(st[:2], tu[:2], T, groups=[0, 0], group_offset=-1)
    with pytest.raises(bg.BgamdError, match="-1"):          # (a rollout that failed leaves nothing to read)
        env.rollout_paired([0] * env._rollout_shape[0], "value")
    with pytest.raises(ValueError):
        env.rollout(st[:2], tu[:2], T, groups=[0, 0], position_offset=1)
    with pytest.raises(ValueError):
        env.rollout(st[:2], tu[:2], T, groups=[0])
    bad = st[:2].copy()
    bad[1, 3] = 16
    with pytest.raises(bg.BgamdError, match="-5"):
        env.rollout(bad, tu[:2], T, groups=[0, 0])
    # the last group a table may hold: ids up to 2^31 - 1 - (2^31 mod T), on the dice of the plain call at that offset
    r = _call(env, st[1:3], tu[1:3], T, True, 2, groups=[top, 0], lanes=64)
    _assert_same(r, _singles(single, "top", st[1:3], tu[1:3], [top, 0], 0, T, True, 2, lanes=64), PLAIN)
    with pytest.raises(bg.BgamdError, match="-1"):          # which = 1 needs a rollout that had the luck adjustment
        env.rollout_paired([0, 1], "vr")
    with pytest.raises(ValueError):
        env.rollout_paired([0, 1], "luck")
    with pytest.raises(ValueError):
        env.rollout_paired([0], "value")
    dm, _ = env.rollout_paired([0, 1], "value")
    assert (dm.cpu().numpy() == 0.0).all()


# ---- analysis.rollout_decisions ----------------------------------------------------------------------------------------------------------

def _decision_env(bg, W, st, tu, dice):
    e = bg.VecGame(len(st), seed=3)
    e.load_weights(W)
    e.set_states(st, tu)
    e.set_dice(dice)
    return e


def _check_lane(single, res, mover, lane, T, M, offset=0):
    """a lane's list against the plain rollout of each candidate alone at position_offset = offset + lane"""
    assert len(res) >= 1
    key = [c["mean"] for c in res]
    assert key == sorted(key, reverse=mover == 0)          # best first
    rows = [_np(single.rollout(c["state"][None], [1 - mover], T, max_plies=M, rotate=True, seed=SEED, position_offset=offset + lane,
                               per_trial=True)) for c in res]
    x = [r["trial_value"][0].astype(np.float64).tolist() for r in rows]
    for k, (c, r) in enumerate(zip(res, rows)):
        assert c["mean"] == float(r["mean"][0]) and c["stderr"] == float(r["stderr"][0]) and c["turns"] == int(r["turns"][0])
        m, se = GM.paired_fsum(x, [0] * len(x), k, 0)
        assert GM.close(c["diff"], m, T) and GM.close(c["diff_stderr"], se, T, stderr=True), (lane, k)
        # diff against the two means.  Each of the three is a wave's sum of T numbers of size <= 1 over T: at most T + 63 additions, each
        # rounding a partial sum of size <= T by at most T 2^-53, and a division -- within (T + 64) 2^-53 of exact; one more for c - best
        assert abs(c["diff"] - (c["mean"] - res[0]["mean"])) <= (3 * (T + 64) + 1) * 2.0 ** -53
        want = 0.0 if c["diff"] == 0.0 else (math.inf if c["diff_stderr"] == 0.0 else abs(c["diff"]) / c["diff_stderr"])
        assert c["jsd"] == want
        assert c["diff"] <= 0.0 if mover == 0 else c["diff"] >= 0.0
    assert res[0]["diff"] == 0.0 and res[0]["diff_stderr"] == 0.0 and res[0]["jsd"] == 0.0


def test_rollout_decisions(bg, W, single):
    from backgammon_env.analysis import rollout_decisions, rollout_moves
    gst, gtu = RC.g10_picks()
    st = np.concatenate([OR.START[None], gst[:4]]).astype(np.int32)
    tu = np.concatenate([[0], gtu[:4]]).astype(np.int32)
    dice = np.array([[3, 1], [6, 4], [5, 5], [2, 1], [6, 3]], np.int32)
    T, M, K = 36, 6, 3
    e = _decision_env(bg, W, st, tu, dice)
    before = e.snapshot().cpu().numpy()
    res = rollout_decisions(e, top_k=K, trials=T, max_plies=M, seed=SEED)
    after = e.snapshot().cpu().numpy()
    np.testing.assert_array_equal(after[:, :31], before[:, :31])           # board, side to move, dice: restored
    assert len(res) == 5 and all(1 <= len(x) <= K for x in res) and sum(len(x) for x in res) > 5
    for lane in range(5):
        _check_lane(single, res[lane], int(tu[lane]), lane, T, M)
    # lane 0 at group_offset 0 plays rollout_moves' trials: the same list, field for field
    one = bg.VecGame(1, seed=3)
    one.load_weights(W)
    want = rollout_moves(one, st[0], int(tu[0]), dice[0], top_k=K, trials=T, max_plies=M, seed=SEED)
    one.close()
    assert len(want) == len(res[0])
    for c, w in zip(res[0], want):
        assert set(c) == set(w) | {"diff", "diff_stderr", "jsd"}
        for k in w:
            assert np.array_equal(c[k], w[k]) if k == "state" else c[k] == w[k], k
    # group_offset moves every lane's dice: lane 0 at offset 1 is lane 1's dice id
    res1 = rollout_decisions(e, top_k=K, trials=T, max_plies=M, seed=SEED, group_offset=1)
    _check_lane(single, res1[0], int(tu[0]), 0, T, M, offset=1)
    e.close()


def test_rollout_decisions_pass_and_finished_lanes(bg, W, single):
    from backgammon_env.analysis import rollout_decisions
    gst, gtu = RC.g10_picks()
    bst, btu = RC.bar_position()
    fst, ftu, _, _ = OR.forced_positions()
    T, M = 36, 4
    # a lane whose mover has no move keeps no candidate
    e = _decision_env(bg, W, np.stack([bst, gst[1]]), [btu, int(gtu[1])], [[6, 5], [4, 2]])
    res = rollout_decisions(e, top_k=3, trials=T, max_plies=M, seed=SEED)
    assert res[0] == [] and len(res[1]) >= 1
    _check_lane(single, res[1], int(gtu[1]), 1, T, M)
    e.close()
    # a game that finished without auto_reset is frozen: its lane takes no part in the search and keeps no candidate
    e = _decision_env(bg, W, np.stack([gst[2], fst[0]]), [int(gtu[2]), int(ftu[0])], [[3, 2], [6, 5]])
    e.step_greedy(roll=False, auto_reset=False)
    e.set_dice([[5, 1], [5, 1]])
    before = e.snapshot().cpu().numpy()
    assert before[1, 31] & 4 and not before[0, 31] & 4
    res = rollout_decisions(e, top_k=3, trials=T, max_plies=M, seed=SEED)
    assert res[1] == [] and len(res[0]) >= 1
    _check_lane(single, res[0], int(before[0, 28]), 0, T, M)
    np.testing.assert_array_equal(e.snapshot().cpu().numpy()[:, :31], before[:, :31])
    # no lane with a candidate: nothing is rolled out
    e.set_states(np.stack([bst, bst]), [btu, btu])
    e.set_dice([[6, 5], [5, 4]])
    assert rollout_decisions(e, top_k=3, trials=T, seed=SEED) == [[], []]
    # ... but a DOUBLES roll without a move lists one empty sequence, the board itself, and the search keeps it: a one-entry list
    e.set_dice([[6, 5], [6, 6]])
    res = rollout_decisions(e, top_k=3, trials=T, max_plies=M, seed=SEED)
    assert res[0] == [] and len(res[1]) == 1
    c = res[1][0]
    assert c["seq"] == [] and (c["state"] == bst).all() and c["diff"] == 0.0 and c["jsd"] == 0.0
    _check_lane(single, res[1], btu, 1, T, M)
    e.close()
