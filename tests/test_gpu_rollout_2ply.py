"""Rollouts played by the filtered 2-ply search on the MI355X (bgamd_env_rollout_policy, VecGame.rollout(plies=2)):
  (5) every trial bit for bit against a lane-by-lane replay with step_search(margin=...) -- value, turns and points; a contact position,
      a bear-off that ends inside the turn limit and a position that is already over; rotated and not, cut at 4 turns and played out;
  (6) the same results for any lane count, from call to call and over a position_offset split; one turn per run;
  (7) plies = 1 set explicitly is the env that never called the setter, bit for bit;
  (8) luck-adjusted: the plain outputs unchanged, trial_luck against the replay's evaluate_preroll lucks, the six counts;
  (9) error codes, weight slot 1, rollout_moves(plies=2)."""
import numpy as np
import pytest

import nets as N
from test_gpu_rollout import SEED, _greedy_positions
from test_gpu_rollout_vr import IDX, VR, _assert_same, _np

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOP_K, MARGIN, LANES = 2, 0.04, 256
POLICY = dict(plies=2, top_k=TOP_K, margin=MARGIN)


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


@pytest.fixture(scope="module")
def env(bg, weights):
    e = bg.VecGame(64, seed=7)
    e.load_weights(weights)
    yield e
    e.close()


@pytest.fixture(scope="module")
def positions(bg, weights):
    """a contact position, a bear-off that ends within four turns, a position that is already over"""
    st, tu = _greedy_positions(bg, weights, 12, 11)
    contact = st[11]
    assert (contact[:24] > 0).any() and np.where(contact[:24] > 0)[0].min() < np.where(contact[:24] < 0)[0].max()
    b_st, b_tu = N._bearoffs()
    over = np.zeros(28, np.int32)
    over[27] = 15; over[19:24] = 3
    return (np.stack([contact, b_st[2], over]).astype(np.int32), np.array([tu[11], b_tu[2], 0], np.int32))


def _replay_position(bg, weights, state, turn, T, lane_offset, rotate, max_plies, luck):
    """T lanes with the rollout's seed: lane i plays game id lane_offset + i, so step_search(roll=True, auto_reset=False) draws the
    trial's dice.  -> value [T] float32, turns [T], points [T], luck [T] float64, truncated"""
    if state[26] == 15 or state[27] == 15:                 # already over: never played, its winner at 0 turns
        pts = int(bg.outcomes(state[None]).cpu().numpy()[0])
        return (np.full(T, 1.0 if state[26] == 15 else 0.0, np.float32), np.zeros(T, np.int64), np.full(T, pts, np.int64), np.zeros(T), 0)
    e = bg.VecGame(T, seed=SEED, lane_offset=lane_offset)
    e.load_weights(weights)
    e.set_states(np.tile(state, (T, 1)), np.full(T, turn))
    turns = np.zeros(T, np.int64)
    lk = np.zeros(T)
    ar = np.arange(T)
    first = np.stack([1 + (ar % 36) // 6, 1 + (ar % 36) % 6], 1).astype(np.int32)
    k = 0
    while max_plies == 0 or k < max_plies:
        live = (e.flags().cpu().numpy() & 4) == 0
        if not live.any():
            break
        if luck:
            f, m = (x.cpu().numpy() for x in e.evaluate_preroll(e.states(), e.turns()))
        if k == 0 and rotate:
            e.set_dice(first)
            e.step_search(top_k=TOP_K, roll=False, auto_reset=False, margin=MARGIN)
        else:
            e.step_search(top_k=TOP_K, roll=True, auto_reset=False, margin=MARGIN)
        if luck:
            d = e.dice().cpu().numpy()
            lk[live] += (f[ar, IDX[d[:, 0], d[:, 1]]].astype(np.float64) - m)[live]
        turns[live] += 1
        k += 1
    fl = e.flags().cpu().numpy()
    frozen = (fl & 4) != 0
    value = np.where(frozen, np.where((fl >> 1) & 1, 0.0, 1.0), np.nan)
    if (~frozen).any():
        value = np.where(frozen, value, e.evaluate(e.states(), e.turns()).cpu().numpy())
    points = np.where(frozen, e.outcomes().cpu().numpy(), 0).astype(np.int64)
    assert e.stats()["error_flags"] == 0
    e.close()
    return value.astype(np.float32), turns, points, lk, int((~frozen).sum())


def _replay(bg, weights, st, tu, T, offset, rotate, max_plies, luck=False):
    """-> value [P, T], turns [P, T], points [P, T], luck [P, T], truncated [P] of the trials with ids (offset + p) T + i"""
    per = [_replay_position(bg, weights, st[p], int(tu[p]), T, (offset + p) * T, rotate, max_plies, luck) for p in range(len(st))]
    return tuple(np.stack([x[q] for x in per]) for q in range(5))


# ---- (5) trial for trial ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rotate,T", [(True, 36), (False, 40)])
def test_trials_against_a_lane_by_lane_replay(bg, weights, env, positions, rotate, T):
    st, tu = positions
    off = 3
    r = _np(env.rollout(st, tu, T, max_plies=4, rotate=rotate, seed=SEED, position_offset=off, lanes=LANES, per_trial=True,
                        outcomes=True, **POLICY))
    assert env.rollout_info()[3] == 1
    value, turns, points, _, trunc = _replay(bg, weights, st, tu, T, off, rotate, 4)
    np.testing.assert_array_equal(r["trial_value"], value)
    np.testing.assert_array_equal(r["trial_turns"], turns)
    np.testing.assert_array_equal(r["trial_points"], points)
    np.testing.assert_array_equal(r["truncated"], trunc)
    assert trunc[0] == T and trunc[1] == 0 and (turns[1] >= 1).all() and (turns[2] == 0).all() and (r["trial_value"][2] == 0.0).all()
    # the bear-off position played to its end
    r = _np(env.rollout(st[1:2], tu[1:2], T, max_plies=0, rotate=rotate, seed=SEED, position_offset=off + 1, lanes=LANES, per_trial=True,
                        outcomes=True, **POLICY))
    value, turns, points, _, trunc = _replay(bg, weights, st[1:2], tu[1:2], T, off + 1, rotate, 0)
    np.testing.assert_array_equal(r["trial_value"], value)
    np.testing.assert_array_equal(r["trial_turns"], turns)
    np.testing.assert_array_equal(r["trial_points"], points)
    assert trunc[0] == 0 and (points != 0).all()


def test_the_policy_is_not_the_greedy_one(env, positions):
    """... on the contact position some trial must take another course than under the greedy step (same dice), or nothing above was tested"""
    st, tu = positions
    args = dict(max_plies=4, rotate=True, seed=SEED, lanes=LANES, per_trial=True)
    a = _np(env.rollout(st[:1], tu[:1], 72, **args))
    b = _np(env.rollout(st[:1], tu[:1], 72, **args, **POLICY))
    assert not np.array_equal(a["trial_value"], b["trial_value"])


# ---- (6) independence -----------------------------------------------------------------------------------------------------------------------

def test_independence_of_lanes_calls_and_offsets(env, positions):
    st, tu = positions
    st, tu = np.concatenate([st, st[:1]]), np.concatenate([tu, tu[:1]])
    P, T = 4, 144
    args = dict(max_plies=5, rotate=True, seed=SEED, per_trial=True, outcomes=True, **POLICY)
    base = _np(env.rollout(st, tu, T, **args))
    assert env.rollout_info()[0] == 768 and env.rollout_info()[3] == 1
    for lanes in (256, 512):
        _assert_same(base, _np(env.rollout(st, tu, T, lanes=lanes, **args)))
        assert env.rollout_info()[0] == lanes and env.rollout_info()[3] == 1
    _assert_same(base, _np(env.rollout(st, tu, T, **args)))
    a = _np(env.rollout(st[:P // 2], tu[:P // 2], T, position_offset=0, **args))
    b = _np(env.rollout(st[P // 2:], tu[P // 2:], T, position_offset=P // 2, **args))
    _assert_same(base, {k: np.concatenate([a[k], b[k]]) for k in base})
    assert not np.array_equal(base["trial_value"][0], base["trial_value"][3])      # the same position under other trial ids: other dice


# ---- (7) plies = 1 is untouched -------------------------------------------------------------------------------------------------------------

def test_one_ply_policy_is_the_default(bg, weights, positions):
    from backgammon_env import _capi
    st, tu = positions
    args = dict(max_plies=9, rotate=True, seed=SEED, per_trial=True, variance_reduction=True, outcomes=True)
    out = []
    for setter in (False, True):
        e = bg.VecGame(64, seed=7)
        e.load_weights(weights)
        if setter:
            e.rollout(st, tu, 36, max_plies=2, seed=SEED, **POLICY)        # a 2-ply rollout first: rollout() puts plies = 1 back
            _capi.check(e._lib.bgamd_env_rollout_policy(e._h, 1, 5, 0.25), "rollout_policy")
        out.append((_np(e.rollout(st, tu, 72, **args)), e.rollout_info()))
        e.close()
    _assert_same(out[0][0], out[1][0])
    assert out[0][1] == out[1][1] and out[0][1][3] > 1


# ---- (8) luck adjustment and outcomes -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rotate,T", [(True, 36), (False, 40)])
def test_luck_and_outcomes_at_two_plies(bg, weights, env, positions, rotate, T):
    st, tu = positions
    args = dict(max_plies=4, rotate=rotate, seed=SEED, position_offset=2, lanes=LANES, per_trial=True, outcomes=True, **POLICY)
    a = _np(env.rollout(st, tu, T, **args))
    ia = env.rollout_info()
    b = _np(env.rollout(st, tu, T, variance_reduction=True, **args))
    assert env.rollout_info() == ia
    _assert_same(a, b, [k for k in a])
    assert set(b) == set(a) | set(VR)
    value, _, _, luck, trunc = _replay(bg, weights, st, tu, T, 2, rotate, 4, luck=True)
    np.testing.assert_array_equal(b["trial_value"], value)
    np.testing.assert_array_equal(b["trial_luck"], luck)
    assert np.count_nonzero(luck[0]) > T // 2 and not luck[2].any()
    np.testing.assert_array_equal(b["counts"].sum(1), T - b["truncated"])
    np.testing.assert_array_equal(b["truncated"], trunc)


# ---- (9) plumbing ---------------------------------------------------------------------------------------------------------------------------

def test_policy_errors(bg, weights, positions):
    st, tu = positions
    e = bg.VecGame(64, seed=1)
    lib = e._lib
    assert lib.bgamd_env_rollout_policy(None, 1, 0, 0.0) == -1
    for plies, k, mg in ((0, 2, 0.1), (3, 2, 0.1), (2, -1, 0.1), (2, 2, -0.1), (2, 2, float("nan")), (1, -1, 0.0)):
        assert lib.bgamd_env_rollout_policy(e._h, plies, k, mg) == -1, (plies, k, mg)
    assert lib.bgamd_env_rollout_policy(e._h, 2, 0, float("inf")) == 0 and lib.bgamd_env_rollout_policy(e._h, 1, 0, 0.0) == 0
    with pytest.raises(bg.BgamdError, match="-6"):
        e.rollout(st, tu, 8, **POLICY)                     # no weights
    e.load_weights(weights)
    with pytest.raises(bg.BgamdError, match="-1"):
        e.rollout(st, tu, 8, plies=3)
    bad = st.copy()
    bad[0, 3] = 16
    with pytest.raises(bg.BgamdError, match="-5"):
        e.rollout(bad, tu, 8, **POLICY)
    r = _np(e.rollout(st, tu, 8, max_plies=2, seed=SEED, per_trial=True))       # ... and the env plays one ply again after each
    f = bg.VecGame(64, seed=1)
    f.load_weights(weights)
    _assert_same(r, _np(f.rollout(st, tu, 8, max_plies=2, seed=SEED, per_trial=True)))
    e.close()
    f.close()


def test_weight_slot_1(bg, weights, positions):
    st, tu = positions
    a = bg.VecGame(64, seed=2)
    a.load_weights(N.table("normal"), slot=0)
    a.load_weights(weights, slot=1)
    b = bg.VecGame(64, seed=2)
    b.load_weights(weights)
    args = dict(max_plies=3, rotate=True, seed=SEED, per_trial=True, **POLICY)
    ra, rb = _np(a.rollout(st, tu, 36, slot=1, **args)), _np(b.rollout(st, tu, 36, **args))
    _assert_same(ra, rb)
    assert not np.array_equal(_np(a.rollout(st, tu, 36, **args))["trial_value"], ra["trial_value"])
    a.close()
    b.close()


def test_rollout_moves_at_two_plies(bg, weights, positions):
    from backgammon_env.analysis import rollout_moves
    st, tu = positions
    one = bg.VecGame(1, seed=3)
    one.load_weights(weights)
    ref = bg.VecGame(1, seed=3)
    ref.load_weights(weights)
    res = rollout_moves(one, st[0], int(tu[0]), (3, 1), top_k=3, trials=36, max_plies=3, seed=SEED, plies=2, rollout_top_k=TOP_K,
                        rollout_margin=MARGIN)
    assert 2 <= len(res) <= 3
    for c in res:
        d = ref.rollout(c["state"][None], [1 - int(tu[0])], 36, max_plies=3, rotate=True, seed=SEED, **POLICY)
        assert c["mean"] == float(d["mean"][0]) and c["stderr"] == float(d["stderr"][0]) and c["turns"] == int(d["turns"][0])
    means = [c["mean"] for c in res]
    assert means == sorted(means, reverse=int(tu[0]) == 0)
    one.close()
    ref.close()
