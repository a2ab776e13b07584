"""Monte Carlo rollouts at the edges of their refill schedule on the MI355X (bgamd_env_rollout, ro_refill_kernel), trial by trial:
  (a) every horizon of rollout_cases.HORIZONS -- every run length 1..8, M = 1 with and without rotation, prime horizons, two and three
      full runs -- against a lane-by-lane replay with the greedy step, and four of them against the fp64 reference;
  (b) trial counts below, at and above the 36 ordered pairs of the rotation;
  (c) any lane count: 1, partial waves and workgroups, more lanes than trials -- plain, luck-adjusted and in points;
  (d) a fan of exactly one chunk, one entry more, one less than two, several chunks; more positions than lanes with the luck pass;
  (e) the seat loop: trials that are over before a lane plays them outnumber the lanes many times over;
  (f) nothing of one call's buffers shows in the next;
  (g) the luck and the 2-ply policy at the shortest horizons and at run length 1;
  (h) every read call answers for the last rollout call alone: plain, with luck and cube, refused, ungrouped after grouped.
The conditions these tests rest on (what the horizons cover, what the positions are, how few near ties the reference meets) are checked
on the CPU: tests/test_rollout_cases_cpu.py.  Everything is bit equality, except a truncated trial's fp32 value against fp64 (1e-5)."""
import numpy as np
import pytest

import outcome_ref as OR
import rollout_cases as RC
import test_gpu_rollout_2ply as P2
from test_gpu_rollout import _play_lanes
from test_gpu_rollout_vr import IDX, _replay as _replay_luck

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = RC.SEED
PLAIN = ("mean", "stderr", "turns", "truncated", "trial_value", "trial_turns")


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
def positions():
    return RC.positions()


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _assert_same(a, b, keys=None):
    assert set(a) == set(b)
    for k in keys or a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _rollout(env, st, tu, T, **kw):
    """env.rollout with per-trial outputs -> numpy; the env's error word stays clear (a rollout that met an error raises)"""
    r = _np(env.rollout(st, tu, T, seed=SEED, per_trial=True, **kw))
    assert env.stats()["error_flags"] == 0
    return r


def _replay(bg, W, state, turn, T, trial0, M, rotate):
    """Trials trial0 .. trial0 + T - 1 of one position on the lanes of a fresh env (_play_lanes: the greedy step itself, lane i with
    game id trial0 + i), the rule's first dice, at most M turns; a lane still running is scored by evaluate (bgamd_evaluate_slot, F32).
    -> (value [T] float32, turns [T], truncated, points [T])"""
    pts = OR.points(state)
    if pts:                                              # over: never played, its winner at 0 turns
        return np.full(T, 1.0 if pts > 0 else 0.0, np.float32), np.zeros(T, np.int64), 0, np.full(T, pts, np.int64)
    value, turns, e = _play_lanes(bg, W, state, int(turn), T, trial0, first_dice=RC.first_dice(T) if rotate else None, max_plies=M)
    running = np.isnan(value)
    if running.any():
        assert M > 0 and (turns[running] == M).all()
        value = np.where(running, e.evaluate(e.states(), e.turns()).cpu().numpy(), value)
    points = np.where(running, 0, e.outcomes().cpu().numpy()).astype(np.int64)
    assert e.stats()["error_flags"] == 0
    e.close()
    return value.astype(np.float32), turns.astype(np.int64), int(running.sum()), points


def _check_against_replay(bg, W, r, st, tu, T, offset, M, rotate, which=None):
    """the rollout's per-trial outputs of the positions `which` (all) against _replay"""
    for p in (range(len(st)) if which is None else which):
        value, turns, trunc, points = _replay(bg, W, st[p], tu[p], T, (offset + p) * T, M, rotate)
        np.testing.assert_array_equal(r["trial_value"][p], value, err_msg=f"position {p}")
        np.testing.assert_array_equal(r["trial_turns"][p], turns, err_msg=f"position {p}")
        assert int(r["truncated"][p]) == trunc, p
        if "trial_points" in r:
            np.testing.assert_array_equal(r["trial_points"][p], points, err_msg=f"position {p}")


# ---- (a) the horizon sweep -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,rotate", RC.HORIZONS)
def test_horizon_sweep(bg, W, env, positions, M, rotate):
    st, tu, kind = positions
    P, T, off = len(st), RC.SWEEP_T, RC.SWEEP_OFFSET
    r = _rollout(env, st, tu, T, max_plies=M, rotate=rotate, position_offset=off, outcomes=True)
    info = env.rollout_info()
    assert info[3] == RC.run_length(M, rotate) and info[0] == RC.default_lanes(P * T)
    _check_against_replay(bg, W, r, st, tu, T, off, M, rotate)
    over = kind == "over"
    assert (r["trial_turns"][over] == 0).all() and (r["truncated"][over] == 0).all()
    np.testing.assert_array_equal(r["trial_value"][over], np.repeat([[1.0], [0.0]], T, 1).astype(np.float32))
    np.testing.assert_array_equal(r["trial_points"][over], np.repeat([[1], [-2]], T, 1))
    assert r["truncated"][:RC.N_LIVE].sum() > 0 and (r["trial_turns"] <= M).all()

    if (M, rotate) in RC.REF_HORIZONS:                   # the fp64 reference, on the live positions
        ref = RC.sweep_reference(M, rotate)
        n = RC.N_LIVE
        tv, tt = r["trial_value"][:n], r["trial_turns"][:n]
        cmp = ~ref["near_tie"]
        print(f"horizon ({M}, {rotate}): {cmp.mean():.4f} of {cmp.size} trials compared with the fp64 reference")
        assert cmp.mean() >= 0.9
        np.testing.assert_array_equal(tt[cmp], ref["turns"][cmp])
        full, trunc = ~ref["truncated"] & cmp, ref["truncated"] & cmp
        np.testing.assert_array_equal(tv[full], ref["value"][full])
        assert trunc.sum() > 0
        np.testing.assert_allclose(tv[trunc], ref["value"][trunc], atol=1e-5, rtol=0)
        np.testing.assert_array_equal(r["truncated"][:n], ((tt == M) & (r["trial_points"][:n] == 0)).sum(1))

    if (M, rotate) == (1, True):                         # fan_val: the fan afterstate through bgamd_evaluate_slot, F32
        pairs = RC.first_dice(36)
        for p in np.nonzero(~over)[0]:
            e = bg.VecGame(36, seed=1)
            e.load_weights(W)
            e.set_states(np.tile(st[p], (36, 1)), np.full(36, tu[p]))
            e.set_dice(pairs)
            e.step_greedy(roll=False, auto_reset=False)
            fin = (e.flags().cpu().numpy() & 4) != 0
            pts = e.outcomes().cpu().numpy()
            assert (e.turns().cpu().numpy()[~fin] == 1 - tu[p]).all()          # the side now to move
            ev = e.evaluate(e.states(), e.turns(), precision=bg.F32).cpu().numpy()
            e.close()
            want = np.where(fin, (pts > 0).astype(np.float32), ev)[np.arange(T) % 36]
            np.testing.assert_array_equal(r["trial_value"][p], want, err_msg=f"position {p}")
            np.testing.assert_array_equal(r["trial_points"][p], np.where(fin, pts, 0)[np.arange(T) % 36], err_msg=f"position {p}")
            assert (r["trial_turns"][p] == 1).all()


# ---- (b) trials with rotation --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [3, 0])
@pytest.mark.parametrize("T", [1, 5, 35, 36, 37, 73])
def test_trial_counts_with_rotation(bg, W, env, positions, T, M):
    st, tu, kind = positions
    if M == 0:                                           # whole games: the late boards and the forced positions
        lst, ltu = RC.late_boards(4)
        st, tu = np.concatenate([lst, st[kind == "forced"]]), np.concatenate([ltu, tu[kind == "forced"]])
        kind = np.array(["late"] * 4 + ["forced"] * 10)
    off = 2
    r = _rollout(env, st, tu, T, max_plies=M, rotate=True, position_offset=off, outcomes=True)
    assert env.rollout_info()[0] == RC.default_lanes(len(st) * T) and env.rollout_info()[3] == RC.run_length(M, True)
    _check_against_replay(bg, W, r, st, tu, T, off, M, True)
    if M == 0:
        assert (r["truncated"] == 0).all() and (r["trial_points"] != 0).all()
    # the first dice themselves: the last forced position ends on its first turn exactly for a pair holding a 1
    f8 = int(np.nonzero(kind == "forced")[0][9])
    has1 = (RC.first_dice(T) == 1).any(1)
    np.testing.assert_array_equal(r["trial_turns"][f8] == 1, has1)
    np.testing.assert_array_equal(r["trial_points"][f8][has1], np.full(int(has1.sum()), -3))


# ---- (c) any lane count --------------------------------------------------------------------------------------------------------------------

LANES = (1, 2, 63, 65, 99, 100, 101, 255, 257, 1000)
MODES = {"plain": dict(), "luck": dict(variance_reduction=True), "points": dict(outcomes=True)}


@pytest.fixture(scope="module")
def small_set():
    """two late boards and two forced positions"""
    lst, ltu = RC.late_boards(2)
    fst, ftu, _, _ = OR.forced_positions()
    return np.concatenate([lst, fst[[2, 9]]]).astype(np.int32), np.concatenate([ltu, ftu[[2, 9]]]).astype(np.int32)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("M", [0, 5])
def test_any_lane_count(env, small_set, M, rotate, mode):
    st, tu = small_set
    T = 25
    assert len(st) * T == 100
    args = dict(max_plies=M, rotate=rotate, position_offset=1, **MODES[mode])
    base = _rollout(env, st, tu, T, **args)
    assert env.rollout_info()[0] == 256
    want_keys = set(PLAIN) | {"luck": {"vr_mean", "vr_stderr", "trial_luck"}, "points": {"counts", "equity", "equity_stderr", "trial_points"},
                              "plain": set()}[mode]
    assert set(base) == want_keys
    assert (base["truncated"].sum() > 0) == (M > 0)
    if mode == "luck":
        assert np.count_nonzero(base["trial_luck"]) > 50
    for lanes in LANES:
        r = _rollout(env, st, tu, T, lanes=lanes, **args)
        assert env.rollout_info()[0] == lanes and env.rollout_info()[3] == RC.run_length(M, rotate)
        for k in base:
            np.testing.assert_array_equal(r[k], base[k], err_msg=f"{k} at {lanes} lanes")


# ---- (d) fan chunks, and more positions than lanes ----------------------------------------------------------------------------------------------

def _cycled(positions, P):
    st, tu, _ = positions
    idx = np.arange(P) % len(st)
    return st[idx], tu[idx]


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("P,T", [(2, 32), (5, 13), (127, 1), (9, 37)])
def test_fan_chunks(bg, W, env, positions, P, T, M):
    L = 64
    n_fan = P * RC.fan_size(T)
    assert n_fan in (L, L + 1, 2 * L - 1, 36 * 9)
    st, tu = _cycled(positions, P)
    args = dict(max_plies=M, rotate=True, position_offset=4, outcomes=True)
    r = _rollout(env, st, tu, T, lanes=L, **args)
    assert env.rollout_info()[0] == L
    _assert_same(r, _rollout(env, st, tu, T, **args))
    # the positions whose fan entries end a chunk, begin the next and end the fan
    which = sorted({min(P - 1, (L - 1) // RC.fan_size(T)), min(P - 1, L // RC.fan_size(T)), P - 1, 0})
    assert len(which) >= 2
    _check_against_replay(bg, W, r, st, tu, T, 4, M, True, which)


def test_more_positions_than_lanes_with_luck(bg, W, env, positions):
    P, T, L = 70, 2, 64
    st, tu = _cycled(positions, P)
    args = dict(max_plies=2, rotate=True, variance_reduction=True, outcomes=True)
    r = _rollout(env, st, tu, T, lanes=L, **args)
    assert env.rollout_info()[0] == L and P > L
    _assert_same(r, _rollout(env, st, tu, T, **args))
    assert env.rollout_info()[0] == 256
    d = RC.first_dice(T)
    for p in (0, 19, 65, 69):                            # the start and the bar position, and two positions past the lane count
        value, luck = _replay_luck(bg, W, st[p], int(tu[p]), T, p * T, d, 2)
        np.testing.assert_array_equal(r["trial_value"][p], value.astype(np.float32), err_msg=f"position {p}")
        np.testing.assert_array_equal(r["trial_luck"][p], luck, err_msg=f"position {p}")
    assert np.count_nonzero(r["trial_luck"]) > P


# ---- (e) the seat loop ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rotate", [True, False])
@pytest.mark.parametrize("M", [0, 1])
def test_seat_loop(bg, W, env, M, rotate):
    st, tu, kind = RC.skip_heavy()
    P, T, L = len(st), 200, 64
    args = dict(max_plies=M, rotate=rotate, outcomes=True)
    r = _rollout(env, st, tu, T, lanes=L, **args)
    assert env.rollout_info()[0] == L and env.rollout_info()[3] == RC.run_length(M, rotate)
    _assert_same(r, _rollout(env, st, tu, T, **args))
    assert env.rollout_info()[0] == RC.default_lanes(P * T) == 8192
    known = (kind == "over") | (kind == "forced")
    assert known.sum() * T >= 90 * L                     # trials that are over before a lane plays them: ~94 per lane
    for p in np.nonzero(known)[0]:
        value, turns, points = RC.known_result(st[p], kind[p])
        assert (r["trial_value"][p] == np.float32(value)).all() and (r["trial_turns"][p] == turns).all(), p
        assert (r["trial_points"][p] == points).all() and r["truncated"][p] == 0, p
        want = np.zeros(6, np.int64)
        want[(points - 1) if points > 0 else (2 - points)] = T
        np.testing.assert_array_equal(r["counts"][p], want)
        assert r["equity"][p] == float(points) and r["mean"][p] == value and r["turns"][p] == turns * T
    _check_against_replay(bg, W, r, st, tu, T, 0, M, rotate, np.nonzero(~known)[0])
    live = r["trial_turns"][kind == "late"]
    assert (live >= max(M, 1)).all() and ((live > 2).any() if M == 0 else (live == 1).all())


# ---- (f) stale state -----------------------------------------------------------------------------------------------------------------------

def test_nothing_stale_between_calls(bg, W, positions):
    st, tu, kind = positions
    sel = [0, 3, 5, 8, 16, 17, 18, 19]                   # live, forced, over, bar
    a_st, a_tu = st[sel], tu[sel]
    lst, ltu = RC.late_boards(3)

    def call_a(e):
        r = _rollout(e, a_st, a_tu, 72, max_plies=1, rotate=True, variance_reduction=True, outcomes=True)
        return r, e.rollout_info()

    e = bg.VecGame(64, seed=7)
    e.load_weights(W)
    a1, ia = call_a(e)
    assert set(a1) == set(PLAIN) | {"vr_mean", "vr_stderr", "trial_luck", "counts", "equity", "equity_stderr", "trial_points"}
    b = _rollout(e, lst, ltu, 5, max_plies=0, rotate=False)
    assert (b["truncated"] == 0).all() and e.rollout_info()[3] == 8
    c = _rollout(e, st[[1, 9, 17]], tu[[1, 9, 17]], 36, max_plies=2, rotate=True, plies=2, top_k=3, margin=0.04)
    assert e.rollout_info()[3] == 1 and c["truncated"][2] == 0 and (c["trial_turns"][1] == 1).all()
    a2, ia2 = call_a(e)
    e.close()
    _assert_same(a1, a2)
    assert ia == ia2 and ia[3] == 1
    f = bg.VecGame(64, seed=7)
    f.load_weights(W)
    a3, ia3 = call_a(f)
    f.close()
    _assert_same(a1, a3)
    assert ia == ia3
    assert np.count_nonzero(a1["trial_luck"]) > 72 and (a1["trial_turns"][:4] == 1).all()


# ---- (g) luck and two plies at the edges -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,rotate", [(1, True), (2, True), (11, False)])
def test_luck_at_the_edges(bg, W, env, positions, M, rotate):
    st, tu, kind = positions
    sel = [0, 4, 19]                                     # the start position, a fixture board, the bar position
    st, tu = st[sel], tu[sel]
    P, T, off = 3, 37, 5
    r = _rollout(env, st, tu, T, max_plies=M, rotate=rotate, position_offset=off, variance_reduction=True)
    assert env.rollout_info()[3] == RC.run_length(M, rotate) == 1
    d = RC.first_dice(T)
    for p in range(P):
        value, luck = _replay_luck(bg, W, st[p], int(tu[p]), T, (off + p) * T, d if rotate else None, M)
        np.testing.assert_array_equal(r["trial_value"][p], value.astype(np.float32), err_msg=f"position {p}")
        np.testing.assert_array_equal(r["trial_luck"][p], luck, err_msg=f"position {p}")
    assert np.count_nonzero(r["trial_luck"][:2]) > T
    if (M, rotate) == (1, True):                         # turn 0's luck alone: the position's own pre-roll evaluation
        f, m = (x.cpu().numpy() for x in env.evaluate_preroll(st, tu))
        want = f[:, IDX[d[:, 0], d[:, 1]]].astype(np.float64) - m[:, None]
        np.testing.assert_array_equal(r["trial_luck"], want)


@pytest.mark.parametrize("lanes", [1, 65])
@pytest.mark.parametrize("T", [5, 37])
@pytest.mark.parametrize("M,rotate", [(1, True), (3, False)])
def test_two_plies_at_the_edges(bg, W, env, positions, monkeypatch, M, rotate, T, lanes):
    st, tu, kind = positions
    lst, ltu = RC.late_boards(1)
    sel = [0, 2, 9, 17]                                  # the start position, a fixture board, a forced position, a board that is over
    st, tu = np.concatenate([st[sel], lst]), np.concatenate([tu[sel], ltu])
    monkeypatch.setattr(P2, "TOP_K", 3)                  # the replay of test_gpu_rollout_2ply.py plays with its module's policy
    assert P2.MARGIN == 0.04
    off = 1
    r = _rollout(env, st, tu, T, max_plies=M, rotate=rotate, position_offset=off, lanes=lanes, outcomes=True, plies=2, top_k=3, margin=0.04)
    assert env.rollout_info()[3] == 1 and env.rollout_info()[0] == lanes
    value, turns, points, _, trunc = P2._replay(bg, W, st, tu, T, off, rotate, M)
    np.testing.assert_array_equal(r["trial_value"], value)
    np.testing.assert_array_equal(r["trial_turns"], turns)
    np.testing.assert_array_equal(r["trial_points"], points)
    np.testing.assert_array_equal(r["truncated"], trunc)
    assert trunc[0] == T and (turns[3] == 0).all()


# ---- (h) the read calls follow the last call ---------------------------------------------------------------------------------------------------

def test_reads_follow_the_last_call(bg, W, positions):
    """One env, four calls in sequence: what each read call returns or refuses is decided by the LAST rollout call alone -- a plain one,
    a luck-adjusted one with the cube, one refused for a bad state (every read refuses; the two info calls keep the numbers of the last
    call that succeeded), and an ungrouped call after a grouped one (no trace of the group table)."""
    from backgammon_env import _capi
    st, tu, _ = positions
    st, tu = st[:3], tu[:3]
    T, ref = 40, [1, 1, 0]
    args = dict(max_plies=3, lanes=256, seed=SEED)

    def vr_read(e):
        _capi.check(e._lib.bgamd_env_rollout_vr_read(e._h, None, None, None, None), "rollout_vr_read")

    def refuses(call):
        with pytest.raises(bg.BgamdError, match="-1"):
            call()

    e = bg.VecGame(64, seed=7)
    e.load_weights(W)
    # 1. a plain call
    e.rollout(st, tu, T, **args)
    assert e.rollout_outcomes_read()["counts"].shape == (3, 6)
    e.rollout_paired(ref, "value")
    e.rollout_paired(ref, "equity")
    for call in (lambda: vr_read(e), e.rollout_cube_read, lambda: e.rollout_paired(ref, "cubeful"), lambda: e.rollout_paired(ref, "vr")):
        refuses(call)
    # 2. luck-adjusted, the cube on: every read works
    e.rollout(st, tu, T, variance_reduction=True, cube=bg.Cube(), **args)
    vr_read(e)
    assert e.rollout_cube_read()["cubeful"].shape == (3,) and e.rollout_outcomes_read(per_trial=True)["trial_points"].shape == (3, T)
    for which in ("value", "vr", "equity", "cubeful"):
        e.rollout_paired(ref, which)
    info, cube_info = e.rollout_info(), e.rollout_cube_info()
    assert info[0] == 256 and info[3] == RC.run_length(3, True) and info[1] > 0 and info[2] > 0 and cube_info[0] > 0
    # 3. a call refused for a bad state (one checker too many): nothing to read, the infos as they were
    bad = st.copy()
    bad[1, 3] = 16
    with pytest.raises(bg.BgamdError, match="-5"):
        e.rollout(bad, tu, T, variance_reduction=True, cube=bg.Cube(), **args)
    for call in (lambda: vr_read(e), e.rollout_cube_read, e.rollout_outcomes_read, *(lambda w=w: e.rollout_paired(ref, w) for w in e.PAIRED_WHICH)):
        refuses(call)
    assert e.rollout_info() == info and e.rollout_cube_info() == cube_info
    # 4. grouped, then ungrouped with the same positions: the paired read pairs what a fresh env pairs
    e.rollout(st, tu, T, variance_reduction=True, groups=[0, 0, 1], **args)
    grouped = _np(dict(zip("ms", e.rollout_paired(ref, "vr"))))
    assert np.isfinite(grouped["m"][:2]).all() and np.isnan(grouped["m"][2])                # positions 0 and 1 share dice, 2 and 0 do not
    e.rollout(st, tu, T, variance_reduction=True, **args)
    after = {w: _np(dict(zip("ms", e.rollout_paired(ref, w)))) for w in ("value", "vr", "equity")}
    assert e.stats()["error_flags"] == 0
    e.close()
    f = bg.VecGame(64, seed=7)
    f.load_weights(W)
    f.rollout(st, tu, T, variance_reduction=True, **args)
    for w in after:
        fresh = _np(dict(zip("ms", f.rollout_paired(ref, w))))
        for k in "ms":
            np.testing.assert_array_equal(after[w][k].view(np.int64), fresh[k].view(np.int64), err_msg=w + k)
        assert np.isnan(after[w]["m"][[0, 2]]).all() and after[w]["m"][1] == 0              # ungrouped: a position pairs with itself only
    f.close()
