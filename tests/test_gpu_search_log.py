"""The search log on the MI355X (bgamd_env_set_search_log: csrc/bg_search_log.h and the host code around it), lane by lane and bit for
bit:
  (1) one step, every field, every lane -- plain and filtered steps, five lane counts, the checkpoint and the dyadic table -- against the
      env's own boards, search_candidates, last_choice and search_info, and against the exact model tests/search_log_model.py;
  (2) the target is a function of the logged position: v2_from_replies of evaluate_preroll's roll values of `after`, bit for bit;
  (3) a played round against the same games stepped one search step at a time without a log;
  (4) truncation at max_plies with guard rows behind the buffers;
  (5) BGAMD_ONLY_P1/P2 and BGAMD_NO_FLIP;
  (6) the learner takes it: replay_rows, fit_search, fit_rows against fit;
  (7) error codes and the log's life cycle;
  (8) examples/search_fit.py at tiny size.
tests/test_search_log_model_cpu.py holds the conditions these rest on (the model, the lane classes among the first 63 boards)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import search_lanes as L
import search_log_model as G
import search_model as M
from test_gpu_search_rules import _indices, _np, _table, _u32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INF = float("inf")
NS = (1, 63, 64, 257, 1000)            # a partial wave, exactly one wave, one workgroup + 1, several workgroups
# (top_k, margin): the plain step at top_k 1, 3, 0; the filtered step at top_k 3 with the margins 0, 0.02, +inf
STEPS = [(1, None), (3, None), (0, None), (3, 0.0), (3, 0.02), (3, INF)]
SENT_I, SENT_F = 0x5A5A5A5A, 123.0
QNAN = G.QNAN


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


def _fill(log):
    rows, after, target, v1 = log
    rows.fill_(SENT_I); after.fill_(SENT_I); target.fill_(SENT_F); v1.fill_(SENT_F)


def _log_np(log):
    rows, after, target, v1 = log
    return dict(rows=_np(rows).view(np.uint32), after=_np(after).view(np.uint32), target=_u32(_np(target)), v1=_u32(_np(v1)))


def _untouched(lg, where):
    """the sentinel fill stands in all four buffers at the [ply, lane] places `where` (a bool mask or an index tuple)"""
    return ((lg["rows"][where] == SENT_I).all() and (lg["after"][where] == SENT_I).all()
            and (lg["target"][where] == _u32(np.float32(SENT_F))).all() and (lg["v1"][where] == _u32(np.float32(SENT_F))).all())


def _rows(bg, st, tu):
    return _np(bg.pack_rows(st, tu)).view(np.uint32)


def _logged_step(bg, env, st, tu, dice, top_k, margin, T=3, **flags):
    """every lane back to ply 0 on the given boards and dice, a sentinel-filled log of T plies, one search step (no roll, no restart)
    -> the step's results and the log as numpy; the log stays set (the caller drops it)"""
    env.reset()
    env.set_states(st, tu)
    env.set_dice(dice)
    log = env.record_search_log(T)
    _fill(log)
    env.step_search(top_k=top_k, roll=False, auto_reset=False, margin=margin, **flags)
    out = dict(zip(("states", "v1", "v2", "kept"), (_np(x) for x in env.search_candidates())))
    out["value"] = _np(env.last_choice()["value"])
    out["post"], out["turns"], out["flags"] = _np(env.states()), _np(env.turns()), _np(env.flags())
    out["info"] = env.search_info()
    out["log"] = _log_np(log)
    out["log_t"] = log
    assert env.stats()["error_flags"] == 0
    return out


def _played(run, i):
    """the place in lane i's kept list of the candidate that was played: the one the lane's board now shows (the kept states differ)"""
    k = int(run["kept"][i])
    hit = [j for j in range(k) if np.array_equal(run["states"][i, j], run["post"][i])]
    assert len(hit) == 1, (i, k, hit)
    return hit[0]


# ---- (1) one step, every field, every lane -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("net", ["ckpt", "dyadic"])
def test_one_step_every_field_every_lane(bg, weights, net, n):
    st, tu, dice = (x[:n] for x in L.g10())
    env = bg.VecGame(n)
    env.load_weights(_table(net, weights))
    nan_seen = term_seen = 0
    for top_k, margin in STEPS:
        filtered = margin is not None
        run = _logged_step(bg, env, st, tu, dice, top_k, margin)
        lg = run["log"]
        what = (net, n, top_k, margin)
        assert np.array_equal(lg["rows"][0], _rows(bg, st, tu)), what
        assert np.array_equal(lg["after"][0], _rows(bg, run["post"], 1 - tu)), what     # a finished, frozen lane keeps its final board
        assert _untouched(lg, (slice(1, None),)), what
        want_t, want_v = np.full(n, QNAN, np.uint32), np.full(n, QNAN, np.uint32)
        for i in range(n):
            k = int(run["kept"][i])
            if k == 0:
                assert np.array_equal(run["post"][i], st[i]), (what, i)
                continue
            j = _played(run, i)
            want_v[i] = _u32(run["v1"][i, j:j + 1])[0]
            if k >= (2 if filtered else 1):
                want_t[i] = _u32(run["v2"][i, j:j + 1])[0]
                assert want_t[i] == _u32(run["value"][i:i + 1])[0], (what, i)
            # ... and the exact model, fed with the device's own values
            idx = _indices(run, i)
            e = G.entry(st[i], tu[i], True, idx, run["states"][i, :k], _u32(run["v1"][i, :k]), _u32(run["v2"][i, :k]),
                        L.terminal(run["states"][i, :k], tu[i]), filtered)
            got = dict(rows=lg["rows"][0, i], after=lg["after"][0, i], target=lg["target"][0, i], v1=lg["v1"][0, i])
            assert G.same(e, got), (what, i)
            term_seen += bool(L.terminal(run["states"][i, j:j + 1], tu[i])[0])
        assert np.array_equal(lg["target"][0], want_t) and np.array_equal(lg["v1"][0], want_v), what
        # the NaN sets by the step's own counts: lanes with a move have a v1, searched lanes a target
        assert int((lg["v1"][0] != QNAN).sum()) == run["info"][0] == int((run["kept"] >= 1).sum()), what
        assert int((lg["target"][0] != QNAN).sum()) == run["info"][1], what
        nan_seen += int((lg["target"][0] == QNAN).sum())
        # a second step (rolled dice): the lanes the first one finished are frozen, take no part and write nothing; the others log ply 1
        fin = (run["flags"] & 4) != 0
        pre2, tu2 = run["post"], run["turns"]
        env.step_search(top_k=top_k, roll=True, auto_reset=False, margin=margin)
        lg2 = _log_np(run["log_t"])
        assert _untouched(lg2, (1, fin)) and _untouched(lg2, (slice(2, None),)), what
        assert np.array_equal(lg2["rows"][1, ~fin], _rows(bg, pre2, tu2)[~fin]), what
        assert np.array_equal(lg2["after"][1, ~fin], _rows(bg, _np(env.states()), 1 - tu2)[~fin]), what
        assert all(np.array_equal(lg2[f][0], lg[f][0]) for f in lg), what
        if n >= 63:
            assert fin.any() and not fin.all(), what
        env.record_search_log(None)
    if n >= 63:
        assert nan_seen and term_seen                      # lanes without a move, singletons, played terminal candidates
    env.close()


# ---- (2) the target is a function of the logged position ----------------------------------------------------------------------------------

@pytest.mark.parametrize("net", ["ckpt", "dyadic"])
def test_target_is_a_function_of_the_logged_position(bg, weights, net):
    n = 1000
    st, tu, dice = (x[:n] for x in L.g10())
    env = bg.VecGame(n)
    env.load_weights(_table(net, weights))
    for top_k, margin in ((3, None), (3, 0.02)):
        run = _logged_step(bg, env, st, tu, dice, top_k, margin, no_flip=True)
        env.record_search_log(None)
        post, target = run["post"], run["log"]["target"][0]
        searched = target != QNAN
        term = post[np.arange(n), 26 + tu] == 15
        print("searched entries %s top_k %d margin %r: %d terminal, %d others" % (net, top_k, margin, (searched & term).sum(), (searched & ~term).sum()))
        if margin is None:                                  # (the plain step searches every lane with a move: 1 000 boards hold both kinds)
            assert (searched & term).sum() >= 20 and (searched & ~term).sum() >= 800
        outcome = _u32(np.where(tu == 0, 1.0, 0.0).astype(np.float32))
        assert np.array_equal(target[searched & term], outcome[searched & term])
        # a board that was handed in with the OTHER side already home is no terminal candidate for the search, but evaluate_preroll scores
        # it by its outcome (tests/test_gpu_search_rules.py, the same comparison): no such position arises in play; left out
        cmp = searched & ~term & (post[np.arange(n), 27 - tu] != 15)
        assert cmp.sum() >= (700 if margin is None else 50)
        f, _ = (_np(x) for x in env.evaluate_preroll(post[cmp], 1 - tu[cmp]))
        want = _u32(M.v2_from_replies(f))
        bad = np.where(target[cmp] != want)[0]
        assert len(bad) == 0, (net, top_k, margin, len(bad), np.where(cmp)[0][bad][:8].tolist())
    env.close()


# ---- (3) a played round -------------------------------------------------------------------------------------------------------------------

ROUND = dict(n=257, max_plies=512, top_k=3, margin=0.04, seed=11)


@pytest.fixture(scope="module")
def played_round(bg, weights):
    from backgammon_env.learner import play_round_search
    env = bg.VecGame(ROUND["n"], seed=ROUND["seed"])
    env.load_weights(weights)
    out = play_round_search(env, max_plies=ROUND["max_plies"], top_k=ROUND["top_k"], margin=ROUND["margin"], episode=0)
    final = (env.states().clone(), env.turns().clone(), env.flags().clone())
    assert env.stats()["error_flags"] == 0
    env.close()
    return out, final


def test_a_played_round(bg, weights, played_round):
    (rows, lengths, p1_won, after, target, v1), (fin_st, fin_tu, fin_fl) = played_round
    n, T = ROUND["n"], int(rows.shape[0])
    assert rows.shape == after.shape == (T, n, 8) and target.shape == v1.shape == (T, n)
    assert int((lengths > 0).sum()) == n and int(lengths.max()) == T > 60         # every game ended inside the log
    env = bg.VecGame(n, seed=ROUND["seed"])
    env.load_weights(weights)
    env.reset(episode=0)
    hand_rows, hand_after = torch.zeros_like(rows), torch.zeros_like(after)
    live_at = torch.zeros((T, n), dtype=torch.bool, device=rows.device)
    for t in range(T):
        pre, mover, live = env.states(), env.turns(), (env.flags() & 4) == 0
        env.step_search(top_k=ROUND["top_k"], auto_reset=False, margin=ROUND["margin"])
        hand_rows[t], hand_after[t], live_at[t] = bg.pack_rows(pre, mover), bg.pack_rows(env.states(), 1 - mover), live
    done = (env.flags() & 4) != 0
    ply, _ = env.progress()
    assert bool(done.all()) and torch.equal(ply + 1, lengths)
    assert torch.equal(((env.flags() >> 1) & 1) == 0, p1_won)
    inside = torch.arange(T, device=rows.device)[:, None] < lengths[None, :]
    assert torch.equal(inside, live_at)
    assert torch.equal(rows[inside], hand_rows[inside]) and torch.equal(after[inside], hand_after[inside])
    # the log has no side effect on the game: the boards both envs end on, bit for bit
    assert torch.equal(env.states(), fin_st) and torch.equal(env.turns(), fin_tu) and torch.equal(env.flags(), fin_fl)
    # slots past a lane's length are untouched: zeros and NaN, as record_search_log made them
    assert not rows[~inside].any() and not after[~inside].any()
    assert bool(torch.isnan(target[~inside]).all()) and bool(torch.isnan(v1[~inside]).all())
    assert bool(torch.isfinite(target[inside]).any()) and bool(torch.isnan(target[inside]).any())    # searched turns and singletons
    env.close()


# ---- (4) truncation -----------------------------------------------------------------------------------------------------------------------

def test_truncation_leaves_the_guard_rows(bg, weights):
    n, T, guard = 64, 3, 2
    env = bg.VecGame(n, seed=3)
    env.load_weights(weights)
    dev = env.device
    log = (torch.empty((T + guard, n, 8), dtype=torch.int32, device=dev), torch.empty((T + guard, n, 8), dtype=torch.int32, device=dev),
           torch.empty((T + guard, n), dtype=torch.float32, device=dev), torch.empty((T + guard, n), dtype=torch.float32, device=dev))
    _fill(log)
    p = [ctypes.c_void_p(t.data_ptr()) for t in log]
    assert env._lib.bgamd_env_set_search_log(env._h, p[0], p[1], p[2], p[3], T) == 0
    for _ in range(T + 3):                                  # plies 0 .. T + 2: the last three are dropped
        env.step_search(top_k=2, auto_reset=False, margin=0.04)
    assert bool((env.progress()[0] == T + 3).all())
    lg = _log_np(log)
    assert (lg["rows"][:T] != SENT_I).any(-1).all() and (lg["after"][:T] != SENT_I).any(-1).all()     # every lane logged plies 0 .. T - 1
    assert (lg["v1"][:T] != _u32(np.float32(SENT_F))).all() and (lg["target"][:T] != _u32(np.float32(SENT_F))).all()
    assert _untouched(lg, (slice(T, None),))
    assert env._lib.bgamd_env_set_search_log(env._h, None, None, None, None, 0) == 0
    env.close()


# ---- (5) participation --------------------------------------------------------------------------------------------------------------------

def test_only_one_side_and_no_flip(bg, weights):
    n = 257
    st, tu, dice = (x[:n] for x in L.g10())
    env = bg.VecGame(n)
    env.load_weights(weights)
    both = _logged_step(bg, env, st, tu, dice, 3, 0.02)
    env.record_search_log(None)
    for side in (0, 1):
        run = _logged_step(bg, env, st, tu, dice, 3, 0.02, only_player=side)
        env.record_search_log(None)
        on = tu == side
        assert on.sum() > 60 and (~on).sum() > 60
        assert _untouched(run["log"], (slice(None), ~on))                  # the other side's lanes log nothing
        for f in both["log"]:
            assert np.array_equal(run["log"][f][0, on], both["log"][f][0, on]), (side, f)
        assert np.array_equal(run["post"][~on], st[~on])
    # BGAMD_NO_FLIP: the side to move stays, the logged afterstate still carries the other side's bit
    run = _logged_step(bg, env, st, tu, dice, 3, 0.02, no_flip=True)
    env.record_search_log(None)
    assert np.array_equal(run["turns"], tu)
    assert np.array_equal(run["log"]["after"][0], _rows(bg, run["post"], 1 - tu))
    assert ((run["log"]["after"][0, :, 0] >> 31) == (1 - tu)).all() and ((run["log"]["rows"][0, :, 0] >> 31) == tu).all()
    for f in both["log"]:
        assert np.array_equal(run["log"][f][0], both["log"][f][0]), f
    env.close()


# ---- (6) the learner takes it -------------------------------------------------------------------------------------------------------------

def test_the_learner_takes_it(bg, weights, played_round):
    from backgammon_env.learner import DeviceTDLambdaLearner
    (rows, lengths, p1_won, after, target, v1), _ = played_round
    n, T = ROUND["n"], int(rows.shape[0])
    Ld = DeviceTDLambdaLearner(weights, max_games=n)
    sq, cnt = Ld.replay_rows(rows, lengths, p1_won, batch_scale=24.0 / n)
    assert cnt == int(lengths.sum()) and np.isfinite(sq) and sq > 0
    # fit_search: every logged turn is handed over, the fit step skips and counts the turns that were not searched
    inside = torch.arange(T, device=rows.device)[:, None] < lengths[None, :]
    nans = int(torch.isnan(target[inside]).sum())
    assert 0 < nans < int(inside.sum())
    Lf = DeviceTDLambdaLearner(weights, max_games=n)
    mse = Lf.fit_search(after, target, lengths, epochs=1, batch=1024, seed=2)
    assert len(mse) == 1 and np.isfinite(mse[0])
    _, counted, skipped = Lf.last_fit_stats                 # what fit_stats reported (fit_rows reads it per epoch, which clears it)
    assert skipped == nans and counted == int(inside.sum()) - nans
    assert Lf.fit_stats() == (0.0, 0, 0)
    th = _np(Lf.theta)
    assert np.isfinite(th).all() and not np.array_equal(th, weights)
    # fit_rows on packed rows against fit on the same states: bit-identical weights
    st, tu, _ = (x[:500] for x in L.g10())
    y = np.random.RandomState(4).uniform(0, 1, 500).astype(np.float32)
    y[::37] = np.nan
    A, B = DeviceTDLambdaLearner(weights, max_games=8), DeviceTDLambdaLearner(weights, max_games=8)
    ma = A.fit(st, tu, y, epochs=2, batch=128, seed=3)
    mb = B.fit_rows(bg.pack_rows(st, tu), y, epochs=2, batch=128, seed=3)
    assert ma == mb and torch.equal(A.theta, B.theta) and A.last_fit_stats == B.last_fit_stats
    assert A.last_fit_stats[2] == 2 * int(np.isnan(y).sum())


# ---- (7) error codes and life cycle -------------------------------------------------------------------------------------------------------

def test_errors_and_life_cycle(bg, weights):
    n = 64
    st, tu, dice = (x[:n] for x in L.g10())
    env = bg.VecGame(n, seed=9)
    env.load_weights(weights)
    others = [lambda: env.step_greedy(auto_reset=False), lambda: env.run_greedy(2, auto_reset=False),
              lambda: env.step_sampled(0.5, auto_reset=False), lambda: env.run_sampled(2, 0.5, auto_reset=False),
              lambda: env.step_sampled(0.0, auto_reset=False), lambda: env.step_random(auto_reset=False),
              lambda: env.step_random(auto_reset=False, walk=True)]
    log = env.record_search_log(8)
    _fill(log)
    for step in others:                                     # no step but the search's while the log is set
        with pytest.raises(bg.BgamdError, match="-1"):
            step()
    for margin in (None, 0.04):                             # auto-reset: a lane's next game would write over its last one
        with pytest.raises(bg.BgamdError, match="-1"):
            env.step_search(top_k=2, auto_reset=True, margin=margin)
    assert _untouched(_log_np(log), (slice(None),)) and bool((env.progress()[0] == 0).all())       # the refused calls did nothing
    env.step_search(top_k=2, auto_reset=False)
    env.step_search(top_k=2, auto_reset=False, margin=0.04)
    assert (_log_np(log)["rows"][:2] != SENT_I).any(-1).all()
    # the trajectory and ring refusals are what they were, with both logs set; the search log's own rule holds beside them
    env.record_trajectory(8)
    with pytest.raises(bg.BgamdError, match="-1"):
        env.step_search(top_k=2, auto_reset=False)
    with pytest.raises(bg.BgamdError, match="-1"):
        env.step_greedy(auto_reset=False)
    env.record_trajectory(None)
    env.record_ring(8)
    with pytest.raises(bg.BgamdError, match="-1"):
        env.step_search(top_k=2, auto_reset=False, margin=0.04)
    env.record_ring(None)
    env.step_search(top_k=2, auto_reset=False)
    # max_plies 0
    buf = torch.zeros((4, n, 8), dtype=torch.int32, device=env.device)
    assert env._lib.bgamd_env_set_search_log(env._h, ctypes.c_void_p(buf.data_ptr()), None, None, None, 0) == -1
    assert env._lib.bgamd_env_set_search_log(env._h, ctypes.c_void_p(buf.data_ptr()), None, None, None, -3) == -1
    assert env._lib.bgamd_env_set_search_log(None, None, None, None, None, 0) == -1
    with pytest.raises(bg.BgamdError):
        env.record_search_log(0)
    with pytest.raises(bg.BgamdError, match="-1"):
        env.step_greedy(auto_reset=False)                   # the refused settings left the log as it was
    # rows alone: the other three pointers may be NULL
    buf.fill_(SENT_I)
    assert env._lib.bgamd_env_set_search_log(env._h, ctypes.c_void_p(buf.data_ptr()), None, None, None, 4) == 0
    env.reset()
    env.step_search(top_k=2, auto_reset=False)
    assert torch.equal(buf[0], log[0][0]) and bool((buf[1:] == SENT_I).all())       # the same opening rows as the round above logged
    # analyze_moves, rollout(plies=2) and evaluate_preroll ignore the log and leave it and the env untouched
    log = env.record_search_log(8)
    env.set_states(st, tu)
    env.set_dice(dice)
    _fill(log)
    before = (_np(env.states()), _np(env.turns()), _np(env.progress()[0]))
    res = env.analyze_moves(st, top_k=2)
    assert int((res["status"] == 3).sum()) > 0              # (the lanes' own boards are no afterstates: the analysis ran and said so)
    r = env.rollout(st[:8], tu[:8], 4, max_plies=2, plies=2, top_k=2, margin=0.04)
    assert bool(torch.isfinite(r["mean"]).all())
    env.evaluate_preroll(st[:8], tu[:8])
    assert _untouched(_log_np(log), (slice(None),))
    after_calls = (_np(env.states()), _np(env.turns()), _np(env.progress()[0]))
    assert all(np.array_equal(a, b) for a, b in zip(before, after_calls))
    # dropped: every step works again, search steps may restart games
    env.record_search_log(None)
    for step in others:
        step()
    env.step_search(top_k=2, auto_reset=True)
    env.step_search(top_k=2, auto_reset=True, margin=0.04)
    assert _untouched(_log_np(log), (slice(None),))
    assert env.stats()["error_flags"] == 0
    env.close()


# ---- (8) the example ----------------------------------------------------------------------------------------------------------------------

def test_the_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "search_fit.py"), "--games", "256", "--rounds", "1", "--td",
                        "--arena", "64", "--judge-turns", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert any(x.startswith("round 0:") and "mean |V2 - v1|" in x and "skipped" in x and "held-out mse" in x for x in lines), r.stdout
    assert any("judged by the starting one" in x for x in lines) and any(x.startswith("arena,") for x in lines) and lines[-1] == "done"
