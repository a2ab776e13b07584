"""The 3-ply search step on the MI355X (bgamd_env_step_search3, bgamd_env_search3_read, bgamd_env_search3_info: csrc/bg_search3.h and the
host code around it), lane by lane and bit for bit:
  (1) R3 and V3 by REPLAY: every (deep candidate, opponent roll) is searched again as a lane of a second env by bgamd_env_step_search, the
      reply filter applied to its (v1, v2) by the model, a roll without a move taken from evaluate_preroll; V3 = v2_from_replies(R3);
  (2) the 2-ply part against bgamd_env_step_search_filtered on a twin env;
  (3) the deep set, the depths, the choice, last_choice and search3_info against tests/search3_model.py on the device's own V2 / V3, with
      the exact ties the dyadic table brings;
  (4) the same lanes alone, in another order and beside others; BGAMD_SEARCH3_CHUNK = 256 against the default chunk;
  (5) deep_k = 1, deep_margin = 0 is the filtered step, flags and bookkeeping included; only_player, slot 1, the flip and the terminal flag;
  (6) error codes; a greedy step, a rollout and an analysis after a 3-ply step; the arena at 3 plies against 2.
Lane counts 1, 3, 65 and 295 (G10's first 288 boards and seven hand-built ones).  tests/test_search3_model_cpu.py holds the conditions
these rest on: the model against the whole tree, the census of the lane set."""
import os

import numpy as np
import pytest

import filter_model as F
import search3_model as S3
import search_lanes as L
import search_model as M
import search_ref as S
from test_gpu_search_rules import _np, _same_runs, _table, _u32
from test_search3_model_cpu import INF, NARROW, PARAMS, WIDE, lane_set

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FIELDS3 = ("kept", "states", "v1", "v2", "v3", "depth", "after", "value", "seq", "seq_len", "chosen", "count")


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


def _step3(env, params, **flags):
    top_k, mg, dk, dmg, rk, rmg = params
    env.step_search(top_k=top_k, margin=mg, plies=3, deep_k=dk, deep_margin=dmg, reply_top_k=rk, reply_margin=rmg, **flags)


def _results(env, names):
    out = dict(zip(names, (_np(x) for x in env.search_candidates())))
    out.update({k: _np(v) for k, v in env.last_choice().items()})
    out["after"] = _np(env.states())
    out["info"] = env.search_info()
    assert env.stats()["error_flags"] == 0
    return out


def _search3(env, st, tu, dice, params, **flags):
    """one 3-ply step of `env` from the given boards and dice (no roll, no flip, no restart unless asked for) -> every result as numpy"""
    env.set_states(st, tu)
    env.set_dice(dice)
    kw = dict(roll=False, auto_reset=False, no_flip=True)
    kw.update(flags)
    _step3(env, params, **kw)
    out = _results(env, ("states", "v1", "v2", "kept", "v3", "depth"))
    out["info3"] = env.search3_info()
    return out


def _filtered(env, st, tu, dice, top_k, margin, **flags):
    env.set_states(st, tu)
    env.set_dice(dice)
    kw = dict(roll=False, auto_reset=False, no_flip=True)
    kw.update(flags)
    env.step_search(top_k=top_k, margin=margin, **kw)
    return _results(env, ("states", "v1", "v2", "kept"))


def _zero_v3(run):
    """v3 is zero wherever depth < 3; depth is zero exactly past the kept count"""
    past = np.arange(run["depth"].shape[1])[None, :] >= run["kept"][:, None]
    assert not run["v3"][run["depth"] < 3].any() and np.array_equal(run["depth"] == 0, past)


_envs, _runs = {}, {}


@pytest.fixture(scope="module")
def runs(bg, weights):
    """(net, params) -> the 3-ply step over the whole lane set, on one env per net kept for the module"""
    def get(net, params):
        if (net, params) not in _runs:
            if net not in _envs:
                _envs[net] = bg.VecGame(len(lane_set()[0]))
                _envs[net].load_weights(_table(net, weights))
            _runs[net, params] = _search3(_envs[net], *lane_set(), params)
            _zero_v3(_runs[net, params])
        return _runs[net, params]
    yield get
    for e in _envs.values():
        e.close()
    _envs.clear()
    _runs.clear()


_index = {}


def _indices(run, i):
    """the reference-order indices of lane i's kept states, in the device's order"""
    st, tu, dice = lane_set()
    if i not in _index:
        _index[i] = L.index_of(np.ascontiguousarray(S.distinct_afterstates(st[i], int(tu[i]), int(dice[i, 0]), int(dice[i, 1])),
                                                    dtype=np.int32).reshape(-1, 28))
    rows = np.ascontiguousarray(run["states"][i, :int(run["kept"][i])], dtype=np.int32)
    return np.array([_index[i][r.tobytes()] for r in rows], np.int64)


NETS_PARAMS = [(net, p) for net in ("ckpt", "dyadic") for p in PARAMS]


# ---- (1) R3 and V3 by replay ---------------------------------------------------------------------------------------------------------------

def _replay(bg, w, run, tu, params):
    """-> (R3 float32 [D, 21] of the D non-terminal deep candidates in (lane, slot) order, their (lane, slot), the level-3 roots counted)"""
    _, _, _, _, rk, rmg = params
    lane, slot = np.where(run["depth"] == 3)
    live = run["states"][lane, slot, 26 + tu[lane]] != 15
    lane, slot = lane[live], slot[live]
    c = run["states"][lane, slot]
    D = len(lane)
    o = (1 - tu[lane]).astype(np.int32)
    env = bg.VecGame(D * 21)
    env.load_weights(w)
    rolls = np.array(S.ROLLS, np.int32)
    c21, o21, m21 = np.repeat(c, 21, axis=0), np.repeat(o, 21), np.repeat(tu[lane].astype(np.int32), 21)
    env.set_states(c21, o21)
    env.set_dice(np.tile(rolls, (D, 1)))
    env.step_search(top_k=rk, roll=False, auto_reset=False)
    kept = torch.zeros(D * 21, dtype=torch.int32, device=env.device)
    bg._capi.check(env._lib.bgamd_env_search_read(env._h, None, None, None, bg._ptr(kept), bg._stream()), "search_read")
    K = rk if rk else int(kept.max().item())
    v1, v2 = (torch.zeros((D * 21, K), dtype=torch.float32, device=env.device) for _ in range(2))
    bg._capi.check(env._lib.bgamd_env_search_read(env._h, None, bg._ptr(v1), bg._ptr(v2), None, bg._stream()), "search_read")
    kept, v1, v2, value = _np(kept), _np(v1), _np(v2), _np(env.last_choice()["value"])
    pre = _np(env.evaluate_preroll(c21, m21)[0])            # (computed for every mid lane, used where the opponent has no move)
    R3 = np.empty(D * 21, np.float32)
    for v in range(D * 21):
        k = int(kept[v])
        if k == 0:                                         # no move on a non-doubles roll: the pass reply's V2 = m's 21 rolls from c
            R3[v] = M.v2_from_replies(pre[v])
            continue
        keep = F.select(np.arange(k), v1[v, :k], o21[v], rk, rmg)
        R3[v] = S3.best_for(v2[v, keep], o21[v])
        if rmg == INF:
            assert _u32(R3[v]) == _u32(value[v]), v         # the replayed step's own choice
    # the level-3 roots: the filtered step on the same lanes counts 21 per non-terminal reply of the lanes that kept >= 2; a single kept
    # reply is searched too (terminal iff the lane's game ended with it), and so is the pass reply
    env.set_states(c21, o21)
    env.set_dice(np.tile(rolls, (D, 1)))
    env.step_search(top_k=rk, margin=rmg, roll=False, auto_reset=False)
    fkept = _np(env.search_candidates()[3])
    ended = (_np(env.flags()) & 4) != 0
    roots = env.search_info()[3] + 21 * int(((fkept == 1) & ~ended).sum()) + 21 * int((kept == 0).sum())
    assert env.stats()["error_flags"] == 0
    classes = dict(no_move_plain=int((kept == 0).sum()), single_reply=int((fkept == 1).sum()), ended=int(ended.sum()))
    env.close()
    return R3.reshape(D, 21), lane, slot, roots, classes


@pytest.mark.parametrize("net,params", NETS_PARAMS)
def test_r3_and_v3_by_replay(bg, weights, runs, net, params):
    run = runs(net, params)
    _, tu, _ = lane_set()
    R3, lane, slot, roots, classes = _replay(bg, _table(net, weights), run, tu, params)
    print("REPLAY %s %s: %d deep candidates, mid-lane classes %s" % (net, params, len(lane), classes))
    assert len(lane) >= 50
    if params == WIDE:
        assert classes["no_move_plain"] and classes["single_reply"] and classes["ended"]
    want = M.v2_from_replies(R3)
    assert np.array_equal(_u32(run["v3"][lane, slot]), _u32(want)), np.where(_u32(run["v3"][lane, slot]) != _u32(want))[0][:8]
    assert run["info3"][4] == 21 * len(lane) and run["info3"][5] == roots
    # a terminal deep candidate keeps its outcome
    tl, ts = np.where(run["depth"] == 3)
    term = run["states"][tl, ts, 26 + tu[tl]] == 15
    assert np.array_equal(_u32(run["v3"][tl[term], ts[term]]), _u32(np.where(tu[tl[term]] == 0, 1.0, 0.0)))
    if params == WIDE:
        assert term.any()


# ---- (2) the 2-ply part ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("net,params", NETS_PARAMS)
def test_two_ply_part_is_the_filtered_step(bg, weights, runs, net, params):
    run = runs(net, params)
    st, tu, dice = lane_set()
    twin = bg.VecGame(len(st))
    twin.load_weights(_table(net, weights))
    flt = _filtered(twin, st, tu, dice, params[0], params[1])
    twin.close()
    _same_runs(run, flt, "the 2-ply part", fields=("kept", "states", "v1", "v2", "count"))
    assert run["info"] == flt["info"] and run["info3"][:2] == flt["info"][:2]


# ---- (3) deep set, depth, choice, counts -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("net,params", NETS_PARAMS)
def test_deep_set_and_choice_against_the_model(runs, net, params):
    run = runs(net, params)
    st, tu, _ = lane_set()
    _, _, dk, dmg, _, _ = params
    seen = dict(deep=0, deep_cut=0, singleton=0, no_move=0, v2_tie_across=0, v3_tie_at_top=0, changed=0)
    n3 = n_deep = n_mid = 0
    for i in range(len(tu)):
        k, mover = int(run["kept"][i]), int(tu[i])
        if k == 0:
            assert np.array_equal(run["after"][i], st[i]), i
            seen["no_move"] += 1
            continue
        idx = _indices(run, i)
        v1, v2, v3, depth = run["v1"][i, :k], run["v2"][i, :k], run["v3"][i, :k], run["depth"][i, :k]
        if k == 1:
            assert depth[0] == 1 and _u32(run["value"][i]) == _u32(v1[0]) and np.array_equal(run["after"][i], run["states"][i, 0]), i
            seen["singleton"] += 1
            continue
        deep = S3.deep_set(idx, v2, mover, dk, dmg)
        in_deep = np.isin(idx, deep)
        if len(deep) == 1:
            j = int(np.where(in_deep)[0][0])
            assert (depth == 2).all() and _u32(run["value"][i]) == _u32(v2[j]) and j == M.choose(idx, v2, mover), i
            seen["deep_cut"] += 1
        else:
            assert np.array_equal(depth, np.where(in_deep, 3, 2)), (i, depth, deep)
            j = int(np.where(in_deep)[0][M.choose(idx[in_deep], v3[in_deep], mover)])
            assert _u32(run["value"][i]) == _u32(v3[j]), i
            seen["deep"] += 1
            seen["changed"] += j != M.choose(idx, v2, mover)
            srt = np.sort(M.bits(v2))
            seen["v2_tie_across"] += bool(dk and len(srt) > dk and (srt[::-1][dk - 1] == srt[::-1][dk] if mover == 0 else srt[dk - 1] == srt[dk]))
            b3 = M.bits(v3[in_deep])
            seen["v3_tie_at_top"] += int((b3 == (b3.max() if mover == 0 else b3.min())).sum()) >= 2
            n3 += 1; n_deep += len(deep)
            n_mid += 21 * int((run["states"][i, :k][in_deep][:, 26 + mover] != 15).sum())
        assert np.array_equal(run["after"][i], run["states"][i, j]), i
    print("CLASSES %s %s by the device's own values: %s" % (net, params, seen))
    moved = int((run["kept"] >= 1).sum())
    assert run["info3"][:5] == [moved, int((run["kept"] >= 2).sum()), n3, n_deep, n_mid]
    assert seen["deep"] >= 25 and seen["singleton"] and seen["no_move"] and seen["changed"]
    if params == NARROW:
        assert seen["deep_cut"] >= 1
    if net == "dyadic":
        assert seen["v3_tie_at_top"] >= 1                  # exact V3 ties decided by the key
        assert params != WIDE or seen["v2_tie_across"] >= 1  # exact V2 ties across the deep_k-th place


# ---- (4) independence ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [[288], [291, 5, 100], list(range(294, 229, -1))], ids=["1", "3", "65"])
def test_lanes_alone_and_in_another_order(bg, weights, runs, lanes):
    st, tu, dice = lane_set()
    for params in PARAMS:
        big = runs("ckpt", params)
        env = bg.VecGame(len(lanes))
        env.load_weights(weights)
        run = _search3(env, st[lanes], tu[lanes], dice[lanes], params)
        env.close()
        _same_runs(run, big, "lanes %s" % lanes[:3], lanes_b=lanes, fields=FIELDS3[:8] + ("seq", "seq_len"))
        assert len(lanes) < 65 or (run["depth"] == 3).any()


def test_chunk_independence(bg, weights, runs):
    st, tu, dice = lane_set()
    big = runs("ckpt", WIDE)
    os.environ["BGAMD_SEARCH3_CHUNK"] = "256"
    try:
        env = bg.VecGame(len(st))
        env.load_weights(weights)
        run = _search3(env, st, tu, dice, WIDE)
        again = _search3(env, st, tu, dice, NARROW)
    finally:
        del os.environ["BGAMD_SEARCH3_CHUNK"]
    env.close()
    assert run["info3"][4] > 4 * 256                       # more than one mid chunk was used
    _same_runs(run, big, "chunks of 256", fields=FIELDS3)
    _same_runs(again, runs("ckpt", NARROW), "chunks of 256, narrow", fields=FIELDS3)
    assert run["info3"] == big["info3"]


# ---- (5) collapse to 2 plies, flags ------------------------------------------------------------------------------------------------------------

def _book(env):
    r = {k: _np(v) for k, v in env.last_choice().items()}
    r.update(dict(zip(("states", "v1", "v2", "kept"), (_np(x) for x in list(env.search_candidates())[:4]))))
    r.update(after=_np(env.states()), turns=_np(env.turns()), flags=_np(env.flags()), dice=_np(env.dice()))
    r["ply"], r["episode"] = (_np(x) for x in env.progress())
    assert env.stats()["error_flags"] == 0
    return r


@pytest.mark.parametrize("auto_reset", [False, True])
def test_deep_k_1_is_the_filtered_step(bg, weights, auto_reset):
    st, tu, dice = lane_set()
    every = ("kept", "states", "v1", "v2", "value", "after", "turns", "flags", "dice", "ply", "episode", "seq", "seq_len", "chosen", "count")
    out = []
    for plies in (2, 3):
        env = bg.VecGame(len(st), seed=5)
        env.load_weights(weights)
        env.set_states(st, tu)
        env.set_dice(dice)
        steps = []
        for roll in (False, True):                         # the second step rolls; without auto-reset the finished lanes are frozen
            env.step_search(top_k=3, margin=INF, plies=plies, deep_k=1, deep_margin=0.0, roll=roll, auto_reset=auto_reset, want_index=True)
            steps.append(_book(env))
        if plies == 3:
            assert env.search3_info()[2:] == [0, 0, 0, 0]
            assert (_np(env.search_candidates()[5]) <= 2).all()
        env.close()
        out.append(steps)
    for a, b in zip(*out):
        _same_runs(a, b, "deep_k = 1", fields=every)
    assert (out[0][0]["flags"] & 0x14).any() and (out[0][1]["kept"] >= 2).sum() > 100


def test_flags(bg, weights, runs):
    st, tu, dice = lane_set()
    base = runs("ckpt", WIDE)
    env = bg.VecGame(len(st))
    env.load_weights(L.dyadic(), slot=0)
    env.load_weights(weights, slot=1)
    run = _search3(env, st, tu, dice, WIDE, slot=1)        # the other weight slot
    _same_runs(run, base, "slot 1", fields=FIELDS3)
    assert not np.array_equal(_search3(env, st, tu, dice, WIDE)["v3"], base["v3"])
    for side in (0, 1):                                    # one side only: the other side's lanes do not take part
        run = _search3(env, st, tu, dice, WIDE, slot=1, only_player=side)
        on = tu == side
        _same_runs(run, base, "only player %d" % side, lanes_a=on, lanes_b=on, fields=FIELDS3[:8])
        assert not run["kept"][~on].any() and np.array_equal(run["after"][~on], st[~on])
    run = _search3(env, st, tu, dice, WIDE, slot=1, no_flip=False, want_index=True)      # the flip and the terminal flag
    assert np.array_equal(run["after"], base["after"])
    over = base["after"][np.arange(len(tu)), 26 + tu] == 15
    assert over.any() and ((_np(env.flags()) & 4) != 0)[over].all()
    moved = (base["kept"] >= 1) & ~over
    assert np.array_equal(_np(env.turns())[moved], 1 - tu[moved])
    assert (run["count"] >= run["kept"]).all()
    env.close()


# ---- (6) plumbing ------------------------------------------------------------------------------------------------------------------------------

def test_errors(bg, weights):
    env = bg.VecGame(64)
    st, tu, dice = (x[:64] for x in lane_set())
    ok = dict(top_k=3, margin=INF, plies=3, deep_k=2, deep_margin=INF, reply_top_k=2, reply_margin=INF)
    with pytest.raises(bg.BgamdError, match="-6"):
        env.step_search(**ok)                              # no weights
    env.load_weights(weights)
    with pytest.raises(bg.BgamdError, match="-6"):
        env.step_search(slot=1, **ok)
    with pytest.raises(bg.BgamdError, match="-1"):
        env.search3_info()                                 # before the first 3-ply step
    assert env._lib.bgamd_env_search3_read(env._h, None, None, None) == -1
    for name in ("top_k", "deep_k", "reply_top_k"):
        with pytest.raises(bg.BgamdError, match="-1"):
            env.step_search(**dict(ok, **{name: -1}))
    for name in ("margin", "deep_margin", "reply_margin"):
        for bad in (-0.5, float("nan"), -INF):
            with pytest.raises(bg.BgamdError, match="-1"):
                env.step_search(**dict(ok, **{name: bad}))
    assert env._lib.bgamd_env_step_search3(None, 0, 3, 0.1, 2, 0.1, 2, 0.1, None) == -1
    assert env._lib.bgamd_env_search3_info(env._h, None) == -1 and env._lib.bgamd_env_search3_read(None, None, None, None) == -1
    env.record_trajectory(8)                               # the search step's refusals
    with pytest.raises(bg.BgamdError, match="-1"):
        env.step_search(**ok)
    env.record_trajectory(None)
    env.record_ring(8)
    with pytest.raises(bg.BgamdError, match="-1"):
        env.step_search(**ok)
    env.record_ring(None)
    env.record_search_log(8)                               # 3-ply targets are not logged
    with pytest.raises(bg.BgamdError, match="-1"):
        env.step_search(auto_reset=False, **ok)
    env.record_search_log(None)
    _search3(env, st, tu, dice, WIDE)
    assert env.search3_info()[2] > 0
    env.set_states(st, tu)
    env.set_dice(dice)
    env.step_search(top_k=3, margin=INF, roll=False, auto_reset=False)       # a step of another kind overwrites the search state
    assert env._lib.bgamd_env_search3_read(env._h, None, None, None) == -1
    with pytest.raises(bg.BgamdError, match="-1"):
        env.search3_info()
    assert len(env.search_candidates()) == 4
    env.close()


def test_other_features_after_a_3_ply_step(bg, weights):
    st, tu, dice = (x[:65] for x in lane_set())
    out = []
    for first in (False, True):
        env = bg.VecGame(65, seed=11)
        env.load_weights(weights)
        if first:
            _search3(env, st, tu, dice, WIDE)
        env.set_states(st, tu)
        env.set_dice(dice)
        env.step_greedy(roll=False, auto_reset=False, no_flip=True)
        r = {k: _np(v) for k, v in env.last_choice().items()}
        r["after"] = _np(env.states())
        ro = env.rollout(st[:8], tu[:8], 36, max_plies=6, per_trial=True)
        r.update(ro_mean=_np(ro["mean"]), ro_trial=_np(ro["trial_value"]))
        env.set_states(st, tu)
        env.set_dice(dice)
        an = env.analyze_moves(r["after"], top_k=3)
        r.update({"an_" + k: _np(an[k]) for k in ("status", "rank2", "v2_played", "v2_best", "error", "best")})
        assert env.stats()["error_flags"] == 0
        env.close()
        out.append(r)
    _same_runs(out[0], out[1], "after a 3-ply step", fields=tuple(out[0]))


def test_arena_three_plies_against_two(bg, weights):
    env = bg.VecGame(64, seed=3)
    from backgammon_env import arena
    r = arena.head_to_head(env, weights, L.dyadic(), max_turns=4, plies_a=3, plies_b=2, top_k=3, deep_k=2, reply_top_k=2)
    assert env.search3_info()[0] > 0 and env.stats()["error_flags"] == 0
    assert r["games"] >= 0 and set(r) >= {"win_rate", "ppg"}
    with pytest.raises(ValueError):
        arena.head_to_head(env, weights, None, plies_b=3)
    env.close()
