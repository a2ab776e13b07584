"""The filtered 2-ply search step on the MI355X (bgamd_env_step_search_filtered, bgamd_env_search_info: csrc/bg_filter.h and the host
code around it), lane by lane and bit for bit against the exact model tests/filter_model.py fed with the device's own float32 values:
  (1) the rule: kept sets, their order, kept[n], search_read, the choice and last_choice, V2 of every searched lane against the full-width
      run -- top_k 1, 3, 0 x the margins 0, the two margins candidates sit on exactly, a mid margin, +inf; checkpoint and dyadic table;
  (2) margin = +inf against step_search on every lane;
  (3) singletons cost no virtual root; margin 0 without exact ties plays the greedy step's move and scores nothing;
  (4) search_info after the plain step agrees with search_read;
  (9) error codes, weight slot 1, BGAMD_ONLY_P1/P2, the trajectory log's refusal.
tests/test_filter_model_cpu.py holds the conditions these rest on (the model, the lane classes)."""
import numpy as np
import pytest

import filter_model as F
import search_lanes as L
import search_model as M
from test_filter_model_cpu import INF, KS, MID
from test_gpu_search_rules import FIELDS, _g10_runs, _indices, _np, _same_runs, _search, _table, _u32, _zero_past_kept

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


def _filtered(env, st, tu, dice, top_k, margin, **flags):
    out = _search(env, st, tu, dice, top_k, margin=margin, **flags)
    out["info"] = env.search_info()
    return out


_envs = {}


@pytest.fixture(scope="module")
def g10_env(bg, weights):
    """one 1 500-lane env per net, kept for the module"""
    def get(net):
        if net not in _envs:
            _envs[net] = bg.VecGame(1500)
            _envs[net].load_weights(_table(net, weights))
        return _envs[net]
    yield get
    for e in _envs.values():
        e.close()
    _envs.clear()


def _margins(v1s, tu):
    return [0.0] + F.equality_margins(v1s, tu) + [MID, INF]


# ---- (1) the rule -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("top_k", KS)
@pytest.mark.parametrize("net", ["ckpt", "dyadic"])
def test_the_rule_bit_for_bit(bg, weights, g10_env, net, top_k):
    _, _, (v1s, v2s) = _g10_runs(bg, weights, net)         # the device's own v1 and V2 of every distinct afterstate (one full-width search)
    st, tu, dice = L.g10()
    env = g10_env(net)
    term = [L.terminal(L.afterstates(i), tu[i]) for i in range(len(tu))]
    seen = dict(cut=0, at_margin=0, made_single=0, forced=0, terminal=0)
    for mg in _margins(v1s, tu):
        run = _filtered(env, st, tu, dice, top_k, mg)
        _zero_past_kept(run)
        c = F.census(v1s, tu, term, top_k, mg)
        for k in seen:
            seen[k] += c[k]
        n_moved = n_searched = n_kept = n_roots = 0
        for i in range(len(tu)):
            m, mover = len(v1s[i]), int(tu[i])
            want = F.select(np.arange(m), v1s[i], mover, top_k, mg)
            k = len(want)
            assert int(run["kept"][i]) == k, (net, top_k, mg, i)
            if m == 0:
                assert np.array_equal(run["after"][i], st[i]), i
                continue
            idx = _indices(run, i)
            assert np.array_equal(idx, want), (net, top_k, mg, i, idx, want)
            assert np.array_equal(_u32(run["v1"][i, :k]), _u32(v1s[i][idx])), (net, top_k, mg, i)
            if k >= 2:                                   # searched: V2 depends on the candidate and the weights alone
                assert np.array_equal(_u32(run["v2"][i, :k]), _u32(v2s[i][idx])), (net, top_k, mg, i)
                n_searched += 1
                n_roots += 21 * int((~term[i][idx]).sum())
            else:                                        # a singleton: not searched, v2 = v1
                assert _u32(run["v2"][i, 0]) == _u32(run["v1"][i, 0]), (net, top_k, mg, i)
            j = M.choose(idx, run["v2"][i, :k], mover)
            assert np.array_equal(run["after"][i], run["states"][i, j]), (net, top_k, mg, i)
            assert _u32(run["value"][i]) == _u32(run["v2"][i, j]), (net, top_k, mg, i)
            n_moved += 1
            n_kept += k
        assert run["info"] == [n_moved, n_searched, n_kept, n_roots], (net, top_k, mg, run["info"])
        assert run["states"].shape[1] == (top_k if top_k else int(run["kept"].max()))
    print("CLASSES %s top_k %d, the device's own v1, summed over the margins: %s" % (net, top_k, seen))
    assert seen["forced"] and seen["terminal"]
    if top_k != 1:
        assert seen["cut"] and seen["made_single"]
        assert net != "dyadic" or seen["at_margin"] >= 10                  # candidates exactly at the margin: `<=` is tested


# ---- (2) margin = +inf against step_search -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("top_k", [3, 0])
def test_infinite_margin_against_step_search(bg, weights, top_k):
    st, tu, dice = (x[:777] for x in L.g10())
    out = []
    for margin in (None, INF):
        env = bg.VecGame(777, seed=5)
        env.load_weights(weights)
        env.set_states(st, tu)
        env.set_dice(dice)
        env.step_search(top_k=top_k, roll=False, auto_reset=True, want_index=True, margin=margin)      # flips, restarts finished games
        r = dict(zip(("states", "v1", "v2", "kept"), (_np(x) for x in env.search_candidates())))
        r.update({k: _np(v) for k, v in env.last_choice().items()})
        r.update(after=_np(env.states()), turns=_np(env.turns()), flags=_np(env.flags()), dice=_np(env.dice()))
        r["ply"], r["episode"] = (_np(x) for x in env.progress())
        assert env.stats()["error_flags"] == 0
        env.close()
        out.append(r)
    plain, flt = out
    every = ("kept", "states", "v1", "after", "turns", "flags", "dice", "ply", "episode", "seq", "seq_len", "chosen", "count")
    _same_runs(plain, flt, "margin inf", fields=every)
    many = plain["kept"] >= 2
    assert many.sum() > 300 and (plain["kept"] == 1).sum() > 100
    _same_runs(plain, flt, "margin inf, searched lanes", lanes_a=many, lanes_b=many, fields=("v2", "value"))
    one = plain["kept"] == 1
    assert np.array_equal(_u32(flt["v2"][one, 0]), _u32(plain["v1"][one, 0]))
    assert np.array_equal(_u32(flt["value"][one]), _u32(plain["v1"][one, 0]))
    assert (plain["count"] > plain["kept"]).any() and (plain["flags"] & 0x10).any()      # exact counts with copies; games that ended


# ---- (3) singletons cost nothing ------------------------------------------------------------------------------------------------------------

def test_margin_zero_is_the_greedy_step(bg, weights, g10_env):
    _, _, (v1s, _) = _g10_runs(bg, weights, "ckpt")
    st, tu, dice = L.g10()
    # lanes whose best 1-ply value is held by ONE candidate (by the device's own values): margin 0 keeps that one alone.  Lanes with a
    # terminal candidate are left out: the search scores it by its outcome (item 2 of the header), the greedy step by the net
    lanes = np.array([i for i in range(len(tu))
                      if len(v1s[i]) == 0 or (len(F.select(np.arange(len(v1s[i])), v1s[i], int(tu[i]), 0, 0.0)) == 1
                                              and not L.terminal(L.afterstates(i), tu[i]).any())])
    assert len(lanes) > 1300 and sum(len(v1s[i]) >= 2 for i in lanes) > 1000
    env = bg.VecGame(len(lanes))
    env.load_weights(weights)
    run = _filtered(env, st[lanes], tu[lanes], dice[lanes], 5, 0.0)
    moved = int((run["kept"] == 1).sum())
    assert run["info"] == [moved, 0, moved, 0] and (run["kept"] <= 1).all()
    env.set_states(st[lanes], tu[lanes])
    env.set_dice(dice[lanes])
    env.step_greedy(roll=False, auto_reset=False, no_flip=True)
    greedy = {k: _np(v) for k, v in env.last_choice().items()}
    assert np.array_equal(_np(env.states()), run["after"])
    has = run["kept"] == 1
    assert np.array_equal(_u32(run["value"][has]), _u32(greedy["value"][has]))
    assert np.array_equal(run["seq"], greedy["seq"]) and np.array_equal(run["seq_len"], greedy["seq_len"])
    env.close()


# ---- (4) the unfiltered step ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("top_k", [3, 0])
def test_search_info_after_the_plain_step(bg, weights, top_k):
    runs, _, _ = _g10_runs(bg, weights, "ckpt")
    st, tu, dice = (x[:512] for x in L.g10())
    env = bg.VecGame(512)
    env.load_weights(weights)
    with pytest.raises(bg.BgamdError, match="-1"):
        env.search_info()                                  # before the first search step
    run = _search(env, st, tu, dice, top_k)
    info = env.search_info()
    assert env.search_info() == info
    _same_runs(run, runs[top_k], "the plain step, as ever", lanes_b=slice(0, 512))
    has = np.arange(run["states"].shape[1])[None, :] < run["kept"][:, None]
    lane = np.broadcast_to(np.arange(512)[:, None], has.shape)[has]
    term = run["states"][has][np.arange(has.sum()), 26 + tu[lane]] == 15
    moved = int((run["kept"] >= 1).sum())
    assert info == [moved, moved, int(run["kept"].sum()), 21 * int((~term).sum())] and term.any()
    env.analyze_moves(run["after"], top_k=2)               # an analysis invalidates the search results
    with pytest.raises(bg.BgamdError, match="-1"):
        env.search_info()
    env.close()


# ---- (9) plumbing -----------------------------------------------------------------------------------------------------------------------------

def test_errors(bg, weights):
    env = bg.VecGame(64)
    st, tu, dice = (x[:64] for x in L.g10())
    with pytest.raises(bg.BgamdError, match="-6"):
        env.step_search(top_k=2, margin=0.1)               # no weights
    env.load_weights(weights)
    for bad in (-0.5, float("nan"), -INF):
        with pytest.raises(bg.BgamdError, match="-1"):
            env.step_search(top_k=2, margin=bad)
    with pytest.raises(bg.BgamdError, match="-1"):
        env.step_search(top_k=-1, margin=0.1)
    with pytest.raises(bg.BgamdError, match="-6"):
        env.step_search(top_k=2, margin=0.1, slot=1)
    assert env._lib.bgamd_env_step_search_filtered(None, 0, 2, 0.1, None) == -1
    assert env._lib.bgamd_env_search_info(env._h, None) == -1 and env._lib.bgamd_env_search_info(None, None) == -1
    env.record_trajectory(8)                               # a search step logs nothing: refused, as the plain step is
    with pytest.raises(bg.BgamdError, match="-1"):
        env.step_search(top_k=2, margin=0.1)
    with pytest.raises(bg.BgamdError, match="-1"):
        env.step_search(top_k=2)
    env.record_trajectory(None)
    _filtered(env, st, tu, dice, 2, 0.1)
    env.close()


def test_weight_slot_1(bg, weights):
    st, tu, dice = (x[:256] for x in L.g10())
    a = bg.VecGame(256)
    a.load_weights(L.dyadic(), slot=0)
    a.load_weights(weights, slot=1)
    b = bg.VecGame(256)
    b.load_weights(weights)
    ra, rb = _filtered(a, st, tu, dice, 3, MID, slot=1), _filtered(b, st, tu, dice, 3, MID)
    _same_runs(ra, rb, "slot 1 against slot 0")
    assert ra["info"] == rb["info"]
    r0 = _filtered(a, st, tu, dice, 3, MID)
    assert not np.array_equal(r0["v1"], ra["v1"])
    a.close()
    b.close()


def test_only_one_side(bg, weights, g10_env):
    st, tu, dice = L.g10()
    env = g10_env("ckpt")
    both = _filtered(env, st, tu, dice, 3, MID)
    for side in (0, 1):
        run = _filtered(env, st, tu, dice, 3, MID, only_player=side)
        on = tu == side
        assert on.sum() > 500
        _same_runs(run, both, "only player %d" % side, lanes_a=on, lanes_b=on, fields=FIELDS[:8])
        assert not run["kept"][~on].any() and np.array_equal(run["after"][~on], st[~on])
        assert run["info"][0] == int((both["kept"][on] >= 1).sum()) and run["info"][1] == int((both["kept"][on] >= 2).sum())
