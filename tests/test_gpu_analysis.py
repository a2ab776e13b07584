"""The move analysis on the MI355X (bgamd_env_analyze_moves / bgamd_env_analysis_read: csrc/bg_analysis.h and SearchCall in
csrc/bgamd.hip), lane by lane and bit for bit against the exact model tests/analysis_model.py fed with the device's own float32 values:
one full-width search per net on the 1 500 G10 boards (test_gpu_search_rules' cached runs) gives v1 and V2 of every distinct afterstate
by reference index; every analysis below -- any top_k, any played candidate, one to four scoring passes -- must report exactly what
the model makes of those values.  tests/test_analysis_model_cpu.py holds the conditions these rest on."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import analysis_model as A
import search_lanes as L
import test_gpu_search_rules as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KS = (1, 3, 8, 0)
E_INVALID, E_NOWEIGHTS = -1, -6
_np, _u32 = R._np, R._u32


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


def _analyse(env, played, top_k, **kw):
    out = env.analyze_moves(played, top_k=top_k, **kw)
    assert env.stats()["error_flags"] == 0
    return {k: (v if k == "summary" else _np(v)) for k, v in out.items()}


_envs = {}


def _env(bg, weights, net):
    """per net: a 1 500-lane env standing on the G10 boards and dice (an analysis moves nothing: it is set up once), and the full-width
    search's v1 / V2 by reference index"""
    if net not in _envs:
        _, _, (v1s, v2s) = R._g10_runs(bg, weights, net)
        st, tu, dice = L.g10()
        env = bg.VecGame(len(st))
        env.load_weights(R._table(net, weights))
        env.set_states(st, tu)
        env.set_dice(dice)
        _envs[net] = (env, v1s, v2s)
    return _envs[net]


def _played(family, v1s, v2s, top_k, lanes=None):
    """-> (played boards [n, 28], played reference indices [n]) of a family; a lane without a move "plays" its own board"""
    st, tu, _ = L.g10()
    lanes = range(len(tu)) if lanes is None else lanes
    idx = np.array([A.played_index(family, v1s[i], v2s[i], int(tu[i]), top_k) if len(v1s[i]) else -1 for i in lanes])
    return np.stack([L.afterstates(i)[p] if p >= 0 else st[i] for i, p in zip(lanes, idx)]).astype(np.int32), idx


def _expect(v1s, v2s, top_k, idx, lanes=None, takes_part=None):
    tu = L.g10()[1]
    lanes = range(len(tu)) if lanes is None else lanes
    return [A.analyse(v1s[i], v2s[i], int(tu[i]), top_k, int(p), True if takes_part is None else bool(takes_part[i]))
            for i, p in zip(lanes, idx)]


def _check(got, want, what, lanes=None):
    """every per-lane field of a device result against the model's, bit for bit"""
    st = L.g10()[0]
    lanes = list(range(len(st)) if lanes is None else lanes)
    for k in A.FIELDS:
        w = np.array([r[k] for r in want], got[k].dtype)
        same = got[k].view(np.uint32) == w.view(np.uint32)
        assert same.all(), (what, k, "lanes", np.where(~same)[0][:8].tolist(), got[k][~same][:4].tolist(), w[~same][:4].tolist())
    best = np.stack([L.afterstates(i)[r["best"]] if r["best"] >= 0 else np.zeros(28, np.int32) for i, r in zip(lanes, want)])
    same = (got["best"] == best).all(1)
    assert same.all(), (what, "best28", np.where(~same)[0][:8].tolist())


def _check_summary(got, want, movers, what):
    """counts and the largest error exact; the sum within n roundings of an fp64 running sum of math.fsum of the per-lane errors"""
    s, ref = got["summary_raw"], A.summary(want, movers)
    n = len(want)
    for q in range(12):
        if q in (3, 8):
            assert abs(s[q] - ref[q]) <= n * 2.0 ** -52 * ref[q], (what, q, s[q], ref[q])
        else:
            assert s[q] == ref[q], (what, q, s[q], ref[q])
    named = got["summary"]
    assert [named["player1"][k] for k in ("decisions", "unforced", "mistakes", "error_sum", "max_error")] == s[:5].tolist()
    assert [named["player2"][k] for k in ("decisions", "unforced", "mistakes", "error_sum", "max_error")] == s[5:10].tolist()
    assert (named["no_move"], named["not_found"]) == (s[10], s[11])


_results = {}


def _run(bg, weights, net, top_k, family):
    """the 1 500-lane analysis of a family, cached: (device result, model results)"""
    key = (net, top_k, family)
    if key not in _results:
        env, v1s, v2s = _env(bg, weights, net)
        boards, idx = _played(family, v1s, v2s, top_k)
        _results[key] = (_analyse(env, boards, top_k), _expect(v1s, v2s, top_k, idx))
    return _results[key]


# ---- 1. fields against the model ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("top_k", KS)
@pytest.mark.parametrize("net", ["ckpt", "dyadic"])
def test_fields_against_the_model(bg, weights, net, top_k):
    """v2_played / v2_best are the full-width run's V2 of that candidate, bit for bit: the forced candidate is scored like any other, over
    one (K = 1, 3), three (K = 8: the bound n (K + 1) 21) and four (K = 0) scoring passes"""
    tu = L.g10()[1]
    _, v1s, _ = _env(bg, weights, net)
    n_forced = n_tied_outside = 0
    for family in A.FAMILIES:
        got, want = _run(bg, weights, net, top_k, family)
        _check(got, want, (net, top_k, family))
        _check_summary(got, want, tu, (net, top_k, family))
        assert (got["error"] >= 0).all() and ((got["error"] == 0) == (_u32(got["v2_played"]) == _u32(got["v2_best"]))).all()
        if top_k:
            forced = np.array([r["status"] == A.OK and r["rank1"] >= top_k for r in want])
            n_forced += int(forced.sum())
            if family == "first_out":
                n_tied_outside += sum(bool(f) and L.tie_across(v1s[i], tu[i], top_k) for i, f in enumerate(forced))
    if top_k:
        assert n_forced >= 300, n_forced
    if net == "dyadic" and top_k in (3, 8):
        assert n_tied_outside >= 100, n_tied_outside       # the played move is the tied one just outside the top K


# ---- 2. statuses --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["illegal", "bad"])
def test_played_state_that_is_no_afterstate(bg, weights, kind):
    env, v1s, v2s = _env(bg, weights, "ckpt")
    st, tu, _ = L.g10()
    boards = st.copy()
    if kind == "bad":
        boards[:, 5] = 16                                   # cannot be packed: matches nothing, raises nothing
        idx = np.full(len(st), -1)
    else:                                                   # the lane's own board: an afterstate only as a doubles roll's empty sequence
        idx = np.array([L.index_of(L.afterstates(i)).get(st[i].tobytes(), -1) if len(v1s[i]) else -1 for i in range(len(st))])
        assert (idx >= 0).sum() == 36 and all(len(v1s[i]) == 1 for i in np.where(idx >= 0)[0])
    got = _analyse(env, boards, 3)
    want = _expect(v1s, v2s, 3, idx)
    _check(got, want, kind)
    _check_summary(got, want, tu, kind)
    c = L.counts()
    assert (got["status"][c == 0] == A.NO_MOVE).all() and (got["status"][(c > 0) & (idx < 0)] == A.NOT_FOUND).all()
    nf = got["status"] == A.NOT_FOUND
    assert nf.sum() >= 1400 and (got["rank1"][nf] == -1).all() and (got["rank2"][nf] == -1).all()
    assert (got["distinct"][nf] == c[nf]).all() and got["best"][nf].any(1).all()
    for k in ("v1_played", "v2_played", "error"):
        assert not got[k][nf].any(), k
    assert got["summary"]["no_move"] == 47 and got["summary"]["not_found"] == int(nf.sum())


@pytest.mark.parametrize("side", [0, 1])
def test_only_player(bg, weights, side):
    """the other side's lanes take no part: status 1, everything else 0; the side's five numbers are the two-sided call's, bit for bit"""
    env, v1s, v2s = _env(bg, weights, "dyadic")
    tu = L.g10()[1]
    both, _ = _run(bg, weights, "dyadic", 3, "worst")
    boards, idx = _played("worst", v1s, v2s, 3)
    got = _analyse(env, boards, 3, only_player=side)
    want = _expect(v1s, v2s, 3, idx, takes_part=tu == side)
    _check(got, want, ("only", side))
    out = tu != side
    assert (got["status"][out] == A.IDLE).all() and not got["best"][out].any()
    s, b = got["summary_raw"], both["summary_raw"]
    assert s[5 * side:5 * side + 5].tobytes() == b[5 * side:5 * side + 5].tobytes() and s[5 * side] > 600
    assert not s[5 * (1 - side):5 * (1 - side) + 5].any()
    assert s[10] == ((L.counts() == 0) & (tu == side)).sum() and s[11] == 0


# ---- 3. cross-check with the search step and the greedy step ------------------------------------------------------------------------------

@pytest.mark.parametrize("net", ["ckpt", "dyadic"])
def test_against_the_search_step_and_the_greedy_step(bg, weights, net):
    runs, _, (v1s, _) = R._g10_runs(bg, weights, net)
    st, tu, dice = L.g10()
    sib = bg.VecGame(len(st))
    sib.load_weights(R._table(net, weights))
    sib.set_states(st, tu)
    sib.set_dice(dice)
    sib.step_greedy(roll=False, auto_reset=False, no_flip=True)
    value = _np(sib.last_choice()["value"])
    sib.close()
    no_term = np.array([len(v1s[i]) > 0 and not L.terminal(L.afterstates(i), tu[i]).any() for i in range(len(st))])
    n_inside = n_best = 0
    for K in (1, 3, 8):
        for family in ("best", "inside", "v2best", "worst"):
            got, _ = _run(bg, weights, net, K, family)
            boards, _ = _played(family, *_env(bg, weights, net)[1:], K)
            inside = (got["status"] == A.OK) & (got["rank1"] < K)
            lands = (runs[K]["after"] == boards).all(1)     # a twin env's step_search(top_k = K) from the same boards and dice
            assert ((got["rank2"] == 0) == lands)[inside].all(), (net, K, family)
            assert np.array_equal(_u32(got["v1_best"][no_term]), _u32(value[no_term])), (net, K, family)
            n_inside += int(inside.sum()); n_best += int((inside & lands).sum())
    assert n_inside > 6000 and 2000 < n_best < n_inside


# ---- 4. no side effect --------------------------------------------------------------------------------------------------------------------

def test_no_side_effect(bg, weights):
    n = 512
    st, tu, dice = (x[:n] for x in L.g10())
    _, v1s, v2s = _env(bg, weights, "ckpt")
    boards, _ = _played("first_out", v1s, v2s, 3, range(n))
    envs = [bg.VecGame(n, seed=5) for _ in range(2)]
    for e in envs:
        e.load_weights(weights)
        e.step_greedy()                                     # (a last_choice to keep, counters that are not zero)
        e.step_search(top_k=2)
        e.set_states(st, tu)
        e.set_dice(dice)
    env, twin = envs

    def state(e):
        s = e.stats()
        return ([_np(e.snapshot())] + [_np(x) for x in e.progress()] + [_np(v) for v in e.last_choice().values()],
                (s["steps"], s["games_finished"], s["p1_wins"]))
    before = state(env)
    env.search_candidates()                                 # readable before the analysis ...
    got = _analyse(env, boards, 3)
    assert (got["status"] == A.OK).sum() > 400
    after = state(env)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before[0], after[0])) and before[1] == after[1]
    rc = env._lib.bgamd_env_search_read(env._h, None, None, None, None, None)
    assert rc == E_INVALID                                  # ... and invalidated by it
    for step in ("greedy", "search"):
        for e in envs:
            if step == "greedy":
                e.step_greedy(roll=False, auto_reset=False)
            else:
                e.set_states(st, tu)
                e.set_dice(dice)
                e.step_search(top_k=3, roll=False, auto_reset=False)
        a, b = state(env), state(twin)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0])) and a[1] == b[1], step
    for x, y in zip(env.search_candidates(), twin.search_candidates()):
        assert _np(x).tobytes() == _np(y).tobytes()
    assert env.stats()["error_flags"] == 0
    for e in envs:
        e.close()


# ---- 5. the summary -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("net", ["ckpt", "dyadic"])
def test_summary(bg, weights, net):
    """(counts, sum and maximum against numpy / math.fsum: _check_summary in every test above)  Two calls are bit-identical; ONLY_P1 and
    ONLY_P2 calls reproduce the per-side halves bit for bit."""
    env, v1s, v2s = _env(bg, weights, net)
    tu = L.g10()[1]
    first, want = _run(bg, weights, net, 3, "worst")
    boards, _ = _played("worst", v1s, v2s, 3)
    again = _analyse(env, boards, 3)
    for k in A.FIELDS + ("best", "summary_raw"):
        assert first[k].tobytes() == again[k].tobytes(), k
    halves = [_analyse(env, boards, 3, only_player=side)["summary_raw"] for side in (0, 1)]
    assert np.concatenate([halves[0][:5], halves[1][5:10]]).tobytes() == first["summary_raw"][:10].tobytes()
    assert halves[0][10] + halves[1][10] == first["summary_raw"][10] == 47
    s = first["summary_raw"]
    err = first["error"].astype(np.float64)
    ok = first["status"] == A.OK
    for side in (0, 1):
        m = ok & (tu == side)
        assert s[5 * side] == m.sum() and s[5 * side + 1] == (m & (first["distinct"] >= 2)).sum() and s[5 * side + 2] == (m & (err > 0)).sum()
        ref = math.fsum(err[m].tolist())
        assert abs(s[5 * side + 3] - ref) <= len(tu) * 2.0 ** -52 * ref and s[5 * side + 4] == err[m].max() and s[5 * side + 2] > 100


# ---- 6. shapes ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 257])
def test_lane_counts(bg, weights, n):
    st, tu, dice = (x[:n] for x in L.g10())
    _, v1s, v2s = _env(bg, weights, "ckpt")
    big, _ = _run(bg, weights, "ckpt", 3, "first_out")
    boards, idx = _played("first_out", v1s, v2s, 3, range(n))
    env = bg.VecGame(n)
    env.load_weights(weights)
    env.set_states(st, tu)
    env.set_dice(dice)
    got = _analyse(env, boards, 3)
    env.close()
    for k in A.FIELDS + ("best",):
        assert got[k].tobytes() == big[k][:n].tobytes(), (n, k)
    want = _expect(v1s, v2s, 3, idx, range(n))
    _check_summary(got, want, tu, n)


def test_weight_slots(bg, weights):
    """slot 1 against slot 0 with the tables swapped"""
    n = 257
    st, tu, dice = (x[:n] for x in L.g10())
    _, v1s, v2s = _env(bg, weights, "ckpt")
    boards, _ = _played("worst", v1s, v2s, 3, range(n))
    out = []
    for tables in ((L.dyadic(), weights), (weights, L.dyadic())):
        env = bg.VecGame(n)
        for slot, w in enumerate(tables):
            env.load_weights(w, slot=slot)
        env.set_states(st, tu)
        env.set_dice(dice)
        out.append([_analyse(env, boards, 3, slot=slot) for slot in (0, 1)])
        env.close()
    big, _ = _run(bg, weights, "ckpt", 3, "worst")
    for k in A.FIELDS + ("best", "summary_raw"):
        assert out[0][0][k].tobytes() == out[1][1][k].tobytes() and out[0][1][k].tobytes() == out[1][0][k].tobytes(), k
        assert k == "summary_raw" or out[0][1][k].tobytes() == big[k][:n].tobytes(), k
    assert out[0][0]["v2_played"].tobytes() != out[0][1]["v2_played"].tobytes()


# ---- 7. error codes -------------------------------------------------------------------------------------------------------------------------

def test_error_codes(bg, weights):
    from backgammon_env import _capi
    n = 64
    st, tu, dice = (x[:n] for x in L.g10())
    env = bg.VecGame(n)
    lib, h = env._lib, env._h
    played = torch.as_tensor(st).to(env.device).contiguous()
    p = played.data_ptr()
    read = lambda: lib.bgamd_env_analysis_read(h, *([None] * 12))
    assert read() == E_INVALID                              # before the first analysis
    assert lib.bgamd_env_analyze_moves(h, 0, 4, p, None) == E_NOWEIGHTS
    env.load_weights(weights)
    assert lib.bgamd_env_analyze_moves(h, _capi.WEIGHTS_SLOT1, 4, p, None) == E_NOWEIGHTS
    assert lib.bgamd_env_analyze_moves(h, 0, 4, None, None) == E_INVALID
    assert lib.bgamd_env_analyze_moves(None, 0, 4, p, None) == E_INVALID
    assert lib.bgamd_env_analyze_moves(h, 0, -1, p, None) == E_INVALID
    for flag in (_capi.ROLL, _capi.AUTO_RESET, _capi.NO_FLIP, _capi.WANT_INDEX):
        assert lib.bgamd_env_analyze_moves(h, flag, 4, p, None) == E_INVALID, flag
    assert read() == E_INVALID
    env.set_states(st, tu)
    env.set_dice(dice)
    assert lib.bgamd_env_analyze_moves(h, 0, 4, p, None) == 0 and read() == 0
    env.record_trajectory(8)
    assert lib.bgamd_env_analyze_moves(h, 0, 4, p, None) == E_INVALID
    assert read() == 0                                      # (refused before anything ran: the last analysis still stands)
    env.record_trajectory(None)
    env.record_ring(8)
    assert lib.bgamd_env_analyze_moves(h, 0, 4, p, None) == E_INVALID
    env.record_ring(None)
    assert lib.bgamd_env_analyze_moves(h, _capi.ONLY_P1, 0, p, None) == 0 and read() == 0
    torch.cuda.synchronize()
    assert env.stats()["error_flags"] == 0
    env.close()


# ---- 8. error_rate end to end ---------------------------------------------------------------------------------------------------------------

def test_error_rate(bg, weights):
    from backgammon_env import analysis
    n, turns = 512, 24
    judge = bg.VecGame(n)
    judge.load_weights(weights)
    judge_before = _np(judge.progress()[0]).copy()
    seen = {"decisions": 0, "checked": 0}

    def on_turn(t, player, res):
        ok = _np(res["status"]) == A.OK
        running = (_np(player.flags()) & 4) == 0             # the played move was not the game's last
        value = _np(player.last_choice()["value"])
        assert np.array_equal(_u32(_np(res["v1_played"])[ok & running]), _u32(value[ok & running])), t
        assert (_np(res["rank1"])[ok] == 0).all(), t         # player = judge, no exploration: the 1-ply choice
        seen["decisions"] += int(ok.sum()); seen["checked"] += int((ok & running).sum())
    out = {}
    for eps in (0.0, 0.25):
        player = bg.VecGame(n, seed=77)
        player.load_weights(weights)
        out[eps] = r = analysis.error_rate(player, judge, turns, top_k=4, epsilon=eps, on_turn=on_turn if eps == 0.0 else None)
        player.close()
        tot = r["total"]
        assert tot["illegal"] == 0 and r["player1"]["illegal"] == 0 and r["player2"]["illegal"] == 0     # (the dice the step played were read back)
        assert tot["decisions"] + tot["passes"] + tot["idle"] == r["lane_turns"] == n * turns
        assert tot["error_sum"] >= 0 and tot["unforced"] > 0.8 * n * turns and 0 <= tot["mistakes"] <= tot["unforced"]
        for k in ("decisions", "unforced", "mistakes", "passes"):
            assert r["player1"][k] + r["player2"][k] == tot[k], k
        assert tot["error_rate"] == tot["error_sum"] / tot["unforced"] and tot["agreement"] == 1 - tot["mistakes"] / tot["unforced"]
    assert seen["decisions"] == out[0.0]["total"]["decisions"] and seen["checked"] > 0.9 * n * turns
    assert out[0.25]["total"]["mistakes"] > out[0.0]["total"]["mistakes"]
    assert np.array_equal(_np(judge.progress()[0]), judge_before) and judge.stats()["steps"] == 0     # the judge is never stepped
    judge.close()


# ---- 9. the example -------------------------------------------------------------------------------------------------------------------------

def test_example():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "error_rate.py"), "--games", "256", "--turns", "8"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert any("error_rate" in x and "agreement" in x for x in lines), r.stdout
    for row in ("player1", "player2", "total"):
        assert any(x.split()[:1] == [row] for x in lines), (row, r.stdout)
