"""The search's host plan on the MI355X (csrc/bg_search_plan.h as bgamd.hip's SearchCall issues it): after ONE call of each kind on a
fresh 256-lane env -- scratch_env keeps an env that is large enough, so a used env would prove nothing -- the internal envs have the
lanes tests/search_plan_ref.py gives for the counts search_info() / search3_info() report.  Mixed positions a few steps past the
opening (no candidate ends a game there, so the virtual roots scored are all the virtual lanes), the dyadic table.  And what an analysis
leaves behind: search_read and search_info refuse.  The results themselves are held by the suites of the single features."""
import os

import pytest

import search_lanes as L
import search_plan_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 256
B = R.bits


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


def _fresh(bg):
    env = bg.VecGame(N, seed=77)
    env.load_weights(L.dyadic())
    for _ in range(6):
        env.step_greedy(auto_reset=False)
    assert env.scratch_info() == [0, 0, 0] and env.stats()["games_finished"] == 0
    return env


def _plan(kind, top_k, margin=0.0, h=(0, 0, 0), **three):
    q = (kind, 0, top_k, B(margin), three.get("deep_k", 0), B(three.get("deep_margin", 0.0)), three.get("reply_top_k", 0),
         B(three.get("reply_margin", 0.0)), int(kind == R.ANALYSIS), N, 0, 0, 0, 1, 1, *h)
    p = R.plan(q)
    assert p["rc"] == 0
    return p


@pytest.mark.parametrize("top_k", [5, 0])
def test_plain_step(bg, top_k):
    env = _fresh(bg)
    env.step_search(top_k=top_k, auto_reset=False)
    moved, searched, kept, roots = env.search_info()
    assert 0 < moved == searched <= N and roots == 21 * kept and kept >= moved
    p = _plan(R.STEP, top_k, h=(kept, 0, 0))
    assert p["n_virtual"] == (21 * N * top_k if top_k else roots)
    assert env.scratch_info() == [p["scratch_lanes"], 0, 0] and env.stats()["error_flags"] == 0
    env.close()


@pytest.mark.parametrize("top_k,margin", [(5, 0.04), (0, float("inf")), (3, 0.0)])
def test_filtered_step(bg, top_k, margin):
    env = _fresh(bg)
    env.step_search(top_k=top_k, margin=margin, auto_reset=False)
    moved, searched, kept, roots = env.search_info()
    assert 0 < moved <= N and roots % 21 == 0 and kept >= moved
    p = _plan(R.FILTERED, top_k, margin, h=(kept, 0, roots // 21))
    assert p["n_virtual"] == roots and (searched > 0) == (roots > 0)
    assert env.scratch_info() == [p["scratch_lanes"], 0, 0] and env.stats()["error_flags"] == 0
    env.close()


@pytest.mark.parametrize("chunk", [None, "256"])
def test_three_ply_step_and_its_mid_env(bg, chunk):
    """the mid env's lanes exactly; the scratch env has served the root level and every mid search, whose virtual lanes are the level-3
    roots scored and 21 for every pass reply (one per mid lane at most): with one chunk that bounds its lanes from both sides"""
    params = dict(deep_k=2, deep_margin=float("inf"), reply_top_k=2, reply_margin=float("inf"))
    if chunk:
        os.environ["BGAMD_SEARCH3_CHUNK"] = chunk
    try:
        env = _fresh(bg)
        env.step_search(top_k=3, margin=float("inf"), plies=3, auto_reset=False, **params)
    finally:
        if chunk:
            del os.environ["BGAMD_SEARCH3_CHUNK"]
    moved, searched, kept, roots = env.search_info()
    moved3, at2, at3, n_deep, n_mid, l3 = env.search3_info()
    root = _plan(R.THREE_PLY, 3, float("inf"), h=(kept, 0, roots // 21), **params)
    assert root["n_virtual"] == roots and at3 > 0
    d = R.deep(n_deep, R.chunk(chunk))
    assert d["n_mid"] == n_mid and (d["chunks"] > 1) == (chunk is not None)
    lanes = env.scratch_info()
    assert lanes[1:] == [0, d["mid_lanes"]] and d["mid_lanes"] == (256 if chunk else -(-n_mid // 256) * 256)
    assert lanes[0] >= root["scratch_lanes"] and lanes[0] % 256 == 0 and lanes[0] <= L.SEARCH_CHUNK
    if not chunk:                                       # one MID search of all the mid lanes
        mid = [_plan(R.MID, 2, float("inf"), h=(t, 0, 0)) for t in (l3 // 21, l3 // 21 + n_mid)]
        assert max(root["scratch_lanes"], mid[0]["scratch_lanes"]) <= lanes[0] <= max(root["scratch_lanes"], mid[1]["scratch_lanes"])
    assert env.stats()["error_flags"] == 0
    env.close()


def test_analysis(bg):
    """... and an analysis leaves no step behind: search_read and search_info refuse, before it as after it"""
    env = _fresh(bg)
    out = env.analyze_moves(env.states(), top_k=5)
    p = _plan(R.ANALYSIS, 5)
    assert p["n_cand"] == N * 6 and env.scratch_info() == [p["scratch_lanes"], 0, 0]
    assert int((out["status"] == 3).sum()) > 0          # (a board is no afterstate of its own: the search ran all the same)
    for read in (env.search_info, env.search_candidates):
        with pytest.raises(bg.BgamdError) as e:
            read()
        assert e.value.code == R.E_INVALID
    env.step_search(top_k=2, auto_reset=False)
    assert 0 < env.search_info()[0] <= N
    env.analyze_moves(env.states(), top_k=0)
    for read in (env.search_info, env.search_candidates):
        with pytest.raises(bg.BgamdError) as e:
            read()
        assert e.value.code == R.E_INVALID
    assert env.stats()["error_flags"] == 0
    env.close()
