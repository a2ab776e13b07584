"""CPU conditions of the search-log tests on the MI355X (tests/test_gpu_search_log.py): the exact model of a log entry
(tests/search_log_model.py) agrees with a plain-Python restatement of the header's sentences on every G10 lane, three deliberately wrong
models are told from it, the library exports the call, and the G10 boards hold the lane classes the GPU tests rest on -- lanes without
a move, lanes with one afterstate, lanes with a terminal candidate, both movers, doubles -- already among the first 63."""
import ctypes
import os

import numpy as np
import pytest

import filter_model as F
import search_lanes as L
import search_log_model as G
import search_model as M

INF = float("inf")
# (filtered, top_k, margin): the plain step at top_k 1, 3, 0 and the filtered step at top_k 3 with the margins 0, 0.02, +inf
STEPS = [(False, 1, None), (False, 3, None), (False, 0, None), (True, 3, 0.0), (True, 3, 0.02), (True, 3, INF)]


@pytest.fixture(scope="module")
def lanes():
    """per G10 board: (afterstates, v1 under the dyadic table, terminal flags, a V2 for every afterstate).  The V2 are made up -- eighths in
    [0, 1], so that they tie often and the smaller index has to decide; a terminal candidate's is its outcome -- the model is about the
    rule, not the net."""
    st, tu, dice = L.g10()
    v1 = L.np32_values(L.dyadic(), range(len(tu)))
    out = []
    for i in range(len(tu)):
        c = L.afterstates(i)
        term = L.terminal(c, tu[i]) if len(c) else np.zeros(0, bool)
        v2 = (np.random.RandomState(i).randint(0, 9, len(c)) / 8.0).astype(np.float32)
        v2[term] = v1[i][term]
        out.append((c, v1[i], term, v2))
    return out


def _kept(lane, mover, filtered, top_k, margin):
    c, v1, term, v2 = lane
    idx = np.arange(len(c))
    return F.select(idx, v1, mover, top_k, margin) if filtered else M.select(idx, v1, mover, top_k)


def _entries(fn, lanes, i, only=None, **kw):
    st, tu, _ = L.g10()
    c, v1, term, v2 = lanes[i]
    part = only is None or int(tu[i]) == only
    for filtered, top_k, margin in STEPS:
        kept = _kept(lanes[i], tu[i], filtered, top_k, margin)
        v2k = M.bits(v2[kept]).astype(np.uint32)
        if filtered and len(kept) == 1:                    # the device reports v2 = v1 for a singleton; the log does not use it
            v2k = M.bits(v1[kept]).astype(np.uint32)
        yield fn(st[i], tu[i], part, kept, c[kept], M.bits(v1[kept]).astype(np.uint32), v2k, term[kept], filtered, **kw)


def test_model_against_the_plain_restatement(lanes):
    n = nothing = nan = 0
    for i in range(len(lanes)):
        for only in (None, 0, 1):
            for a, b in zip(_entries(G.entry, lanes, i, only), _entries(G.entry_plain, lanes, i, only)):
                assert G.same(a, b), (i, only)
                n += 1
                nothing += a is None
                nan += a is not None and int(a["target"]) == G.QNAN
    assert n == 1500 * 3 * len(STEPS) and nothing > 8000 and nan > 1000


def test_the_entry_s_fields(lanes):
    """what the header says of each field, on every lane: the turn bits, the played state, where the NaNs are"""
    st, tu, _ = L.g10()
    for i in range(len(lanes)):
        c, v1, term, v2 = lanes[i]
        for (filtered, top_k, margin), e in zip(STEPS, _entries(G.entry, lanes, i)):
            kept = _kept(lanes[i], tu[i], filtered, top_k, margin)
            assert bool(e["rows"][0] >> 31) == bool(tu[i]) and bool(e["after"][0] >> 31) != bool(tu[i])
            assert np.array_equal(e["rows"], G.pack_row(st[i], tu[i]))
            if len(kept) == 0:
                assert np.array_equal(e["after"][1:], e["rows"][1:]) and (e["after"][0] ^ e["rows"][0]) == G.TURN_BIT
                assert int(e["target"]) == int(e["v1"]) == G.QNAN
                continue
            j = kept[M.choose(kept, v2[kept] if not (filtered and len(kept) == 1) else v1[kept], tu[i])]
            assert np.array_equal(e["after"], G.pack_row(c[j], 1 - tu[i]))
            assert int(e["v1"]) == int(M.bits(v1[j:j + 1])[0])
            if filtered and len(kept) == 1:
                assert int(e["target"]) == G.QNAN
            else:
                assert int(e["target"]) == int(M.bits(v2[j:j + 1])[0])


@pytest.mark.parametrize("name", sorted(G.WRONG))
def test_wrong_models_are_told_apart(lanes, name):
    differ = 0
    for i in range(len(lanes)):
        only = None if name != "idle_lanes_log" else 0
        differ += any(not G.same(a, b) for a, b in zip(_entries(G.entry, lanes, i, only), _entries(G.entry, lanes, i, only, **G.WRONG[name])))
    print("wrong model %-24s differs on %d of %d lanes" % (name, differ, len(lanes)))
    assert differ >= 300, (name, differ)


def test_census_of_the_lane_classes():
    """the classes the GPU tests rest on, by the oracle's afterstates: (lanes without a move, lanes with one afterstate, lanes with a terminal
    candidate) among the first 63 boards -- the smallest lane count above 1 -- and over all 1 500"""
    st, tu, dice = L.g10()

    def census(n):
        m = L.counts(n)
        term = sum(bool(L.terminal(L.afterstates(i), tu[i]).any()) for i in range(n) if m[i])
        return int((m == 0).sum()), int((m == 1).sum()), term
    assert census(63) == (2, 15, 4)
    assert census(1500) == (47, 363, 75)
    assert set(tu[:63].tolist()) == {0, 1} and set(tu.tolist()) == {0, 1}
    assert int((dice[:, 0] == dice[:, 1]).sum()) == 456 and (dice[:63, 0] == dice[:63, 1]).any()


def test_the_call_is_exported_and_bound():
    """without the feature: no such symbol, no such method"""
    import __graft_entry__ as g
    g.build()
    import backgammon_env as bg
    from backgammon_env import _capi, learner
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "bgamd_env_set_search_log")
    assert "bgamd_env_set_search_log" in {n for n, _, _ in _capi.SYMBOLS}
    assert lib.bgamd_env_set_search_log(None, None, None, None, None, ctypes.c_int64(0)) == -1          # a NULL env
    assert callable(bg.VecGame.record_search_log) and callable(learner.play_round_search)
    assert callable(learner.DeviceTDLambdaLearner.fit_rows) and callable(learner.DeviceTDLambdaLearner.fit_search)
    hdr = open(os.path.join(os.path.dirname(_capi.LIB_PATH), "..", "include", "bgamd.h")).read()
    assert "bgamd_env_set_search_log(bgamd_env *env, void *d_rows, void *d_after, float *d_target, float *d_v1, int64_t max_plies)" in hdr
