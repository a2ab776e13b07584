"""CPU conditions of the filtered-search tests on the MI355X (tests/test_gpu_search_filter.py): the exact model of the move filter
(tests/filter_model.py) agrees with a plain-Python restatement of the header's sentence, three deliberately wrong models are told from
it on the lane set, and under the dyadic table (nets.dyadic_table) the 1 500 G10 boards hold every class of lane the GPU test names --
for the margins it uses: 0, the two margins that candidates sit on exactly, a mid margin and +inf."""
import numpy as np
import pytest

import filter_model as F
import search_lanes as L
import search_model as M

KS = (1, 3, 0)
MID = 0.004
INF = float("inf")


@pytest.fixture(scope="module")
def lanes():
    """-> (reference values of every board's afterstates under the dyadic table, movers, terminal flags)"""
    tu = L.g10()[1]
    vals = L.np32_values(L.dyadic(), range(len(tu)))
    term = [L.terminal(L.afterstates(i), tu[i]) for i in range(len(tu))]
    return vals, tu, term


@pytest.fixture(scope="module")
def margins(lanes):
    vals, tu, _ = lanes
    return [0.0] + F.equality_margins(vals, tu) + [MID, INF]


def test_equality_margins_are_met_exactly(lanes, margins):
    vals, tu, _ = lanes
    a, b = margins[1:3]
    assert 0 < b < a < MID and np.float32(a) == a and np.float32(b) == b
    for mg in (a, b):
        hits = sum(bool((F.margin_distances(np.arange(len(v)), v, m, 0)[1] == np.float32(mg)).any()) for v, m in zip(vals, tu) if len(v))
        assert hits >= 40, (mg, hits)


def test_model_against_the_plain_restatement(lanes, margins):
    vals, tu, _ = lanes
    n = 0
    for i in range(0, len(tu), 3):
        v = vals[i]
        if not 1 <= len(v) <= 60:
            continue
        idx = np.random.RandomState(i).permutation(len(v))                 # the model must not depend on the order the rows come in
        for K in KS + (2, 5):
            for mg in margins:
                want = F.select_plain(idx, v[idx], tu[i], K, mg)
                assert np.array_equal(F.select(idx, v[idx], tu[i], K, mg), want), (i, K, mg)
                assert np.array_equal(F.select(np.arange(len(v)), v, tu[i], K, mg), want), (i, K, mg)
                n += 1
    assert n > 5000


def test_margin_inf_is_the_unfiltered_selection(lanes):
    vals, tu, _ = lanes
    for i in range(len(tu)):
        for K in KS:
            assert np.array_equal(F.select(np.arange(len(vals[i])), vals[i], tu[i], K, INF), M.select(np.arange(len(vals[i])), vals[i], tu[i], K))


def test_kept_set_is_a_prefix_and_rank_0_stays(lanes, margins):
    vals, tu, _ = lanes
    for i in range(len(tu)):
        m = len(vals[i])
        if m == 0:
            continue
        full = M.select(np.arange(m), vals[i], tu[i], 0)
        for mg in margins:
            kept = F.select(np.arange(m), vals[i], tu[i], 0, mg)
            assert 1 <= len(kept) <= m and np.array_equal(kept, full[:len(kept)]), (i, mg)


@pytest.mark.parametrize("name", sorted(F.WRONG))
def test_wrong_models_are_told_apart(lanes, margins, name):
    vals, tu, _ = lanes
    wrong = F.WRONG[name]
    differ = 0
    for i in range(len(tu)):
        m = len(vals[i])
        differ += any(not np.array_equal(wrong(np.arange(m), vals[i], tu[i], K, mg), F.select(np.arange(m), vals[i], tu[i], K, mg))
                      for K in KS for mg in margins)
    print("wrong model %-16s differs on %d of %d lanes" % (name, differ, len(tu)))
    assert differ >= 40, (name, differ)


def test_strict_model_differs_only_at_equality(lanes, margins):
    """... and the equality margins are what tells `<` from `<=`: at the mid margin no candidate sits on the margin and the two agree"""
    vals, tu, _ = lanes
    for i in range(len(tu)):
        m = len(vals[i])
        assert np.array_equal(F.select_strict(np.arange(m), vals[i], tu[i], 0, MID), F.select(np.arange(m), vals[i], tu[i], 0, MID))


def test_census_of_the_lane_classes(lanes, margins):
    vals, tu, term = lanes
    total = dict(cut=0, at_margin=0, made_single=0)
    for K in KS:
        for mg in margins:
            c = F.census(vals, tu, term, K, mg)
            print("census top_k %d margin %-22r %s" % (K, mg, c))
            assert c["lanes"] == 1453 and c["forced"] >= 300 and c["terminal"] >= 40, c
            if K == 1 or mg == INF:
                assert c["cut"] == 0 and c["made_single"] == 0, c          # nothing for the margin to do
            elif mg < MID:                                                 # 0 and the equality margins: every class, at either width
                assert c["cut"] >= 40 and c["made_single"] >= 40, c
                assert (c["at_margin"] >= 10) == (mg > 0), c
            else:
                assert c["cut"] >= 40 and c["made_single"] >= 40 and c["at_margin"] == 0, c
            for k in total:
                total[k] += c[k]
    assert all(total.values())
