"""CPU conditions of the search-rule tests on the MI355X (tests/test_gpu_search_rules.py): the exact model of the search's selection,
V2 and choice (tests/search_model.py) agrees with the fp64 reference (tests/search_ref.py) wherever fp32 and fp64 can agree, three
deliberately wrong models do not, the dyadic table (nets.dyadic_table) produces the exact ties the GPU tests need, and the lane sets
have the shapes those tests name: two and four scoring passes, a candidate whose rolls straddle a pass, boards with more than 64 and
more than 128 distinct afterstates, terminal candidates and lanes without a move."""
import numpy as np
import pytest

import nets as N
import search_lanes as L
import search_model as M
import search_ref as S

KS = (0, 3, 8)
NEAR = 2e-5


@pytest.fixture(scope="module")
def reference_lanes():
    """40 G10 lanes (of every sixth board those with 2 to 40 candidates: the first 20 of each mover) under the dyadic table: per K the
    fp64 reference's result"""
    st, tu, dice = L.g10()
    some = [i for i in range(0, 1500, 6) if 2 <= len(L.afterstates(i)) <= 40]
    lanes = sorted([i for i in some if tu[i] == 0][:20] + [i for i in some if tu[i] == 1][:20])
    w = L.dyadic()
    with N.memoized(S, "reply_values"):
        refs = {(i, K): S.search(w, st[i], int(tu[i]), int(dice[i, 0]), int(dice[i, 1]), K) for i in lanes for K in KS}
    return lanes, refs


def _near(x):
    """two UNEQUAL values within NEAR of each other: fp32 and fp64 may order them differently"""
    s = np.sort(np.unique(np.asarray(x, np.float64)))
    return bool((np.diff(s) <= NEAR).any())


def _full_v1(refs, i):
    """the reference's v1 of every distinct afterstate of lane i in reference order, as float32"""
    r = refs[(i, 0)]
    v = np.empty(len(r["keys"]), np.float32)
    v[r["keys"]] = r["v1"].astype(np.float32)
    return v


def _model(refs, i, K, mover, select=M.select, choose=M.choose):
    r = refs[(i, K)]
    v1 = _full_v1(refs, i)
    kept = select(np.arange(len(v1)), v1, mover, K)
    v2 = dict(zip(r["keys"].tolist(), r["v2"].astype(np.float32)))
    if any(int(k) not in v2 for k in kept):
        return kept, None
    return kept, choose(kept, np.array([v2[int(k)] for k in kept], np.float32), mover)


def test_model_against_the_fp64_reference(reference_lanes):
    lanes, refs = reference_lanes
    tu = L.g10()[1]
    assert len(lanes) >= 36
    left_out = 0
    for i in lanes:
        if _near(refs[(i, 0)]["v1"]) or any(_near(refs[(i, K)]["v2"]) for K in KS):
            left_out += 1
            continue
        for K in KS:
            r = refs[(i, K)]
            kept, choice = _model(refs, i, K, int(tu[i]))
            assert np.array_equal(kept, r["keys"]), (i, K)
            assert choice == r["choice"], (i, K)
    assert left_out <= 0.2 * len(lanes), (left_out, len(lanes))


def test_dyadic_table_is_what_it_says():
    w = L.dyadic()
    W1 = w[:N.O1].reshape(N.N_HID, N.N_IN)
    cols = np.where((W1 != 0).any(0))[0]
    assert len(cols) <= 16 and (cols < 192).all() and len(cols) >= 15
    for part in (W1, w[N.O1:N.O2]):
        k = part.astype(np.float64) * 16
        assert (k == np.round(k)).all() and np.abs(k).max() <= 8
    assert w[N.O3] == 0 and np.abs(w[N.O2:N.O3]).max() > 0
    assert not w.flags.writeable and N.dyadic_table(L.DYADIC_SEED) is w
    assert not np.array_equal(N.dyadic_table(L.DYADIC_SEED + 1), w)
    # the features of the chosen columns are multiples of 1/2 on every G10 afterstate: the pre-activations are exact
    st, tu, _ = L.g10()
    X = np.concatenate([N.encode(L.afterstates(i), np.full(len(L.afterstates(i)), tu[i])) for i in range(0, 1500, 6) if len(L.afterstates(i))])
    assert (X[:, cols] * 2 == np.round(X[:, cols] * 2)).all()
    pre64 = X.astype(np.float64) @ W1.astype(np.float64).T + w[N.O1:N.O2]
    pre32 = X @ W1.T + w[N.O1:N.O2]
    assert np.array_equal(pre32.astype(np.float64), pre64)
    assert "dyadic" not in N.NAMES


def test_tie_census_under_the_dyadic_table():
    tu = L.g10()[1]
    idx = range(0, 1500, 6)
    c = L.census(L.np32_values(L.dyadic(), idx), [tu[i] for i in idx])
    print("tie census, dyadic table, numpy fp32 forward, every sixth G10 board:", c)
    assert c["lanes"] == 181
    assert c["across3"] >= 60 and c["across8"] >= 40, c


# ---- three wrong models: each must be told apart from the reference ------------------------------------------------------------------

def _select_larger_index(order_index, v1, mover, top_k):
    idx = np.asarray(order_index, np.int64)
    b = M.bits(v1)
    kept = idx[np.lexsort((-idx, -b if mover == 0 else b))]
    return kept[:top_k] if top_k else kept


def _choose_larger_index(kept, v2, mover):
    b = M.bits(v2)
    return int(np.lexsort((-np.asarray(kept, np.int64), -b if mover == 0 else b))[0])


def _disagreeing_lanes(reference_lanes, model_of):
    lanes, refs = reference_lanes
    tu = L.g10()[1]
    bad = 0
    for i in lanes:
        differs = False
        for K in KS:
            r = refs[(i, K)]
            kept, choice = model_of(refs, i, K, int(tu[i]))
            differs |= not np.array_equal(kept, r["keys"]) or choice != r["choice"]
        bad += differs
    return bad


def test_wrong_model_ties_to_the_larger_index(reference_lanes):
    n = _disagreeing_lanes(reference_lanes, lambda refs, i, K, mover: _model(refs, i, K, mover, _select_larger_index, _choose_larger_index))
    assert n >= 10, n


def test_wrong_model_player2_ranked_like_player1(reference_lanes):
    n = _disagreeing_lanes(reference_lanes, lambda refs, i, K, mover: _model(refs, i, K, 0))
    assert n >= 10, n


def test_wrong_model_copies_kept(reference_lanes):
    """every sequence's afterstate is a candidate of its own: a copy takes a place among the top K"""
    st, tu, dice = L.g10()

    def model_of(refs, i, K, mover):
        _, _, raw = S.O.evaluate_turn_sequences(S.O.State.from28(st[i], mover), mover, int(dice[i, 0]), int(dice[i, 1]))
        index = L.index_of(L.afterstates(i))
        of_row = np.array([index[np.ascontiguousarray(s, dtype=np.int32).tobytes()] for s in raw])
        kept_rows = M.select(np.arange(len(raw)), _full_v1(refs, i)[of_row], mover, K)
        return of_row[kept_rows], None
    assert _disagreeing_lanes(reference_lanes, model_of) >= 10


# ---- the lane sets of the GPU tests -----------------------------------------------------------------------------------------------------

def test_lane_sets():
    c = L.counts()
    tu = L.g10()[1]
    cum = np.concatenate([[0], np.cumsum(c)])
    # 512 boards at full width: two scoring passes, and candidate 6241's rolls 0..10 are in the first, 11..20 in the second
    assert cum[512] == 6515 and cum[512] * 21 == 136815 and L.SEARCH_CHUNK < 136815 <= 2 * L.SEARCH_CHUNK
    assert L.SEARCH_CHUNK == 21 * 6241 + 11
    lane = int(np.searchsorted(cum, 6241, side="right")) - 1
    assert lane == 494 and c[lane] == 6
    # all 1 500: four passes; the three boundaries fall inside lanes that keep at least two candidates
    assert cum[1500] == 20182 and 3 * L.SEARCH_CHUNK < cum[1500] * 21 <= 4 * L.SEARCH_CHUNK
    for p in (1, 2, 3):
        j = L.SEARCH_CHUNK * p // 21
        assert (L.SEARCH_CHUNK * p) % 21 != 0                          # the boundary splits candidate j's rolls
        assert c[int(np.searchsorted(cum, j, side="right")) - 1] >= 2
    # six envs of at most 256 lanes: one pass each
    for k in range(0, 1500, 256):
        assert c[k:k + 256].sum() * 21 <= L.SEARCH_CHUNK
    # more than one round of srch_select_kernel's 64-row walk, and more than two; the largest board
    assert (c > 64).sum() >= 40 and (c > 128).sum() >= 20 and c.max() == 381
    assert (c[:512] > 64).sum() >= 10 and (c[:512] > 128).sum() >= 1
    n_term = sum(bool(L.terminal(L.afterstates(i), tu[i]).any()) for i in range(1500) if c[i])
    assert n_term >= 40 and (c == 0).sum() >= 40, (n_term, (c == 0).sum())
    # the first 256 boards hold copies among their sequences (want_index: count is the sequences', not the distinct afterstates')
    st, _, dice = L.g10()
    n_copies = 0
    for i in range(256):
        _, _, raw = S.O.evaluate_turn_sequences(S.O.State.from28(st[i], int(tu[i])), int(tu[i]), int(dice[i, 0]), int(dice[i, 1]))
        n_copies += len(raw) > c[i]
    assert n_copies >= 100, n_copies


def test_v2_from_replies():
    one = np.ones(21, np.float32)
    assert M.v2_from_replies(one) == np.float32(1.0) and M.v2_from_replies(0 * one) == np.float32(0.0)
    f = np.random.RandomState(5).random_sample((20000, 21)).astype(np.float32)
    f[:100] = np.float32(1) - f[:100] * np.float32(1e-7)               # just below 1.0
    v = M.v2_from_replies(f)
    assert v.dtype == np.float32 and (v >= 0).all() and (v <= 1).all()
    # against the weighted fp64 mean: 21 additions, one scaling and one product, each rounded once (values <= 36: ulp 4e-6 at most)
    w = np.where(M.DOUBLES, 1.0, 2.0) / 36.0
    assert np.abs(v - f.astype(np.float64) @ w).max() <= 1e-6
    # batched and one at a time agree
    assert np.array_equal(v[:50], np.array([M.v2_from_replies(x) for x in f[:50]]))
