"""CPU side of the many-nets tests (tests/nets.py): every table is inside bgamd_weights_check's accepted domain, the condition the flat
1e-5 parity bound rests on holds for each parity family on the rows the GPU tests use, the references break ties by index, and the
feature sweep covers every feature value and every delta entry."""
import ctypes

import numpy as np
import pytest

import nets as N
import rollout_ref as R
import rollout_vr_ref as V
import search_ref as S
from oracle import oracle as O


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from backgammon_env import _capi
    return _capi.load()


def _chk(lib, w):
    w = np.ascontiguousarray(w, dtype=np.float32)
    return lib.bgamd_weights_check(w.ctypes.data_as(ctypes.c_void_p))


def test_tables_are_seeded_and_distinct():
    for name in N.NAMES:
        w = N.table(name)
        assert w.dtype == np.float32 and w.shape == (25601,) and np.isfinite(w).all(), name
        assert np.array_equal(w, N._MAKERS[name](np.random.RandomState(N.SEED), N.checkpoint()).astype(np.float32)), name
    assert len({N.table(n).tobytes() for n in N.NAMES}) == len(N.NAMES)
    assert np.array_equal(N.table("ckpt"), N.checkpoint())
    z = N.table("zero_w1")
    assert not z[:N.O1].any() and np.array_equal(z[N.O1:], N.table("normal")[N.O1:])
    lu = np.abs(N.table("loguniform")[:N.O1])
    assert lu.min() >= 0.99e-7 and lu.max() <= 8.0 and (lu < 2.0 ** -14).mean() > 0.3       # f16 hi subnormal for a third of W1
    assert np.abs(N.table("xavier")[:N.O1]).max() <= 0.1 * np.sqrt(6 / 326) and not N.table("xavier")[N.O1:N.O2].any()


def test_weights_check_accepts_every_table(lib):
    for name in N.NAMES:
        assert _chk(lib, N.table(name)) == 0, name
    bad = N.table("ckpt").copy()
    bad[198 * 7 + 40] = 65504.0                            # |w| < 65504 is the domain: the bound itself is outside
    assert _chk(lib, bad) == -8
    assert b"65504" in lib.bgamd_error_string(-8)


@pytest.mark.parametrize("family", N.PARITY)
def test_fp32_forward_is_within_a_quarter_of_the_parity_bound(family):
    """The condition the flat 1e-5 bound rests on, not a measurement: on every row the GPU tests evaluate, the plain numpy fp32
    forward pass is within 2.5e-6 of the oracle's fp64 one -- the reference's own rounding stays under a quarter of the bound.  A family
    that breaks this is replaced, never given a wider bound."""
    w = N.table(family)
    sets = {"dense": N.encode(*N.value_rows())}
    for k, (roots, rt, rows, ri) in N.pair_sets().items():
        sets[k] = N.encode(rows, rt[ri])
    for k, X in sets.items():
        e = float(np.abs(N.forward_np32(w, X).astype(np.float64) - O.forward_f64(w, X)).max())
        print("%s, %s (%d rows): max |numpy fp32 - fp64| = %.3g" % (family, k, len(X), e))
        assert e <= 2.5e-6, (family, k, e)


def test_reference_tables_of_the_exact_output_nets_are_exact_in_fp64():
    """out_lo's references play b2 = -800 instead of -200 (tests/nets.py, reference_table): under it the fp64 forward pass is exactly
    0.0 on the rows used, as out_hi's own table gives exactly 1.0 -- and only b2 differs from the table the GPU is given."""
    X = N.encode(*N.value_rows())
    assert (O.forward_f64(N.reference_table("out_hi"), X) == 1.0).all() and N.reference_table("out_hi") is N.table("out_hi")
    lo = N.reference_table("out_lo")
    assert (O.forward_f64(lo, X) == 0.0).all()
    assert np.array_equal(lo[:N.O3], N.table("out_lo")[:N.O3]) and lo[N.O3] == -800.0 and N.table("out_lo")[N.O3] == -200.0
    assert len(np.unique(O.forward_f64(N.table("out_lo"), X))) > 1          # why: ~1e-90 apart, not equal


# ---- the references break ties by index ------------------------------------------------------------------------------------------------

def _g10(n, step):
    g10 = np.load(N.GOLDEN + "/g10_arbitrary_boards.npz")
    idx = np.arange(n) * step
    return g10["boards"][idx].astype(np.int32), g10["dice"][idx].astype(np.int32)


def test_search_reference_keeps_the_first_k_in_reference_order():
    w = N.table("zero_w1")
    c = N.constant_value(w)
    st, dice = _g10(12, 61)
    n_full = 0
    with N.memoized(S, "reply_values"):                      # (K = 3 and 1 meet the candidates of K = 8 again)
        for s, (mover, d1, d2) in zip(st, dice):
            cand = S.distinct_afterstates(s, int(mover), int(d1), int(d2))
            if len(cand) == 0 or any(S.outcome(x, int(mover)) is not None for x in cand):
                continue
            for K in (8, 3, 1):
                r = S.search(w, s, int(mover), int(d1), int(d2), K)
                k = min(K, len(cand)) if K else len(cand)
                assert np.array_equal(r["keys"], np.arange(k)) and np.array_equal(r["states"], cand[:k])
                assert r["choice"] == 0
                assert (r["v1"] == S.net(w, s, 0)[0]).all() and np.abs(r["v2"] - c).max() < 1e-12
                n_full += K == 8 and len(cand) > 8
    assert n_full >= 3


def test_rollout_references_flag_no_near_tie_when_every_value_is_equal():
    w = N.table("zero_w1")
    st, dice = _g10(4, 301)
    r = R.rollout(w, st, dice[:, 0], 12, 99, max_plies=6, rotate=True)
    assert not r["near_tie"].any() and r["truncated"].any()
    v = V.rollout(w, st[:2], dice[:2, 0], 4, 99, max_plies=4, rotate=True)
    assert not v["near_tie"].any()


# ---- the feature sweep ---------------------------------------------------------------------------------------------------------------

def _feature_values(f):
    if f < 192:
        return {0.0, 1.0} if f % 4 < 3 else {0.0} | {np.float32((c - 3) / 2.0) for c in range(4, 16)}
    if f < 194:
        return {0.0, 1.0}
    return {np.float32(c / 2.0) for c in range(16)} if f < 196 else {np.float32(c / 15.0) for c in range(16)}


def test_sweep_rows_produce_every_value_of_every_feature():
    st, tu = N.sweep_rows()
    assert (np.abs(st[:, :24]) <= 15).all() and (st[:, 24:] >= 0).all() and (st[:, 24:] <= 15).all()
    X = N.encode(st, tu)
    for f in range(198):
        assert {np.float32(v) for v in np.unique(X[:, f])} == {np.float32(v) for v in _feature_values(f)}, f


def test_sweep_pairs_hold_every_delta_entry_with_both_signs():
    roots, rt, rows, ri = N.sweep_pairs()
    assert (np.abs(rows[:, :24]) <= 15).all() and (rows[:, 24:] >= 0).all() and (rows[:, 24:] <= 15).all()
    D = N.encode(rows, rt[ri]).astype(np.float64) - N.encode(roots, rt)[ri]
    assert (D != 0).sum(1).max() <= 16                       # inside the incremental evaluator's list
    assert not D[:, 192:194].any()                           # a row carries its root's turn bit: never a delta entry
    for tb in (0, 1):                                        # ... and the list builder starts with the mover's side: both orders
        Dt = D[rt[ri] == tb]
        for f in list(range(192)) + [194, 195, 196, 197]:
            vals = sorted(_feature_values(f) - {0.0})
            want = {int(round(30 * (a - b))) for a in [0.0] + vals for b in [0.0] + vals} - {0}
            got = {int(round(30 * v)) for v in np.unique(Dt[:, f])} - {0}
            assert got == want, (tb, f)                      # every multiplier the entry can take, + and -
