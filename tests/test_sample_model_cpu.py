"""The sampled step's exact model (tests/sample_model.py) on the CPU: against a plain-Python restatement on every lane of the lane set, as
a sampler of softmax(a / T) over DISTINCT afterstates (chi-square, 200 000 draws), against three deliberately wrong models that must fail
on the same data, and the census of near ties that tests/test_gpu_sampled.py's comparison with the device rests on."""
import math

import numpy as np
import pytest

import nets as N
import sample_model as SM
import search_lanes as L

DRAWS = 200_000
GID = 46
# the 0.999 quantile of chi-square with df degrees of freedom (the seed is fixed: a correct sampler passes or fails once and for all; a
# wrong one misses by orders of magnitude)
CHI2_999 = {5: 20.515, 6: 22.458, 7: 24.322, 8: 26.124, 9: 27.877, 10: 29.588, 11: 31.264}


@pytest.fixture(scope="module")
def ckpt():
    return N.checkpoint()


_ks = {}


def _lane_ks(i):
    """the integers of u of every candidate of lane i (game id i, ply 0, the env's seed), through oracle.philox, once"""
    if i not in _ks:
        rows = SM.planes(SM.candidates(i)[0])
        _ks[i] = (rows, np.array([SM.uniform_int(SM.SEED, i, 0, r) for r in rows], np.int64))
    return _ks[i]


def _plain(rows, values, mover, seed, gid, ply, T):
    """the rule of include/bgamd.h once more, row by row in plain Python (keys = positions) -> (winner, scores)"""
    from oracle import oracle as O
    a = [np.float32(v) if mover == 0 else np.float32(-np.float32(v)) for v in values]
    best = max(a)
    scores = []
    for r, ai in zip(rows, a):
        r = [int(x) for x in r]
        A = O.philox(r[0], r[1], r[2], r[3], seed & 0xFFFFFFFF, seed >> 32)
        B = O.philox(r[4] ^ A[0], r[5] ^ A[1], r[6] ^ A[2], r[7] ^ A[3], seed & 0xFFFFFFFF, seed >> 32)
        c = O.philox(gid & 0xFFFFFFFF, gid >> 32, ply, 2, B[0], B[1])
        u = (2 * (c[0] >> 9) + 1) / 2.0 ** 24
        with np.errstate(over="ignore", under="ignore"):
            q = float(np.float32(ai - best) / np.float32(T))
        scores.append(q - math.log(-math.log(u)))
    w = 0
    for k in range(1, len(scores)):
        if scores[k] > scores[w]:                        # (a later row wins only when strictly better: the smallest key on ties)
            w = k
    return w, scores


def test_planes_are_the_library_layout():
    st = np.zeros((2, 28), np.int32)
    st[0, [0, 11, 16, 18]] = [2, 5, 3, 5]; st[0, [5, 7, 12, 23]] = [-5, -3, -5, -2]          # the start position
    st[1, 0] = 15; st[1, 24], st[1, 25], st[1, 26], st[1, 27] = 1, 2, 4, 8
    p = SM.planes(st)
    # csrc/bg_board.h start_planes(): P1 2 on pt 1, 5 on 12, 3 on 17, 5 on 19; P2 5 on 6, 3 on 8, 5 on 13, 2 on 24
    assert p[0].tolist() == [(1 << 12) | (1 << 17) | (1 << 19), (1 << 1) | (1 << 17), (1 << 12) | (1 << 19), 0,
                             (1 << 6) | (1 << 8) | (1 << 13), (1 << 8) | (1 << 24), (1 << 6) | (1 << 13), 0]
    assert p[1].tolist() == [3, 2, 2 | (1 << 25), 2, 0, 1 << 25, 0, 1]


def test_model_against_plain_python_on_every_lane(ckpt):
    st, tu, dice = SM.lane_set()
    seen = 0
    for i in range(len(st)):
        cand = SM.candidates(i)[0]
        if len(cand) == 0:
            continue
        rows, ks = _lane_ks(i)
        v = SM.oracle_values(ckpt, i)
        for T in (0.05, 1e-30):
            m = SM.lane(rows, np.arange(len(rows)), v, tu[i], SM.SEED, i, 0, T)
            w, s = _plain(rows, v, int(tu[i]), SM.SEED, i, 0, T)
            assert m["winner"] == w, (i, T)
            s, fin = np.asarray(s), np.isfinite(m["s"])                       # the same fp64 numbers up to the two libraries' log, -inf alike
            assert np.array_equal(np.isfinite(s), fin) and np.array_equal(s[~fin], m["s"][~fin]), (i, T)
            assert np.allclose(s[fin], m["s"][fin], rtol=1e-14, atol=1e-14), (i, T)
            assert np.array_equal(m["k"], ks) and ((ks > 0) & (ks < 2 ** 24) & (ks % 2 == 1)).all()
        seen += 1
    assert seen >= 950


# ---- it samples softmax over distinct afterstates --------------------------------------------------------------------------------------------

def _chi_lane(ckpt):
    """the first lane with a twin pair, PLAYER2 to move and 6 to 12 distinct afterstates -> (rows, values, group of every row, mass)"""
    st, tu, dice = SM.lane_set()
    i = next(i for i in range(len(st)) if tu[i] == 1 and SM.twin_pair(i) and 6 <= len(np.unique(SM.candidates(i)[0], axis=0)) <= 12)
    assert i == GID
    cand = SM.candidates(i)[0]
    _, first, group = np.unique(cand, axis=0, return_index=True, return_inverse=True)
    group = np.asarray(group).ravel()
    assert len(cand) > len(first)                                              # the twin pair: more rows than afterstates
    return SM.planes(cand), SM.oracle_values(ckpt, i), group, first


def _softmax(values, first, T):
    a = -np.asarray(values, np.float64)[first]                                 # PLAYER2: the mover-side value is -v
    p = np.exp((a - a.max()) / T)
    return p / p.sum()


def _chi2(winners, group, p):
    obs = np.bincount(group[winners], minlength=len(p)).astype(np.float64)
    exp = p * len(winners)
    assert exp.min() >= 50                                                     # every cell well filled
    return float(((obs - exp) ** 2 / exp).sum())


_draws = {}


def _ks_of_draws(rows, keyed_by_key=False):
    if keyed_by_key not in _draws:
        r = rows
        if keyed_by_key:                                                       # the wrong model: a row's noise from its KEY (its position)
            r = np.zeros_like(rows); r[:, 0] = np.arange(len(rows))
        _draws[keyed_by_key] = SM.uniform_ints_np(SM.SEED, GID, np.arange(DRAWS), r)
    return _draws[keyed_by_key]


def _winners(ks, values, T, **wrong):
    s = SM.quotient(values, 1, T, **wrong).astype(np.float64)[None, :] + SM.gumbel(ks)
    return np.argmax(s, axis=1)                                                # (the first of equal scores: the smallest key)


def test_array_philox_is_the_oracles(ckpt):
    rows = _chi_lane(ckpt)[0]
    ks = _ks_of_draws(rows)
    for ply in (0, 1, 77, DRAWS - 1):
        assert [SM.uniform_int(SM.SEED, GID, ply, r) for r in rows] == ks[ply].tolist()
    kk = _ks_of_draws(rows, True)
    assert [SM.uniform_int(SM.SEED, GID, 5, r, by_key=j) for j, r in enumerate(rows)] == kk[5].tolist()


@pytest.mark.parametrize("T", [0.05, 1.0])
def test_samples_softmax_over_distinct_afterstates(ckpt, T):
    rows, v, group, first = _chi_lane(ckpt)
    ks = _ks_of_draws(rows)
    for k in range(len(first)):                                                # copies of one afterstate draw one u
        cols = np.where(group == k)[0]
        assert (ks[:, cols] == ks[:, cols[:1]]).all()
    w = _winners(ks, v, T)
    # of the copies of an afterstate only the first (the smallest key) is ever played
    assert np.isin(w, first).all()
    chi2 = _chi2(w, group, _softmax(v, first, T))
    print("T", T, "chi2", chi2, "df", len(first) - 1)
    assert chi2 < CHI2_999[len(first) - 1]


@pytest.mark.parametrize("wrong", ["noise_by_key", "no_flip", "no_divide"])
def test_wrong_models_fail(ckpt, wrong):
    T = 0.05
    rows, v, group, first = _chi_lane(ckpt)
    ks = _ks_of_draws(rows, wrong == "noise_by_key")
    w = _winners(ks, v, T, **({"flip": False} if wrong == "no_flip" else {"divide": False} if wrong == "no_divide" else {}))
    chi2 = _chi2(w, group, _softmax(v, first, T))
    print(wrong, "chi2", chi2)
    assert chi2 > 10 * CHI2_999[len(first) - 1]


# ---- the lane set: what the GPU tests count on ----------------------------------------------------------------------------------------------

def test_lane_set_shapes():
    st, tu, dice = SM.lane_set()
    n_cand = np.array([len(SM.candidates(i)[0]) for i in range(len(st))])
    for n in SM.LANE_COUNTS[1:]:
        assert 0 < tu[:n].sum() < n                                            # both movers
        assert (dice[:n, 0] == dice[:n, 1]).any() and (dice[:n, 0] != dice[:n, 1]).any()
        assert (st[:n, 24:26] > 0).any()                                       # somebody on the bar
    assert (n_cand == 0).sum() >= 5                                            # lanes without a move
    home = (st[:, :18] > 0).sum(1) + (st[:, 24] > 0) == 0                      # PLAYER1 to move with every checker home: bear-off turns
    assert ((tu == 0) & home & (n_cand > 0)).sum() >= 5
    assert sum(SM.twin_pair(i) for i in range(len(st))) >= 20


@pytest.mark.parametrize("net", ["ckpt", "dyadic"])
def test_near_tie_census(ckpt, net):
    """Under 1 % of the lanes of every set and temperature the GPU tests use are near ties by the fp64 reference alone"""
    w = ckpt if net == "ckpt" else L.dyadic()
    st, tu, dice = SM.lane_set()
    near = {T: np.zeros(len(st), bool) for T in SM.TEMPERATURES}
    for i in range(len(st)):
        if len(SM.candidates(i)[0]) == 0:
            continue
        rows, ks = _lane_ks(i)
        v = SM.oracle_values(w, i)
        for T in SM.TEMPERATURES:
            near[T][i] = SM.lane(rows, np.arange(len(rows)), v, tu[i], SM.SEED, i, 0, T, ks=ks)["near"]
    for T in SM.TEMPERATURES:
        for n in SM.LANE_COUNTS:
            print(net, "T", T, "lanes", n, "near ties", int(near[T][:n].sum()))
            assert near[T][:n].sum() < 0.01 * n
