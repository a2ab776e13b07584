"""CPU conditions of the move-analysis tests on the MI355X (tests/test_gpu_analysis.py): the exact model of the rule
(tests/analysis_model.py, built on search_model's select / choose) agrees with an independent restatement in plain Python on every G10
lane, three deliberately wrong models do not, the lane set has the shapes the GPU tests name, and the C ABI carries the two entry points.

Values: v1 is the numpy float32 forward pass under the dyadic table (exact ties across the K-th place); V2 stands in as the same lane's v1
values in a seeded permutation -- the model takes any float32 values by index, and a permutation ties exactly as often as v1 does, at
other candidates.  A subset is run under the fp64 reference's own v1 and V2 (tests/search_ref.py) cast to float32."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import analysis_model as A
import nets as N
import search_lanes as L
import search_ref as S

KS = (0, 1, 3, 8)
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _plain(v1, v2, mover, top_k, played, force=True, flip=True, smaller=True):
    """The rule restated with sorted tuples and no numpy.  force / flip / smaller = False are the three wrong models: the played move not
    forced into the kept set, PLAYER2 ranked like PLAYER1, ties to the larger index."""
    m = len(v1)
    if m == 0:
        return dict(status=A.NO_MOVE)
    side = int(mover) if flip else 0

    def order(idx, v):
        return sorted(idx, key=lambda i: ((_bits(v[i]) if side else -_bits(v[i])), i if smaller else -i))
    by_v1 = order(range(m), v1)
    kept = by_v1[:top_k] if top_k else list(by_v1)
    out = dict(status=A.OK, distinct=m, v1_best=_bits(v1[by_v1[0]]))
    if played < 0:
        out.update(status=A.NOT_FOUND, rank1=-1, rank2=-1, v1_played=0, v2_played=0, error=0)
    else:
        out["rank1"] = by_v1.index(played)
        if played not in kept and force:
            kept.append(played)
    by_v2 = order(kept, v2)
    out.update(best=by_v2[0], v2_best=_bits(v2[by_v2[0]]), kept=kept)
    if played >= 0:
        out["rank2"] = by_v2.index(played) if played in by_v2 else -1
        a, b = (by_v2[0], played) if side == 0 else (played, by_v2[0])
        out.update(v1_played=_bits(v1[played]), v2_played=_bits(v2[played]), error=_bits(np.float32(v2[a]) - np.float32(v2[b])))
    return out


def _as_plain(r):
    """a model result in _plain's terms (float fields as bit patterns)"""
    if r["status"] == A.NO_MOVE:
        return dict(status=A.NO_MOVE)
    out = {k: (_bits(r[k]) if k.startswith("v") or k == "error" else int(r[k])) for k in A.FIELDS}
    out.update(best=int(r["best"]), kept=[int(x) for x in r["kept"]])
    return out


@pytest.fixture(scope="module")
def dyadic_lanes():
    """every G10 lane: (v1, v2 stand-in, mover)"""
    tu = L.g10()[1]
    v1s = L.np32_values(L.dyadic(), range(len(tu)))
    rng = np.random.RandomState(11)
    return [(v1, v1[rng.permutation(len(v1))], int(t)) for v1, t in zip(v1s, tu)]


@pytest.fixture(scope="module")
def fp64_lanes():
    """24 G10 lanes with 2 to 24 candidates, 12 of each mover: the fp64 reference's v1 and V2 under the checkpoint, cast to float32"""
    st, tu, dice = L.g10()
    some = [i for i in range(0, 1500, 7) if 2 <= len(L.afterstates(i)) <= 24]
    lanes = [i for i in some if tu[i] == 0][:12] + [i for i in some if tu[i] == 1][:12]
    w = N.checkpoint()
    out = []
    with N.memoized(S, "reply_values"):
        for i in lanes:
            r = S.search(w, st[i], int(tu[i]), int(dice[i, 0]), int(dice[i, 1]), 0)
            v1, v2 = np.empty(len(r["keys"]), np.float32), np.empty(len(r["keys"]), np.float32)
            v1[r["keys"]], v2[r["keys"]] = r["v1"], r["v2"]
            out.append((v1, v2, int(tu[i])))
    assert len(out) == 24
    return out


def _cases(lanes):
    """every (lane, K, family) plus a played state that is none of the lane's"""
    for v1, v2, mover in lanes:
        for K in KS:
            if len(v1) == 0:
                yield v1, v2, mover, K, -1
                continue
            for p in sorted({A.played_index(f, v1, v2, mover, K) for f in A.FAMILIES} | {-1}):
                yield v1, v2, mover, K, p


def _compare(lanes, **wrong):
    n = bad = 0
    for v1, v2, mover, K, p in _cases(lanes):
        bad += _as_plain(A.analyse(v1, v2, mover, K, p)) != _plain(v1, v2, mover, K, p, **wrong)
        n += 1
    return n, bad


def test_model_against_the_plain_restatement(dyadic_lanes, fp64_lanes):
    n, bad = _compare(dyadic_lanes)
    assert n > 15000 and bad == 0, (n, bad)
    n, bad = _compare(fp64_lanes)
    assert n > 300 and bad == 0, (n, bad)


@pytest.mark.parametrize("wrong", ["force", "flip", "smaller"])
def test_wrong_models_are_caught(dyadic_lanes, fp64_lanes, wrong):
    # (the checkpoint's fp64 values hold no exact tie: only the dyadic lanes can tell which index a tie goes to)
    for lanes, floor in ((dyadic_lanes, 500), (fp64_lanes, 0 if wrong == "smaller" else 10)):
        n, bad = _compare(lanes, **{wrong: False})
        assert bad >= floor, (wrong, n, bad)


def test_model_fields():
    """the rule on a hand-made lane: PLAYER1, values by index"""
    v1 = np.array([0.5, 0.75, 0.75, 0.25, 0.125], np.float32)
    v2 = np.array([0.5, 0.25, 0.25, 0.625, 0.75], np.float32)
    r = A.analyse(v1, v2, 0, 2, 3)                          # played ranks third: kept = the tied pair (smaller index first) and the played one
    assert r["kept"].tolist() == [1, 2, 3] and r["rank1"] == 3 and r["rank2"] == 0 and r["best"] == 3 and r["error"] == 0
    r = A.analyse(v1, v2, 0, 2, 2)
    assert r["kept"].tolist() == [1, 2] and r["rank1"] == 1 and r["rank2"] == 1 and r["best"] == 1 and r["error"] == 0   # the bits tie
    r = A.analyse(v1, v2, 1, 2, 1)                          # PLAYER2: smaller is better
    assert r["kept"].tolist() == [4, 3, 1] and r["rank1"] == 3 and r["best"] == 1 and r["rank2"] == 0
    r = A.analyse(v1, v2, 1, 0, 4)
    assert r["rank1"] == 0 and r["rank2"] == 4 and r["best"] == 1 and r["error"] == np.float32(0.5)
    r = A.analyse(v1, v2, 0, 2, -1)
    assert (r["status"], r["rank1"], r["rank2"], r["best"], float(r["error"])) == (A.NOT_FOUND, -1, -1, 1, 0.0) and r["distinct"] == 5
    assert A.analyse(v1[:0], v2[:0], 0, 2, -1)["status"] == A.NO_MOVE
    assert A.analyse(v1, v2, 0, 2, 1, takes_part=False)["status"] == A.IDLE


def test_lane_set(dyadic_lanes):
    """what tests/test_gpu_analysis.py rests on"""
    c = L.counts()
    tu = L.g10()[1]
    assert ((tu == 0).sum(), (tu == 1).sum()) == (724, 776)
    assert (c == 0).sum() == 47 and (c == 1).sum() == 363
    assert ((c >= 9).sum(), ((c >= 9) & (tu == 0)).sum(), ((c >= 9) & (tu == 1)).sum()) == (552, 295, 257)
    assert (c > 128).sum() == 20 and c.max() == 381
    term = np.array([bool(L.terminal(L.afterstates(i), tu[i]).any()) if c[i] else False for i in range(1500)])
    assert (term.sum(), (term & (tu == 0)).sum()) == (75, 29)
    assert (c == 0).sum() >= 40 and term.sum() >= 60
    # exact ties across the K-th place, by mover
    for place, want in ((3, (285, 134)), (8, (210, 111))):
        tie = np.array([L.tie_across(v1, t, place) for v1, _, t in dyadic_lanes])
        got = ((tie & (tu == 0)).sum(), (tie & (tu == 1)).sum())
        assert got == want and min(got) >= 100, (place, got)
    # every played family plays a candidate of its own rank on at least 16 lanes of each mover, for every K it is defined for
    for K in KS:
        for fam in A.FAMILIES:
            need = {"best": 1, "inside": K, "first_out": K + 1, "worst": 1, "v2best": 1}[fam]
            if fam == "inside" and K == 0:
                continue
            has = c >= max(need, 1)
            assert min((has & (tu == 0)).sum(), (has & (tu == 1)).sum()) >= 16, (K, fam)
    # the virtual roots' bound n (K + 1) 21: one, two and three scoring passes
    assert 1500 * 4 * 21 <= L.SEARCH_CHUNK < 1500 * 6 * 21 <= 2 * L.SEARCH_CHUNK < 1500 * 9 * 21 <= 3 * L.SEARCH_CHUNK
    # a tied candidate just outside the top K is played on some lanes (family first_out on a lane that ties across the K-th place)
    for K in (3, 8):
        n = sum(L.tie_across(v1, t, K) and len(v1) > K for v1, _, t in dyadic_lanes)
        assert n >= 100, (K, n)


def test_own_board_is_no_afterstate_when_a_move_exists():
    """the `illegal` family: the pip count falls with every move.  (A doubles roll without a move is one empty sequence: the board itself.)"""
    st = L.g10()[0]
    n_self = 0
    for i in range(1500):
        a = L.afterstates(i)
        if len(a) and (a == st[i]).all(1).any():
            assert len(a) == 1, i
            n_self += 1
    assert n_self == 36                                     # (forced decisions: status 0 with distinct = 1 when the board is "played")


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------

NAMES = ("bgamd_env_analyze_moves", "bgamd_env_analysis_read")


def test_abi_carries_the_analysis():
    import __graft_entry__ as g
    g.build()
    from backgammon_env import _capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bgamd.h")).read(), flags=re.S)
    protos = {n: (res, args) for n, res, args in _capi.SYMBOLS}
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name, n_args in zip(NAMES, (5, 13)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in protos and protos[name][0] is ctypes.c_int and len(protos[name][1]) == n_args, name
        assert hasattr(lib, name), name
