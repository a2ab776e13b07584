"""The 2-ply search's RULES on the MI355X, lane by lane and bit for bit (bgamd_env_step_search: csrc/bg_search.h and the host code from
score_virtual_lanes to bgamd_env_search_read), against the exact model tests/search_model.py fed with the device's own float32 values:
  (a) selection: the kept candidates are the oracle's distinct afterstates, v1 is the greedy step's value of that row, the order and the
      top-K cut are select() of the device's own v1 -- under the checkpoint and under a table that ties candidates exactly ACROSS the
      K-th place (nets.dyadic_table);
  (b) the choice is choose() of the device's own V2, last_choice reports it, want_index names the played sequence;
  (c) V2 is v2_from_replies() of the reply values evaluate_preroll returns, bit for bit;
  (d) the virtual lanes' scoring passes: a four-pass env against one-pass envs, on every lane;
  (e) the scratch env grown, reused while larger than needed and shared with evaluate_preroll; odd lane counts;
  (f) every parity family against the fp64 reference at 1e-5, order and choice held to the model;
  (g) a played run with flips and auto-reset.
tests/test_search_model_cpu.py holds the conditions these rest on (the model against the fp64 reference, the lane sets' shapes)."""
import contextlib

import numpy as np
import pytest

import nets as N
import search_lanes as L
import search_model as M
import search_ref as S
from test_gpu_search import _greedy_positions

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BOUND = 1e-5
KS = (1, 2, 3, 5, 8)
FIELDS = ("kept", "states", "v1", "v2", "after", "value", "seq", "seq_len", "chosen", "count")


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


def _np(x):
    return x.cpu().numpy()


def _table(net, weights):
    return weights if net == "ckpt" else L.dyadic() if net == "dyadic" else N.table(net)


def _search(env, st, tu, dice, top_k, **flags):
    """one search step of `env` from the given boards and dice (no roll, no flip, no restart) -> every result as numpy"""
    env.set_states(st, tu)
    env.set_dice(dice)
    env.step_search(top_k=top_k, roll=False, auto_reset=False, no_flip=True, **flags)
    out = dict(zip(("states", "v1", "v2", "kept"), (_np(x) for x in env.search_candidates())))
    out.update({k: _np(v) for k, v in env.last_choice().items()})
    out["after"] = _np(env.states())
    assert env.stats()["error_flags"] == 0
    return out


def _fresh_search(bg, w, st, tu, dice, top_k, **flags):
    env = bg.VecGame(len(st))
    env.load_weights(w)
    out = _search(env, st, tu, dice, top_k, **flags)
    env.close()
    return out


def _same_runs(a, b, what, lanes_a=slice(None), lanes_b=slice(None), fields=FIELDS):
    """bit-identical results; the candidate arrays may differ in width (top_k = 0: the largest kept count): zeros beyond the narrower"""
    for k in fields:
        x, y = a[k][lanes_a], b[k][lanes_b]
        if k in ("states", "v1", "v2"):
            K = min(x.shape[1], y.shape[1])
            assert not x[:, K:].any() and not y[:, K:].any(), (what, k)
            x, y = x[:, :K], y[:, :K]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.shape, y.shape)
        same = x.reshape(len(x), -1).view(np.uint8) == y.reshape(len(y), -1).view(np.uint8)
        assert same.all(), (what, k, "lanes", np.where(~same.all(1))[0][:8].tolist())


# ---- the 1 500-lane runs: per net, top_k = 0 first (a fresh env: four scoring passes), then each K on the same env -----------------------

_runs = {}


def _g10_runs(bg, weights, net):
    if net not in _runs:
        st, tu, dice = L.g10()
        w = _table(net, weights)
        env = bg.VecGame(len(st))
        env.load_weights(w)
        runs = {K: _search(env, st, tu, dice, K) for K in (0,) + KS}
        env.close()
        # the sibling: one greedy step on the same boards and dice, its rows by (game, state) -- of copies the smallest key's
        sib = bg.VecGame(len(st))
        sib.load_weights(w)
        sib.set_states(st, tu)
        sib.set_dice(dice)
        sib.step_greedy(roll=False, auto_reset=False, no_flip=True)
        info, ust, uval = (_np(x) for x in sib.unique_rows())
        assert sib.stats()["error_flags"] == 0
        sib.close()
        greedy = {}
        for (game, key), s, v in zip(info.tolist(), np.ascontiguousarray(ust, dtype=np.int32), uval):
            k = (game, s.tobytes())
            if k not in greedy or (key & 0x7FFFFFFF) < greedy[k][0]:
                greedy[k] = (key & 0x7FFFFFFF, v)
        _runs[net] = (runs, greedy, _by_index(runs[0]))
    return _runs[net]


def _indices(run, i, cands_index=None):
    """the reference-order indices of lane i's kept states, in the device's order"""
    index = cands_index if cands_index is not None else L.index_of(L.afterstates(i))
    k = int(run["kept"][i])
    rows = np.ascontiguousarray(run["states"][i, :k], dtype=np.int32)
    return np.array([index[r.tobytes()] for r in rows], np.int64)           # (KeyError: a kept state that is no afterstate of the lane)


def _by_index(full):
    """a full-width run's v1 and v2 of every lane in REFERENCE order -> (list of float32 [m], list of float32 [m])"""
    v1s, v2s = [], []
    for i in range(len(full["kept"])):
        m = len(L.afterstates(i))
        assert int(full["kept"][i]) == m, (i, int(full["kept"][i]), m)
        idx = _indices(full, i)
        assert np.array_equal(np.sort(idx), np.arange(m)), i               # exactly the oracle's distinct afterstates, each once
        v1, v2 = np.empty(m, np.float32), np.empty(m, np.float32)
        v1[idx], v2[idx] = full["v1"][i, :m], full["v2"][i, :m]
        v1s.append(v1); v2s.append(v2)
    return v1s, v2s


def _zero_past_kept(run):
    past = np.arange(run["states"].shape[1])[None, :] >= run["kept"][:, None]
    assert not run["states"][past].any() and not run["v1"][past].any() and not run["v2"][past].any()


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- (a) selection ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("net", ["ckpt", "dyadic"])
def test_selection_at_full_width(bg, weights, net):
    runs, greedy, (v1s, v2s) = _g10_runs(bg, weights, net)
    full = runs[0]
    _, tu, _ = L.g10()
    n_term = n_rows = 0
    for i in range(len(tu)):
        m = len(v1s[i])
        if m == 0:
            continue
        cands, mover = L.afterstates(i), int(tu[i])
        term = L.terminal(cands, mover)
        outcome = np.float32(1.0 if mover == 0 else 0.0)
        assert (_u32(v1s[i][term]) == _u32(outcome)).all(), i              # a terminal row: exactly its outcome, at both plies
        assert (_u32(v2s[i][term]) == _u32(outcome)).all(), i
        want = np.array([greedy[(i, c.tobytes())][1] for c in cands], np.float32)
        assert np.array_equal(_u32(v1s[i][~term]), _u32(want[~term])), i   # any other: the greedy step's value of that row, bit for bit
        assert np.array_equal(_indices(full, i), M.select(np.arange(m), v1s[i], mover, 0)), i
        n_term += int(term.sum()); n_rows += m
    _zero_past_kept(full)
    assert n_rows == int(L.counts().sum()) and n_term >= 40
    assert full["states"].shape[1] == 381                                  # the widest board: six rounds of the 64-row walk


@pytest.mark.parametrize("net", ["ckpt", "dyadic"])
def test_selection_top_k(bg, weights, net):
    runs, _, (v1s, v2s) = _g10_runs(bg, weights, net)
    _, tu, _ = L.g10()
    for K in KS:
        run = runs[K]
        assert run["states"].shape[1] == K
        _zero_past_kept(run)
        for i in range(len(tu)):
            m = len(v1s[i])
            assert int(run["kept"][i]) == min(K, m), (K, i)
            if m == 0:
                continue
            idx = _indices(run, i)
            assert np.array_equal(idx, M.select(np.arange(m), v1s[i], int(tu[i]), K)), (net, K, i, idx)
            k = len(idx)
            assert np.array_equal(_u32(run["v1"][i, :k]), _u32(v1s[i][idx])), (net, K, i)
            assert np.array_equal(_u32(run["v2"][i, :k]), _u32(v2s[i][idx])), (net, K, i)


@pytest.mark.parametrize("net", ["ckpt", "dyadic"])
def test_top_k_above_every_count_is_full_width(bg, weights, net):
    """top_k = 512 on 64 lanes that include the 381-candidate board and the other boards with more than 128: full width, bit for bit"""
    runs, _, _ = _g10_runs(bg, weights, net)
    st, tu, dice = L.g10()
    c = L.counts()
    lanes = np.argsort(-c, kind="stable")[:40].tolist() + np.where(c == 0)[0][:4].tolist()
    lanes = np.array(sorted(lanes + [i for i in range(64) if i not in lanes][:20]))
    assert len(set(lanes.tolist())) == 64 and int(c.argmax()) in lanes and (c[lanes] > 128).sum() >= 20 and (c[lanes] == 0).any()
    run = _fresh_search(bg, _table(net, weights), st[lanes], tu[lanes], dice[lanes], 512)
    assert run["states"].shape[1] == 512
    _zero_past_kept(run)
    _same_runs(run, runs[0], "top_k 512 against full width", lanes_b=lanes)


def test_device_tie_census(bg, weights):
    """Under the dyadic table the device's own v1 must tie exactly where exact arithmetic ties: across the 3rd and the 8th place on at
    least half as many lanes as the numpy float32 forward pass does on the same 1 500 boards (and as the CPU census of every sixth board
    scales to: 6 x 60 / 2 and 6 x 40 / 2).  Far fewer would mean that the evaluator breaks exact ties by its order of summation -- and that
    the selection tests above never met a tie across the K-th place."""
    _, _, (v1s, _) = _g10_runs(bg, weights, "dyadic")
    tu = L.g10()[1]
    dev = L.census(v1s, tu)
    cpu = L.census(L.np32_values(L.dyadic(), range(len(tu))), tu)
    print("TIE-CENSUS dyadic table, 1500 G10 boards, device v1:    ", dev)
    print("TIE-CENSUS dyadic table, 1500 G10 boards, numpy float32:", cpu)
    assert dev["lanes"] == cpu["lanes"]
    assert dev["across3"] >= max(cpu["across3"] / 2, 180), (dev, cpu)
    assert dev["across8"] >= max(cpu["across8"] / 2, 120), (dev, cpu)


# ---- (b) the choice -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("net", ["ckpt", "dyadic"])
def test_choice(bg, weights, net):
    runs, _, _ = _g10_runs(bg, weights, net)
    st, tu, _ = L.g10()
    n_v2_ties = 0
    for K, run in runs.items():
        for i in range(len(tu)):
            k = int(run["kept"][i])
            if k == 0:
                assert np.array_equal(run["after"][i], st[i]), (net, K, i)   # no move: the board stays
                continue
            v2 = run["v2"][i, :k]
            j = M.choose(_indices(run, i), v2, int(tu[i]))
            assert np.array_equal(run["after"][i], run["states"][i, j]), (net, K, i, j)
            assert _u32(run["value"][i]) == _u32(v2[j]), (net, K, i)
            best = v2.max() if tu[i] == 0 else v2.min()
            n_v2_ties += int((v2 == best).sum() > 1)
    print("V2-TIES %s: %d (lane, K) pairs where the smaller index decided between equal best V2" % (net, n_v2_ties))
    assert net != "dyadic" or n_v2_ties > 0


def _apply_sequence(O, s28, mover, dice, seq):
    s = O.State.from28(s28, mover)
    for o, d in seq:
        die = [x for x in sorted(set(int(v) for v in dice)) if (int(o), int(d)) in O.legal_moves(s, mover, x)]
        assert die, ("not a legal move", s.to28().tolist(), mover, dice, (o, d))
        ok, msg = O.try_move(s, mover, die[0], int(o), int(d))
        assert ok, msg
    return s.to28()


@pytest.mark.parametrize("top_k", [0, 3])
def test_want_index(bg, weights, top_k):
    """include/bgamd.h item 6: with BGAMD_WANT_INDEX chosen and count are exact -- the reference-order index of the FIRST sequence that
    gives the played board, and the number of sequences (copies included: most of these boards have some)."""
    from oracle import oracle as O
    st, tu, dice = (x[:256] for x in L.g10())
    env = bg.VecGame(256)
    env.load_weights(weights)
    env.set_states(st, tu)
    env.set_dice(dice)
    offs, cnts, est, esq, eln = (_np(x) for x in env.enumerate())
    run = _search(env, st, tu, dice, top_k, want_index=True)
    plain = _fresh_search(bg, weights, st, tu, dice, top_k)
    env.close()
    _same_runs(run, plain, "want_index against without", fields=FIELDS[:8])
    assert np.array_equal(run["count"], cnts)
    n_copies = 0
    for i in range(256):
        if cnts[i] == 0:
            assert run["chosen"][i] == -1 and np.array_equal(run["after"][i], st[i])
            continue
        lane = est[offs[i]:offs[i] + cnts[i]]
        n_copies += cnts[i] > len(L.afterstates(i))
        ch = int(run["chosen"][i])
        assert 0 <= ch < cnts[i] and np.array_equal(lane[ch], run["after"][i]), i
        assert not (lane[:ch] == run["after"][i]).all(1).any(), i           # the first sequence with that board
        ln = int(run["seq_len"][i])
        assert ln == eln[offs[i] + ch] and np.array_equal(run["seq"][i], esq[offs[i] + ch]), i
        assert np.array_equal(_apply_sequence(O, st[i], int(tu[i]), dice[i], run["seq"][i][:ln]), run["after"][i]), i
    assert n_copies >= 100


# ---- (c) V2 from the replies, bit for bit -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def run_512(bg, weights):
    """the first 512 G10 boards at full width on a fresh env: 136 815 virtual lanes, two scoring passes"""
    st, tu, dice = (x[:512] for x in L.g10())
    return _fresh_search(bg, weights, st, tu, dice, 0)


def _no_reply(c28, opp):
    """rolls the opponent cannot play because it sits on the bar against made points (bool [n, 21]; other reasons are not looked for)"""
    c28 = np.asarray(c28)
    out = np.zeros((len(c28), 21), bool)
    for r, (a, b) in enumerate(S.ROLLS):
        for side in (0, 1):
            on_bar = c28[:, 24 + side] > 0
            shut = [(c28[:, d - 1] <= -2) if side == 0 else (c28[:, 24 - d] >= 2) for d in (a, b)]
            out[:, r] |= (opp == side) & on_bar & shut[0] & shut[1]
    return out


def test_v2_is_the_stated_sum_of_the_reply_values(bg, weights, run_512):
    tu = L.g10()[1][:512]
    has = np.arange(run_512["states"].shape[1])[None, :] < run_512["kept"][:, None]
    lane = np.broadcast_to(np.arange(512)[:, None], has.shape)[has]
    cand, v1, v2 = run_512["states"][has], run_512["v1"][has], run_512["v2"][has]
    mover = tu[lane]
    term = cand[np.arange(len(cand)), 26 + mover] == 15
    assert (_u32(v2[term]) == _u32(v1[term])).all() and term.sum() > 0
    # a position that is over for the OPPONENT (handed in that way) is no terminal candidate for the search, but evaluate_preroll scores it
    # by its outcome: left out
    cmp = ~term & (cand[np.arange(len(cand)), 27 - mover] != 15)
    assert cmp.sum() > 6000
    env = bg.VecGame(64)
    env.load_weights(weights)
    f, _ = (_np(x) for x in env.evaluate_preroll(cand[cmp], 1 - mover[cmp]))
    assert env.stats()["error_flags"] == 0
    env.close()
    want = M.v2_from_replies(f)
    bad = np.where(_u32(v2[cmp]) != _u32(want))[0]
    assert len(bad) == 0, (len(bad), lane[cmp][bad][:8].tolist(), v2[cmp][bad][:4].tolist(), want[bad][:4].tolist())
    # rolls without a reply among them (srch_collect_kernel's own hidden-to-value loop)
    shut = _no_reply(cand[cmp], 1 - mover[cmp])
    assert shut.any()
    q, r = (int(x[0]) for x in np.where(shut))
    x = S.distinct_afterstates(cand[cmp][q], int(1 - mover[cmp][q]), *S.ROLLS[r])
    assert len(x) == 0 or (len(x) == 1 and (x[0] == cand[cmp][q]).all())


# ---- (d) the scoring passes ---------------------------------------------------------------------------------------------------------------

def test_chunk_boundaries(bg, weights):
    """1 500 lanes at full width are scored in four passes of 131 072 virtual lanes; six envs of at most 256 lanes in one pass each.  Every
    lane's result is bit-identical -- the lanes whose candidates' 21 rolls are split between two passes among them."""
    runs, _, _ = _g10_runs(bg, weights, "ckpt")
    big = runs[0]
    st, tu, dice = L.g10()
    koff = np.concatenate([[0], np.cumsum(big["kept"])])
    assert 3 * L.SEARCH_CHUNK < koff[-1] * 21 <= 4 * L.SEARCH_CHUNK
    split = [int(np.searchsorted(koff, L.SEARCH_CHUNK * p // 21, side="right")) - 1 for p in (1, 2, 3)]
    assert split == [494, 960, 1400] and (big["kept"][split] >= 2).all(), (split, big["kept"][split])
    for lo in range(0, len(st), 256):
        hi = min(lo + 256, len(st))
        small = _fresh_search(bg, weights, st[lo:hi], tu[lo:hi], dice[lo:hi], 0)
        assert small["kept"].sum() * 21 <= L.SEARCH_CHUNK
        _same_runs(big, small, "lanes %d..%d" % (lo, hi), lanes_a=slice(lo, hi))


# ---- (e) the scratch env's life cycle, lane counts ---------------------------------------------------------------------------------------

def test_scratch_env_life_cycle(bg, weights, run_512):
    """One env: a search that needs a small scratch env, one that needs the full chunk (the scratch env is re-created), the small one again
    (the scratch env is larger than needed: one pass over mostly idle lanes), evaluate_preroll on the same scratch env in between.  Every
    result equals a fresh env's."""
    st, tu, dice = (x[:512].copy() for x in L.g10())
    shut, shut_t = N.closed_board_positions()
    assert len(S.distinct_afterstates(shut[0], int(shut_t[0]), 1, 2)) == 0
    st_s, tu_s, dice_s = st.copy(), tu.copy(), dice.copy()
    st_s[64:], tu_s[64:], dice_s[64:] = shut[0], shut_t[0], (1, 2)          # 448 lanes without a move: a 64-lane-sized search
    ps, pt = N.preroll_positions()
    fresh_small = _fresh_search(bg, weights, st_s, tu_s, dice_s, 0)
    assert 0 < fresh_small["kept"].sum() * 21 < L.SEARCH_CHUNK // 4 and not fresh_small["kept"][64:].any()
    probe = bg.VecGame(64)
    probe.load_weights(weights)
    fresh_pre = [_np(x) for x in probe.evaluate_preroll(ps, pt)]
    probe.close()
    env = bg.VecGame(512)
    env.load_weights(weights)

    def preroll(what):
        got = [_np(x) for x in env.evaluate_preroll(ps, pt)]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, fresh_pre)), what
    _same_runs(_search(env, st_s, tu_s, dice_s, 0), fresh_small, "small, first")
    preroll("after the small search")
    _same_runs(_search(env, st, tu, dice, 0), run_512, "large, after the scratch env grew")
    preroll("after the large search")
    _same_runs(_search(env, st_s, tu_s, dice_s, 0), fresh_small, "small, on the larger scratch env")
    _same_runs(_search(env, st, tu, dice, 0), run_512, "large again")
    assert env.stats()["error_flags"] == 0
    env.close()


@pytest.mark.parametrize("n", [1, 63, 65, 777, 1025])
def test_lane_counts(bg, weights, n):
    """srch_scan_kernel walks the lanes 1 024 at a time with a tail; srch_reduce / srch_read / apply in blocks of 256 and 64"""
    runs, _, _ = _g10_runs(bg, weights, "ckpt")
    st, tu, dice = (x[:n] for x in L.g10())
    _same_runs(_fresh_search(bg, weights, st, tu, dice, 3), runs[3], "%d lanes" % n, lanes_b=slice(0, n))


# ---- (f) every parity family against the fp64 reference -----------------------------------------------------------------------------------

@contextlib.contextmanager
def _memoized_moves():
    """search_ref.distinct_afterstates -- a pure function of (position, player, dice) -- answered from a cache shared by the families"""
    fn = S.distinct_afterstates

    def cached(s28, player, d1, d2):
        key = (np.asarray(s28, np.int32).tobytes(), int(player), int(d1), int(d2))
        if key not in _moves:
            _moves[key] = fn(s28, player, d1, d2)
        return _moves[key]
    S.distinct_afterstates = cached
    try:
        yield
    finally:
        S.distinct_afterstates = fn


_moves = {}


@pytest.fixture(scope="module")
def family_lanes(bg, weights):
    """16 lanes: 8 reached by greedy play, 8 from G10 -- one with 67 candidates (two rounds of the 64-row walk), one without a move, one
    with a terminal candidate, both movers"""
    gs, gt = _greedy_positions(bg, weights, 8, seed=17)
    gd = np.random.RandomState(17).randint(1, 7, (8, 2))
    st, tu, dice = L.g10()
    c = L.counts()
    pick = [315, int(np.where(c == 0)[0][0]),
            next(i for i in range(1500) if 2 <= c[i] <= 12 and L.terminal(L.afterstates(i), tu[i]).any())]
    pick += [i for i in range(1500) if 4 <= c[i] <= 24 and tu[i] == 1 and i not in pick][:3]
    pick += [i for i in range(1500) if 4 <= c[i] <= 24 and tu[i] == 0 and i not in pick][:2]
    assert len(pick) == 8 and c[315] > 64
    return (np.concatenate([gs, st[pick]]).astype(np.int32), np.concatenate([gt, tu[pick]]).astype(np.int32),
            np.concatenate([gd, dice[pick]]).astype(np.int32))


@pytest.mark.parametrize("family", N.PARITY + ("dyadic",))
def test_families(bg, weights, family_lanes, family):
    st, tu, dice = family_lanes
    w = _table(family, weights)
    env = bg.VecGame(len(st))
    env.load_weights(w)
    worst1 = worst2 = 0.0
    n_cmp = 0
    full_v1 = {}                                                          # lane -> the K = 0 run's v1 in reference order
    with _memoized_moves(), N.memoized(S, "reply_values"):
        for K in (0, 3):
            run = _search(env, st, tu, dice, K)
            _zero_past_kept(run)
            for i in range(len(st)):
                r = S.search(w, st[i], int(tu[i]), int(dice[i, 0]), int(dice[i, 1]), K)
                k = len(r["states"])
                assert int(run["kept"][i]) == k, (family, K, i)
                if k == 0:
                    assert np.array_equal(run["after"][i], st[i])
                    continue
                mover = int(tu[i])
                cands = S.distinct_afterstates(st[i], mover, int(dice[i, 0]), int(dice[i, 1]))
                idx = _indices(run, i, L.index_of(cands))
                # values: the reference's, state by state
                ref1 = dict(zip(r["keys"].tolist(), r["v1"]))
                ref2 = dict(zip(r["keys"].tolist(), r["v2"]))
                for j, key in enumerate(idx.tolist()):
                    if key in ref1:
                        worst1 = max(worst1, abs(float(run["v1"][i, j]) - ref1[key]))
                        worst2 = max(worst2, abs(float(run["v2"][i, j]) - ref2[key]))
                        n_cmp += 1
                # order and choice: the model on the device's own values -- no lane is excused as a near tie
                if K == 0:
                    assert np.array_equal(np.sort(idx), np.arange(len(cands))), (family, i)
                    full_v1[i] = np.empty(k, np.float32)
                    full_v1[i][idx] = run["v1"][i, :k]
                else:
                    assert np.array_equal(_u32(run["v1"][i, :k]), _u32(full_v1[i][idx])), (family, K, i)
                assert np.array_equal(idx, M.select(np.arange(len(cands)), full_v1[i], mover, K)), (family, K, i)
                j = M.choose(idx, run["v2"][i, :k], mover)
                assert np.array_equal(run["after"][i], run["states"][i, j]), (family, K, i)
                assert _u32(run["value"][i]) == _u32(run["v2"][i, j]), (family, K, i)
                if family == "dyadic":                                       # exact ties are exact in fp64 too: the reference outright
                    assert np.array_equal(idx, r["keys"]), (K, i, idx, r["keys"])
                    assert np.array_equal(run["after"][i], r["states"][r["choice"]]), (K, i)
    print("NETS-MAX %-13s %-28s %6d values: max |gpu - fp64| = %.3g (v1), %.3g (v2)" % (family, "step_search, K = 0 and 3", n_cmp, worst1, worst2))
    env.close()
    assert n_cmp > 200
    assert worst1 <= BOUND and worst2 <= BOUND, (family, worst1, worst2)


# ---- (g) a played run ---------------------------------------------------------------------------------------------------------------------

def test_played_run(bg, weights):
    """512 lanes from short bear-offs and single-checker races, 12 turns of roll() + step_search(top_k = 2) with flips and auto-reset: every
    board is the model's choice among the kept candidates, the turn passes on, a lane whose mover bore off its 15th checker restarts."""
    n = 512
    p_st, p_tu = N._cat(N._bearoffs(), N._singles())
    reps = -(-n // len(p_st))
    probe = bg.VecGame(1)
    start = _np(probe.states())[0]
    probe.close()
    env = bg.VecGame(n, seed=31)
    env.load_weights(weights)
    env.set_states(np.tile(p_st, (reps, 1))[:n], np.tile(p_tu, reps)[:n])
    finished = n_two = 0
    with _memoized_moves():
        for turn in range(12):
            env.roll()
            pre, pt, dice = _np(env.states()), _np(env.turns()), _np(env.dice())
            env.step_search(top_k=2, roll=False)
            states, v1, v2, kept = (_np(x) for x in env.search_candidates())
            post, after_turn = _np(env.states()), _np(env.turns())
            for i in range(n):
                mover = int(pt[i])
                cands = S.distinct_afterstates(pre[i], mover, int(dice[i, 0]), int(dice[i, 1]))
                k = min(2, len(cands))
                assert int(kept[i]) == k, (turn, i)
                if k == 0:
                    assert np.array_equal(post[i], pre[i]) and after_turn[i] == 1 - mover, (turn, i)
                    continue
                idx = _indices({"kept": kept, "states": states}, i, L.index_of(cands))
                assert len(set(idx.tolist())) == k
                assert np.array_equal(idx, M.select(idx, v1[i, :k], mover, 0)), (turn, i)      # best v1 first, the smaller index on a tie
                n_two += k == 2
                played = states[i, M.choose(idx, v2[i, :k], mover)]
                if played[26 + mover] == 15:
                    finished += 1
                    assert np.array_equal(post[i], start), (turn, i)                        # restarted (the opening roll decides who moves)
                else:
                    assert np.array_equal(post[i], played) and after_turn[i] == 1 - mover, (turn, i)
    s = env.stats()
    env.close()
    assert s["error_flags"] == 0
    assert s["games_finished"] == finished and finished > 100, (s["games_finished"], finished)
    assert n_two > 100
