"""The value net and the move choice on the MI355X under MANY weight tables (tests/nets.py), not the checkpoint alone:
  * every evaluator against the oracle's fp64 forward pass, at the project's flat 1e-5, for each of the seven parity families, on fixture
    rows, on a sweep that gathers every W1 column with every multiplier and sign, and on arbitrary boards;
  * edge nets: a saturated hidden layer (w1_x64), outputs that are exactly 1.0 / 0.0 (out_hi / out_lo);
  * the tie rule "smallest reference key wins" between DISTINCT afterstates, strictly, under a net that gives every row the same value
    (zero_w1): greedy step (4 096 and 65 536 lanes), 2-ply search, rollouts;
  * a reload of the weights reaches the scratch envs of the search, the pre-roll evaluation and the rollouts."""
import numpy as np
import pytest

import nets as N
import rollout_ref as R
import rollout_vr_ref as V
import search_ref as S
from test_gpu_parity import _check_greedy_step, _np
from test_gpu_rollout_vr import _ties
from test_gpu_search import _lanes, _setup

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 4242
BOUND = 1e-5


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


# ---- references, computed once per (family, row set) -------------------------------------------------------------------------------

_refs = {}


def _rowset(key):
    """-> (states, turn bit of each row) of a row set: "dense", "root" (G5 + sweep: root == row), or a pair set's rows"""
    if key == "dense":
        return N.value_rows()
    if key == "root":
        a, b = N.g5_rows(), N.sweep_rows()
        return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    roots, rt, rows, ri = N.pair_sets()[key]
    return rows, rt[ri]


def _ref(O, family, key):
    if (family, key) not in _refs:
        st, tu = _rowset(key)
        X = N.encode(st, tu)
        _refs[(family, key)] = (st, tu, X, O.forward_f64(N.table(family), X))
    return _refs[(family, key)]


def _against_fp64(O, family, what, key, got, idx=None, bound=BOUND):
    """max |gpu - fp64 oracle| over the rows (idx: a subset of the row set); on failure the family, the row, both values and the numpy
    fp32 forward's own error of that row."""
    st, tu, X, ref = _ref(O, family, key)
    if idx is not None:
        st, tu, X, ref = st[idx], tu[idx], X[idx], ref[idx]
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all(), (family, what)          # a sigmoid's output, whatever the net
    err = np.abs(got - ref)
    worst = float(err.max())
    if idx is None:
        print("NETS-MAX %-13s %-28s %6d rows: max |gpu - fp64| = %.3g" % (family, what, len(ref), worst))
    if not np.isfinite(got).all() or worst > bound:
        i = int(np.nanargmax(np.where(np.isfinite(err), err, np.inf)))
        e32 = abs(float(N.forward_np32(N.table(family), X[i:i + 1])[0]) - ref[i])
        pytest.fail("%s, %s: row %d (state %s, turn %d): gpu %r, fp64 %r, |diff| %.3g > %.3g; numpy fp32 forward error of that row %.3g"
                    % (family, what, i, st[i].tolist(), tu[i], float(got[i]), float(ref[i]), err[i], bound, e32))
    return worst


def _dense(bg, O, family, precisions, bound_of=None):
    st, tu = N.value_rows()
    env = bg.VecGame(64)
    env.load_weights(N.table(family))
    rng = np.random.RandomState(7)
    out = {}
    for prec, name in precisions:
        bound = bound_of("dense") if bound_of else BOUND
        v = _np(env.evaluate(st, tu, precision=prec))
        out[name] = _against_fp64(O, family, "evaluate " + name, "dense", v, bound=bound)
        for m in (1, 31, 33):                                # ragged sizes around the 32-row tile
            idx = rng.randint(0, len(tu), m)
            _against_fp64(O, family, "evaluate %s, %d rows" % (name, m), "dense", _np(env.evaluate(st[idx], tu[idx], precision=prec)), idx,
                          bound=bound)
    assert env.stats()["error_flags"] == 0
    env.close()
    return out


def _incremental(bg, O, family, bound_of=None):
    env = bg.VecGame(4096)
    env.load_weights(N.table(family))
    out = {}
    st, tu = _rowset("root")                                 # root == row (an empty list): the root pass alone
    v = _np(env.evaluate_incremental(st, tu, st, np.arange(len(st), dtype=np.int32)))
    out["root"] = _against_fp64(O, family, "root pass alone", "root", v, bound=bound_of("root") if bound_of else BOUND)
    for key, (roots, rt, rows, ri) in N.pair_sets().items():
        v = _np(env.evaluate_incremental(roots, rt, rows, ri))
        out[key] = _against_fp64(O, family, "evaluate_incremental " + key, key, v, bound=bound_of(key) if bound_of else BOUND)
    assert env.stats()["error_flags"] == 0
    env.close()
    return out


def _greedy_rows(bg, O, family, bound=BOUND):
    """One greedy step on fixture G7's roots with their dice: the rows handed to the value net are the reference's distinct afterstates,
    and EVERY row's value is checked (as test_delta_kernel_rows_vs_reference_values does under the checkpoint)."""
    roots, rt, dice, rows, ri, off = N.fixture_pairs("g7_candidate_values")
    env = bg.VecGame(len(roots), arena_rows=1 << 20)
    env.load_weights(N.table(family))
    env.set_states(roots, rt)
    env.set_dice(dice)
    env.step_greedy(roll=False, auto_reset=False, precision=bg.F32)
    info, st, val = [_np(x) for x in env.unique_rows()]
    assert env.stats()["error_flags"] == 0
    game = info[:, 0].astype(np.int64)
    for k in range(len(roots)):
        got = {tuple(int(v) for v in s) for s in st[game == k]}
        assert got == {tuple(int(v) for v in s) for s in rows[off[k]:off[k + 1]]}, (family, k)
    assert len(st) >= len(rows)
    X = N.encode(st, rt[game])
    ref = O.forward_f64(N.table(family), X)
    err = np.abs(val.astype(np.float64) - ref)
    worst = float(err.max())
    print("NETS-MAX %-13s %-28s %6d rows: max |gpu - fp64| = %.3g" % (family, "greedy step rows (G7)", len(st), worst))
    i = int(err.argmax())
    assert np.isfinite(val).all() and worst <= bound, (family, i, st[i].tolist(), float(val[i]), float(ref[i]),
                                                       abs(float(N.forward_np32(N.table(family), X[i:i + 1])[0]) - ref[i]))
    env.close()
    return worst, val


# ---- values, for each parity family, against the fp64 forward pass at 1e-5 ------------------------------------------------------------

@pytest.mark.parametrize("family", N.PARITY)
def test_dense_evaluators(bg, O, family):
    _dense(bg, O, family, ((bg.F32, "F32"), (bg.F16X2, "F16X2")))


@pytest.mark.parametrize("family", N.PARITY)
def test_incremental_evaluator(bg, O, family):
    """root_hidden_resident_kernel + eval_rows_delta_kernel through the stateless operator: the root pass alone, the fixture pairs, and
    the sweep's pairs -- every W1^T row gathered with + and - multipliers of every size the list entry can take from one changed count."""
    _incremental(bg, O, family)


@pytest.mark.parametrize("family", N.PARITY)
def test_greedy_step_rows(bg, O, family):
    _greedy_rows(bg, O, family)


@pytest.fixture(scope="module")
def preroll_positions():
    ps, pt = N.preroll_positions()
    no_move = np.array([[len(S.distinct_afterstates(s, int(t), a, b)) == 0 for a, b in S.ROLLS] for s, t in zip(ps, pt)])
    assert no_move.any()                                     # rolls that srch_collect_kernel scores with its own sigmoid loop
    return ps, pt, no_move


@pytest.mark.parametrize("family", N.PARITY)
def test_preroll(bg, family, preroll_positions):
    ps, pt, no_move = preroll_positions
    w = N.table(family)
    env = bg.VecGame(64)
    env.load_weights(w)
    f, m = (_np(x) for x in env.evaluate_preroll(ps, pt))
    n_cmp, worst, worst_pass = 0, 0.0, 0.0
    for q in range(len(ps)):
        rf, rm = V.preroll(w, ps[q], int(pt[q]))
        ok = ~_ties(w, ps[q], int(pt[q]))
        n_cmp += int(ok.sum())
        d = np.abs(f[q] - rf)
        worst = max(worst, float(d[ok].max()) if ok.any() else 0.0)
        worst_pass = max(worst_pass, float(d[no_move[q]].max()) if no_move[q].any() else 0.0)
        np.testing.assert_allclose(f[q][ok], rf[ok], atol=BOUND, rtol=0, err_msg=f"{family}, position {q}")
        if ok.all():
            assert abs(m[q] - rm) < BOUND
    print("NETS-MAX %-13s %-28s %6d rolls: max |gpu - fp64| = %.3g (rolls without a move: %.3g)" % (family, "evaluate_preroll", n_cmp, worst,
                                                                                                   worst_pass))
    assert n_cmp >= 0.9 * 21 * len(ps)
    assert env.stats()["error_flags"] == 0
    env.close()


@pytest.mark.parametrize("family", N.PARITY)
def test_truncated_rollout(bg, family):
    """Trials cut after 3 turns: the truncation value comes from the dense evaluator on a scratch env."""
    st, tu = N.family_rollout_positions()
    w = N.table(family)
    env = bg.VecGame(64)
    env.load_weights(w)
    T = 36
    r = env.rollout(st, tu, T, max_plies=3, rotate=True, seed=SEED, per_trial=True)
    tv, tt = _np(r["trial_value"]), _np(r["trial_turns"])
    ref = R.rollout(w, st, tu, T, SEED, max_plies=3, rotate=True)
    cmp = ~ref["near_tie"]
    assert cmp.mean() >= 0.9, cmp.mean()
    trunc, full = ref["truncated"] & cmp, ~ref["truncated"] & cmp
    assert trunc.sum() > 0 and full.sum() > 0
    np.testing.assert_array_equal(tt[cmp], ref["turns"][cmp])
    np.testing.assert_array_equal(tv[full], ref["value"][full])
    print("NETS-MAX %-13s %-28s %6d trials: max |gpu - fp64| = %.3g" % (family, "rollout truncation value", int(trunc.sum()),
                                                                        np.abs(tv[trunc] - ref["value"][trunc]).max()))
    np.testing.assert_allclose(tv[trunc], ref["value"][trunc], atol=BOUND, rtol=0)
    env.close()


# loguniform is left out: bf16 keeps 8 bits of a W1 that spans eight decades, and the mode promises nothing there
@pytest.mark.parametrize("family", [f for f in N.PARITY if f != "loguniform"])
def test_bf16_mode_against_its_emulation(bg, family):
    st, tu = N.value_rows()
    w = N.table(family)
    env = bg.VecGame(64)
    env.load_weights(w)
    v = _np(env.evaluate(st, tu, precision=bg.BF16))
    ref = N.forward_bf16_f64(w, N.encode(st, tu))
    err = np.abs(v - ref)
    print("NETS-MAX %-13s %-28s %6d rows: max |gpu - bf16 emulation| = %.3g" % (family, "evaluate BF16", len(v), err.max()))
    i = int(err.argmax())
    assert err.max() < 2e-5, (family, i, st[i].tolist(), int(tu[i]), float(v[i]), float(ref[i]))
    env.close()


# ---- edge nets -----------------------------------------------------------------------------------------------------------------------

def test_saturated_hidden_layer(bg, O):
    """w1_x64: most hidden units saturate, exp2 overflows to inf and underflows to 0.  Every value is finite and inside [0, 1], no error
    flag, and |gpu - fp64| <= max(1e-5, 4 e32), e32 = the largest error of the numpy fp32 forward pass over the same rows: the factor
    covers another summation order plus the two hardware approximations (v_exp_f32, v_rcp_f32) on top of one fp32 evaluation."""
    fam = "w1_x64"
    e32 = {}

    def bound_of(key):
        st, tu, X, ref = _ref(O, fam, key)
        e32[key] = float(np.abs(N.forward_np32(N.table(fam), X).astype(np.float64) - ref).max())
        return max(BOUND, 4 * e32[key])
    got = {("dense " + k): (v, "dense") for k, v in _dense(bg, O, fam, ((bg.F32, "F32"), (bg.F16X2, "F16X2")), bound_of).items()}
    got.update({("incremental " + k): (v, k) for k, v in _incremental(bg, O, fam, bound_of).items()})
    worst, val = _greedy_rows(bg, O, fam, bound_of("g7"))
    got["greedy step rows"] = (worst, "g7")
    assert (val >= 0).all() and (val <= 1).all()
    for k, (v, key) in got.items():
        print("NETS-MAX %-13s %-28s ratio to the numpy fp32 forward's own error %.3g: %.2f" % (fam, k, e32[key], v / e32[key]))
    # in [0, 1]: once more over the dense rows, values themselves
    env = bg.VecGame(64)
    env.load_weights(N.table(fam))
    st, tu = N.value_rows()
    for prec in (bg.F32, bg.F16X2):
        v = _np(env.evaluate(st, tu, precision=prec))
        assert np.isfinite(v).all() and (v >= 0).all() and (v <= 1).all()
    env.close()


def _e32(O, w, rows):
    """the numpy fp32 forward's largest error against fp64 over recorded rows (tests/nets.py, recorded_net_rows)"""
    X = np.concatenate(rows)
    return float(np.abs(N.forward_np32(w, X).astype(np.float64) - O.forward_f64(w, X)).max())


def test_saturated_hidden_layer_preroll_rollout_bf16(bg, O, preroll_positions):
    """w1_x64 through the other evaluators, same conditions: evaluate_preroll (rolls without a move go through srch_collect_kernel's own
    rcp(1 + exp2(h)) loop with exp2 at inf and 0), the truncation value of 3-turn rollouts, and BF16.  e32 is taken over the very rows the
    fp64 reference evaluated.  BF16 is held against its own emulation as for the parity families, at max(2e-5, 4 e32) with e32 the numpy
    fp32 forward's error on the bf16-rounded table and features."""
    fam = "w1_x64"
    w = N.table(fam)
    env = bg.VecGame(64)
    env.load_weights(w)
    # pre-roll
    ps, pt, no_move = preroll_positions
    f, m = (_np(x) for x in env.evaluate_preroll(ps, pt))
    assert np.isfinite(f).all() and (f >= 0).all() and (f <= 1).all() and np.isfinite(m).all() and (m >= 0).all() and (m <= 1).all()
    with N.recorded_net_rows(S) as rows:
        refs = [V.preroll(w, ps[q], int(pt[q])) for q in range(len(ps))]
    e32 = _e32(O, w, rows)
    bound = max(BOUND, 4 * e32)
    n_cmp, worst, worst_pass = 0, 0.0, 0.0
    for q, (rf, rm) in enumerate(refs):
        ok = ~_ties(w, ps[q], int(pt[q]))
        n_cmp += int(ok.sum())
        d = np.abs(f[q] - rf)
        worst = max(worst, float(d[ok].max()) if ok.any() else 0.0)
        worst_pass = max(worst_pass, float(d[no_move[q] & ok].max()) if (no_move[q] & ok).any() else 0.0)
        assert (d[ok] <= bound).all(), (q, d, bound)
        if ok.all():
            assert abs(m[q] - rm) <= bound
    assert n_cmp >= 0.9 * 21 * len(ps) and no_move.any()
    print("NETS-MAX %-13s %-28s %6d rolls: max |gpu - fp64| = %.3g (rolls without a move: %.3g), ratio to the numpy fp32 forward's own "
          "error %.3g: %.2f" % (fam, "evaluate_preroll", n_cmp, worst, worst_pass, e32, worst / e32))
    # 3-turn rollouts
    st, tu = N.family_rollout_positions()
    r = env.rollout(st, tu, 36, max_plies=3, rotate=True, seed=SEED, per_trial=True)
    tv, tt = _np(r["trial_value"]), _np(r["trial_turns"])
    assert np.isfinite(tv).all() and (tv >= 0).all() and (tv <= 1).all()
    with N.recorded_net_rows(S) as rows:
        ref = R.rollout(w, st, tu, 36, SEED, max_plies=3, rotate=True)
    e32 = _e32(O, w, rows)
    bound = max(BOUND, 4 * e32)
    cmp = ~ref["near_tie"]
    assert cmp.mean() >= 0.9, cmp.mean()
    trunc, full = ref["truncated"] & cmp, ~ref["truncated"] & cmp
    assert trunc.sum() > 0 and full.sum() > 0
    np.testing.assert_array_equal(tt[cmp], ref["turns"][cmp])
    np.testing.assert_array_equal(tv[full], ref["value"][full])
    worst = float(np.abs(tv[trunc] - ref["value"][trunc]).max())
    print("NETS-MAX %-13s %-28s %6d trials: max |gpu - fp64| = %.3g, ratio to the numpy fp32 forward's own error %.3g: %.2f"
          % (fam, "rollout truncation value", int(trunc.sum()), worst, e32, worst / e32))
    assert worst <= bound
    # BF16 against its emulation
    ds, dt = N.value_rows()
    X = N.encode(ds, dt)
    v = _np(env.evaluate(ds, dt, precision=bg.BF16))
    assert np.isfinite(v).all() and (v >= 0).all() and (v <= 1).all()
    ref = N.forward_bf16_f64(w, X)
    wb = w.copy()
    wb[:N.O1] = N.bf16_round(w[:N.O1])
    e32 = float(np.abs(N.forward_np32(wb, N.bf16_round(X)).astype(np.float64) - ref).max())
    worst = float(np.abs(v - ref).max())
    print("NETS-MAX %-13s %-28s %6d rows: max |gpu - bf16 emulation| = %.3g, ratio to the numpy fp32 forward's own error %.3g: %.2f"
          % (fam, "evaluate BF16", len(v), worst, e32, worst / e32))
    assert worst <= max(2e-5, 4 * e32)
    assert env.stats()["error_flags"] == 0
    env.close()


def _first_k_search(bg, golden_dir, weights, net, Ks, outcome_ties_with=None):
    """step_search under a net that ties every candidate: the kept states are exactly the first K distinct afterstates in the reference's
    order (terminal candidates first, with their outcome), and the board played is the reference's choice.  -> per K: (v1, v2, kept,
    reference results).  outcome_ties_with: the net's one value when it EQUALS an outcome (out_hi: 1.0, out_lo: 0.0) -- on a lane with
    a terminal candidate of that outcome beside another candidate the board played is held to the documented rule itself (the first
    kept state), not to the fp64 reference, whose own rounding of sum w_r = 1 + 2.2e-16 decides there."""
    st, tu, dice = _lanes(bg, golden_dir, weights, 12, 12, seed=29)
    # two lanes that can bear off their last two checkers or keep one on the board: a terminal candidate beside another one
    st[0] = 0; st[0, 18] = 1; st[0, 23] = 1; st[0, 2] = -2; st[0, 26], st[0, 27] = 13, 13; tu[0] = 0; dice[0] = (6, 1)
    st[1] = 0; st[1, 5] = -1; st[1, 0] = -1; st[1, 20] = 3; st[1, 26], st[1, 27] = 12, 13; tu[1] = 1; dice[1] = (1, 6)
    w, wref = N.table(net), N.reference_table(net)
    out = {}
    n_outcome_ties = 0
    with N.memoized(S, "reply_values"):
        for K in Ks:
            env = _setup(bg, w, st, tu, dice)
            env.step_search(top_k=K, roll=False, auto_reset=False, no_flip=True)
            states, v1, v2, kept = (_np(x) for x in env.search_candidates())
            after = _np(env.states())
            assert env.stats()["error_flags"] == 0
            refs = []
            for i in range(len(st)):
                r = S.search(wref, st[i], int(tu[i]), int(dice[i, 0]), int(dice[i, 1]), K)
                refs.append(r)
                k = len(r["states"])
                assert int(kept[i]) == k, (net, K, i)
                if k == 0:
                    assert (after[i] == st[i]).all()
                    continue
                assert np.array_equal(states[i, :k], r["states"]), (net, K, i)          # the same states in the same order
                t = r["terminal"]
                if outcome_ties_with is not None and (~t).any() and (r["v1"][t] == outcome_ties_with).any():
                    # every kept V2 is exactly the outcome: the documented rule (ties: the smaller key) plays the first kept state.  The
                    # fp64 reference's weights sum to 1 + 2.2e-16 and would prefer a candidate that does NOT end the game, as the
                    # library's earlier fmaf chain (1.0000002) did
                    assert (after[i] == r["states"][0]).all(), (net, K, i)
                    n_outcome_ties += 1
                    continue
                assert (after[i] == r["states"][r["choice"]]).all(), (net, K, i)
            out[K] = (v1, v2, kept, refs)
            if K == 1:                                        # top_k = 1 is the greedy step on every lane that does not end the game
                b = _setup(bg, w, st, tu, dice)
                b.step_greedy(roll=False, auto_reset=False, no_flip=True)
                live = np.array([len(r["states"]) > 0 and not r["terminal"][0] for r in refs])
                assert live.sum() > len(st) // 2 and (_np(b.states())[live] == after[live]).all()
                b.close()
            env.close()
    assert sum(int(r["terminal"].sum()) for r in out[Ks[0]][3]) > 0
    assert outcome_ties_with is None or n_outcome_ties > 0
    return out, st, tu, dice


def _first_candidate_greedy(bg, net):
    """4 096 lanes, 25 greedy steps, then one with want_index, as test_greedy_index_matches_ordered_enumeration: candidate 0 is chosen on
    every lane that has a move, and every row's value is bit-identical to evaluate() of that row."""
    n = 4096
    env = bg.VecGame(n, seed=99, arena_rows=4 << 20)
    env.load_weights(N.table(net))
    for _ in range(25):
        env.step_greedy()
    env.roll()
    pt = _np(env.turns())
    offs, cnts, st, sq, ln = [_np(x) for x in env.enumerate()]
    env.step_greedy(roll=False, auto_reset=False, want_index=True)
    post = _np(env.states())
    lc = env.last_choice()
    ch, cn, val = _np(lc["chosen"]), _np(lc["count"]), _np(lc["value"])
    assert (cn == cnts).all()
    moved = cnts > 0
    assert moved.mean() > 0.9
    assert (ch[moved] == 0).all() and (ch[~moved] == -1).all()
    assert (post[moved] == st[offs[moved]]).all()
    info, ust, uval = [_np(x) for x in env.unique_rows()]
    mover = pt[info[:, 0]]
    ev = np.empty(len(ust), np.float32)
    other = bg.VecGame(64, arena_rows=max(len(ust), 65536))
    other.load_weights(N.table(net))
    for tb in (0, 1):
        if (mover == tb).any():
            ev[mover == tb] = _np(other.evaluate(ust[mover == tb], np.full(int((mover == tb).sum()), tb, np.int32)))
    assert np.array_equal(uval.view(np.uint32), ev.view(np.uint32))
    assert np.array_equal(val[moved].view(np.uint32), np.full(int(moved.sum()), ev[0], np.float32).view(np.uint32))
    assert env.stats()["error_flags"] == 0
    other.close(); env.close()
    return ev


@pytest.mark.parametrize("net,target", [("out_hi", 1.0), ("out_lo", 0.0)])
def test_outputs_that_are_exactly_one_or_zero(bg, O, golden_dir, weights, net, target):
    """b2 = +-200: every evaluator returns exactly 1.0 / 0.0, and the greedy step, the search and a truncated rollout choose as under
    zero_w1.  0.0 for a PLAYER1 mover is the smallest pack best_atomic_max can form: it still has to count as "has a move"."""
    w = N.table(net)
    t32 = np.float32(target)
    st, tu = N.value_rows()
    env = bg.VecGame(4096)
    env.load_weights(w)
    for prec in (bg.F32, bg.F16X2, bg.BF16, bg.F32_DENSE):
        assert (_np(env.evaluate(st, tu, precision=prec)) == t32).all(), prec
    for key, (roots, rt, rows, ri) in N.pair_sets().items():
        assert (_np(env.evaluate_incremental(roots, rt, rows, ri)) == t32).all(), key
    ps, pt = N.preroll_positions()
    f, m = (_np(x) for x in env.evaluate_preroll(ps, pt))
    assert (f == t32).all() and np.abs(m - target).max() <= 1e-12
    # a truncated rollout: cut trials score exactly the target, finished ones their outcome, nothing is a near tie
    rs, rt_ = N.family_rollout_positions()
    r = env.rollout(rs, rt_, 36, max_plies=3, rotate=True, seed=SEED, per_trial=True)
    ref = R.rollout(N.reference_table(net), rs, rt_, 36, SEED, max_plies=3, rotate=True)
    assert not ref["near_tie"].any() and ref["truncated"].any() and (~ref["truncated"]).any()
    np.testing.assert_array_equal(_np(r["trial_turns"]), ref["turns"])
    np.testing.assert_array_equal(_np(r["trial_value"]), ref["value"].astype(np.float32))
    assert (_np(r["trial_value"])[ref["truncated"]] == t32).all()
    assert env.stats()["error_flags"] == 0
    env.close()
    # the greedy step: candidate 0 on every lane with a move, the value exactly the target
    ev = _first_candidate_greedy(bg, net)
    assert (ev == t32).all()
    # the search: the first 8 distinct afterstates in reference order, 1- and 2-ply values exactly the target (or the outcome)
    out, _, _, _ = _first_k_search(bg, golden_dir, weights, net, (8,), outcome_ties_with=target)
    v1, v2, kept, refs = out[8]
    for i, r in enumerate(refs):
        k = len(r["states"])
        want = np.where(r["terminal"], r["v1"], target).astype(np.float32)
        assert np.array_equal(v1[i, :k], want) and np.array_equal(v2[i, :k], want), (net, i, v1[i, :k], v2[i, :k])


# ---- the tie rule, strictly: zero_w1 gives every row the same value -------------------------------------------------------------------

def test_tie_rule_greedy_4096(bg):
    ev = _first_candidate_greedy(bg, "zero_w1")
    c = N.constant_value(N.table("zero_w1"))
    assert (ev == ev[0]).all() and abs(float(ev[0]) - c) <= BOUND


def test_tie_rule_greedy_65536(bg, O, weights):
    """All four arenas and the fused boundary route: run_greedy(30) under the checkpoint spreads the game phases, then zero_w1 is loaded
    into the SAME env.  After one step_greedy and after one step inside run_greedy(8) (seen through a twin that takes 7 fused steps and
    one separate step, as _greedy_65536_sampled_lanes does) the board of ~255 sampled lanes EQUALS the oracle's candidate 0."""
    n = 65536
    wz = N.table("zero_w1")
    a, b = bg.VecGame(n, seed=777), bg.VecGame(n, seed=777)
    a.load_weights(weights); b.load_weights(weights)
    a.run_greedy(30); b.run_greedy(30)
    a.load_weights(wz); b.load_weights(wz)
    lanes = list(range(5, n, 257))
    pre, pt = _np(a.states()), _np(a.turns())
    assert np.array_equal(pre, _np(b.states())) and np.array_equal(pt, _np(b.turns()))
    frozen = (_np(a.flags()) & 4) != 0
    a.step_greedy(auto_reset=False); b.step_greedy(auto_reset=False)
    post, dice = _np(a.states()), _np(a.dice())
    assert np.array_equal(post, _np(b.states()))
    checked = [l for l in lanes if not frozen[l]]
    _check_greedy_step(O, wz, pre, pt, dice, post, checked, strict=True)
    a.run_greedy(8, auto_reset=False)
    b.run_greedy(7, auto_reset=False)
    pre, pt = _np(b.states()), _np(b.turns())
    frozen = (_np(b.flags()) & 4) != 0
    b.step_greedy(auto_reset=False)
    post, dice = _np(a.states()), _np(a.dice())
    assert np.array_equal(post, _np(b.states())) and np.array_equal(_np(a.turns()), _np(b.turns()))
    checked2 = [l for l in lanes if not frozen[l]]
    _check_greedy_step(O, wz, pre, pt, dice, post, checked2, strict=True)
    assert len(checked) > 200 and len(checked2) > 150
    assert a.stats()["error_flags"] == 0 and b.stats()["error_flags"] == 0
    a.close(); b.close()


def test_tie_rule_search(bg, golden_dir, weights):
    w = N.table("zero_w1")
    c = N.constant_value(w)
    probe = bg.VecGame(64)
    probe.load_weights(w)
    c32 = _np(probe.evaluate(np.zeros((1, 28), np.int32), [0]))[0]
    probe.close()
    out, st, tu, dice = _first_k_search(bg, golden_dir, weights, "zero_w1", (0, 1, 3, 8))
    for K, (v1, v2, kept, refs) in out.items():
        for i, r in enumerate(refs):
            k = len(r["states"])
            if k == 0:
                continue
            t = r["terminal"]
            assert t[:int(t.sum())].all()                                             # terminal candidates rank first ...
            assert np.array_equal(v1[i, :k][t], r["v1"][t].astype(np.float32))         # ... with their outcome, at both plies
            assert np.array_equal(v2[i, :k][t], r["v1"][t].astype(np.float32))
            assert (v1[i, :k][~t].view(np.uint32) == c32.view(np.uint32)).all(), (K, i)  # v1 == c bit for bit
            assert (np.abs(v2[i, :k][~t].astype(np.float64) - c) <= 1e-6).all(), (K, i)  # fp32 rounding of (sum doubles + 2 sum others) / 36
            if K in (3, 8) and not t.any():
                assert np.array_equal(r["keys"], np.arange(k))                         # (the reference itself: the first K by index)


@pytest.fixture(scope="module")
def tie_rollout_reference():
    st, tu = N.tie_rollout_positions()
    w = N.table("zero_w1")
    with N.memoized(V, "preroll"):
        vr = V.rollout(w, st, tu, 72, SEED, max_plies=16, rotate=True)
    plain = R.rollout(w, st, tu, 72, SEED, max_plies=16, rotate=True)
    return st, tu, plain, vr


@pytest.mark.parametrize("variance_reduction", [False, True])
def test_tie_rule_rollout(bg, tie_rollout_reference, variance_reduction):
    """EVERY trial is compared: with all values equal the reference flags no near tie, so nothing is left out."""
    st, tu, plain, vr = tie_rollout_reference
    ref = vr if variance_reduction else plain
    w = N.table("zero_w1")
    c = N.constant_value(w)
    assert not ref["near_tie"].any()
    assert ref["truncated"].any() and (~ref["truncated"]).any()
    env = bg.VecGame(64)
    env.load_weights(w)
    r = {k: _np(v) for k, v in env.rollout(st, tu, 72, max_plies=16, rotate=True, seed=SEED, per_trial=True,
                                           variance_reduction=variance_reduction).items()}
    np.testing.assert_array_equal(r["trial_turns"], ref["turns"])
    fin = ~ref["truncated"]
    np.testing.assert_array_equal(r["trial_value"][fin], ref["value"][fin].astype(np.float32))
    assert (np.abs(r["trial_value"][~fin].astype(np.float64) - c) <= 1e-6).all()
    np.testing.assert_array_equal(r["truncated"], ref["truncated"].sum(1))
    if variance_reduction:
        assert (np.abs(r["trial_luck"] - ref["luck"]) <= 1e-6).all()
    assert env.stats()["error_flags"] == 0
    env.close()


# ---- a reload reaches the scratch envs ------------------------------------------------------------------------------------------------

def _analysis_calls(bg, env, slot, st, tu, dice):
    """step_search, evaluate_preroll, rollout (plain and luck-adjusted) and rollout_moves once each on a one-lane env, with sizes that fit
    the scratch envs the first round of calls leaves behind (every rollout here has at most 256 trials: one 256-lane scratch env)
    -> everything they return, as numpy.  (rollout_moves plays with slot 0 only: it is left out for slot 1.)"""
    from backgammon_env.analysis import rollout_moves
    out = {}
    env.set_states(st[5:6], tu[5:6])
    env.set_dice(dice[5:6])
    env.step_search(top_k=4, roll=False, auto_reset=False, no_flip=True, slot=slot)
    for k, x in zip(("s_states", "s_v1", "s_v2", "s_kept"), env.search_candidates()):
        out[k] = _np(x)
    out["s_after"] = _np(env.states())
    out["s_value"] = _np(env.last_choice()["value"])
    f, m = env.evaluate_preroll(st[:16], tu[:16], slot=slot)
    out["p_f"], out["p_m"] = _np(f), _np(m)
    for vr in (False, True):
        r = env.rollout(st[:4], tu[:4], 36, max_plies=5, rotate=True, seed=SEED, slot=slot, per_trial=True, variance_reduction=vr)
        out.update({"r%d_%s" % (vr, k): _np(v) for k, v in r.items()})
        out["r%d_lanes" % vr] = np.asarray(env.rollout_info()[0])
    if slot == 0:
        for vr in (False, True):
            res = rollout_moves(env, st[7], int(tu[7]), dice[7], top_k=3, trials=36, max_plies=5, seed=SEED, variance_reduction=vr)
            assert len(res) > 0
            for j, cnd in enumerate(res):
                for k, v in cnd.items():
                    out["m%d_%d_%s" % (vr, j, k)] = np.asarray(v, dtype=np.float64)
    return out


def _same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def test_reload_reaches_the_scratch_envs(bg, golden_dir, weights):
    """A scratch env borrows its parent's tables: weights loaded AFTER the scratch envs exist must be the ones the next search, pre-roll
    evaluation and rollout use.  Every output is bit-identical to that of a fresh env that only ever held that table in that slot.
    What this can and cannot catch: bgamd_env_load_weights copies into the env's existing device buffers, and a scratch env holds
    pointers to those, so the DATA of a reloaded slot cannot go stale whatever scratch_env() does; what the per-call assignment carries
    is the struct's own fields -- has_weights (slot 1 is first loaded here AFTER the scratch envs exist: a scratch env that kept its
    first copy answers BGAMD_E_NOWEIGHTS) and any table pointer a later version might re-allocate."""
    st, tu, dice = _lanes(bg, golden_dir, weights, 16, 4, seed=37)
    tables = {0: N.table("normal"), 1: N.table("xavier")}

    def fresh(w, slot):
        e = bg.VecGame(1, seed=3)
        e.load_weights(w, slot=slot)
        out = _analysis_calls(bg, e, slot, st, tu, dice)
        e.close()
        return out
    want = {slot: fresh(w, slot) for slot, w in tables.items()}
    want_ckpt = fresh(weights, 0)
    env = bg.VecGame(1, seed=3)
    env.load_weights(weights)
    first = _analysis_calls(bg, env, 0, st, tu, dice)                 # both scratch envs exist from here on
    _same(first, want_ckpt, "checkpoint, before any reload")
    lanes = env.rollout_info()[0]
    env.load_weights(tables[0], slot=0)
    env.load_weights(tables[1], slot=1)
    for slot in (0, 1):
        got = _analysis_calls(bg, env, slot, st, tu, dice)
        _same(got, want[slot], "slot %d after the reload" % slot)
        assert env.rollout_info()[0] == lanes                          # the scratch envs were reused, not re-created
    assert not np.array_equal(want[0]["p_f"], want_ckpt["p_f"]) and not np.array_equal(want[1]["p_f"], want[0]["p_f"])
    env.load_weights(weights, slot=0)
    _same(_analysis_calls(bg, env, 0, st, tu, dice), want_ckpt, "checkpoint loaded back")
    assert env.rollout_info()[0] == lanes
    assert env.stats()["error_flags"] == 0
    env.close()
