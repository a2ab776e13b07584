"""The conditions tests/test_gpu_search3.py rests on, without a GPU:
  (1) tests/search3_model.py -- the deep set, the replies a mid lane keeps, the pass reply, "a single reply is still searched", R3, V3
      and the choice -- against a plain-Python restatement of the WHOLE tree of bgamd_env_step_search3's items 1-5, level by level, on
      the oracle's afterstates (search_ref.distinct_afterstates) and the numpy float32 forward pass (nets.forward_np32, the arithmetic of
      search_lanes.np32_values), under the checkpoint and the dyadic table;
  (2) three deliberately wrong models each fail that comparison;
  (3) the census, by the oracle, of the lane set the GPU tests use: every class of lane and of mid lane they must meet is there.
Both sides of (1) take their afterstates and raw net values from one cache (Tree.scored / Tree.net1), so a float32 BLAS product that sums
one row in two orders cannot come between them: what is compared is the rule."""
import numpy as np
import pytest

import filter_model as F
import nets as N
import search3_model as S3
import search_lanes as L
import search_model as M
import search_ref as S

INF = float("inf")
# (top_k, margin, deep_k, deep_margin, reply_top_k, reply_margin): the parameter sets of the GPU tests
WIDE = (3, INF, 2, INF, 2, INF)
NARROW = (3, 0.08, 0, 0.01, 0, 0.01)
PARAMS = (WIDE, NARROW)
TREE_PARAMS = (WIDE, (2, 0.08, 2, 0.02, 2, 0.01))         # the whole-tree check: top_k <= 3, deep_k <= 2, reply_top_k <= 2
N_G10 = 288                    # the GPU tests' lane set: G10's first boards and the hand-built ones


def hand_built():
    """Boards G10 has none of, or too few -> (boards [7, 28], mover [7], dice [7, 2]).
    [0], [1], [2]: the opponent sits on the bar against the mover's closed home board, which the mover's candidates keep closed: no reply
    on any roll, doubles or not (PLAYER1 to move twice, PLAYER2 once).  [3], [4]: the mover cannot finish, the opponent bears its last
    checker off with any roll: every reply is terminal.  [5]: the mover on the bar against a closed board: a lane without a move.
    [6]: PLAYER1 bears its last two checkers off with the 3 and the 1 played one way, not the other: a terminal candidate beside another."""
    (a, _, c, _), _ = N.closed_board_positions()
    e = np.zeros(28, np.int32); e[18] = 3; e[26] = 12; e[0] = -1; e[27] = 14
    f = np.zeros(28, np.int32); f[5] = -3; f[27] = 12; f[23] = 1; f[26] = 14
    g = np.zeros(28, np.int32); g[21] = 1; g[23] = 1; g[26] = 13; g[0:3] = -1; g[27] = 12
    boards = np.array([c, c, a, e, f, a, g], np.int32)
    mover = np.array([0, 0, 1, 0, 1, 0, 0], np.int32)
    dice = np.array([[1, 2], [3, 3], [1, 2], [1, 2], [1, 2], [1, 2], [3, 1]], np.int32)
    return boards, mover, dice


def lane_set():
    """-> (boards [n, 28], mover [n], dice [n, 2]), n = N_G10 + 7"""
    st, tu, dice = L.g10()
    hb, ht, hd = hand_built()
    return np.concatenate([st[:N_G10], hb]), np.concatenate([tu[:N_G10], ht]), np.concatenate([dice[:N_G10], hd])


class Tree:
    """The afterstates of (position, side to move, dice) from the oracle with their RAW float32 net values (no outcome), and the net's
    value of a single position: computed once per key.  On top of them, with numpy and the models: v1, the greedy reply, V2, a mid lane's
    replies and R3 -- what search3_model.lane is fed with."""

    _after = {}                                            # (position, side, dice) -> afterstates: the same under every net

    def __init__(self, w):
        self.w = np.asarray(w, np.float32)
        self._scored, self._net1, self._v2 = {}, {}, {}

    def scored(self, s28, side, d1, d2):
        s28 = np.ascontiguousarray(s28, dtype=np.int32)
        key = (s28.tobytes(), int(side), int(d1), int(d2))
        if key not in self._scored:
            if key not in Tree._after:
                Tree._after[key] = np.ascontiguousarray(S.distinct_afterstates(s28, int(side), int(d1), int(d2)), dtype=np.int32).reshape(-1, 28)
            rows = Tree._after[key]
            vals = N.forward_np32(self.w, N.encode(rows, np.full(len(rows), side))).astype(np.float32) if len(rows) else np.zeros(0, np.float32)
            self._scored[key] = (rows, vals)
        return self._scored[key]

    def net1(self, s28, side):
        s28 = np.ascontiguousarray(s28, dtype=np.int32)
        key = (s28.tobytes(), int(side))
        if key not in self._net1:
            self._net1[key] = np.float32(N.forward_np32(self.w, N.encode(s28[None], np.array([side])))[0])
        return self._net1[key]

    @staticmethod
    def with_outcomes(rows, vals, side):
        term = rows[:, 26 + int(side)] == 15
        v = vals.copy()
        v[term] = np.float32(1.0 if int(side) == 0 else 0.0)
        return v, term

    def v2(self, c, mover):
        """V2 of the afterstate c of `mover` (item 4 of the 2-ply search): the opponent's greedy reply or no-move value, roll by roll"""
        key = (np.ascontiguousarray(c, dtype=np.int32).tobytes(), int(mover))
        if key not in self._v2:
            opp = 1 - int(mover)
            R = np.empty(21, np.float32)
            for r, (a, b) in enumerate(S.ROLLS):
                rows, vals = self.scored(c, opp, a, b)
                R[r] = S3.best_for(vals, opp) if len(rows) else self.net1(c, opp)
            self._v2[key] = M.v2_from_replies(R)
        return self._v2[key]

    def replies(self, c, o, r):
        """the mid lane (c, o to move, roll r) -> (rows, v1 with outcomes, terminal, no_move: the one reply is c itself)"""
        rows, vals = self.scored(c, o, *S.ROLLS[r])
        if len(rows) == 0:
            return np.asarray(c, np.int32)[None], np.array([self.net1(c, o)], np.float32), np.zeros(1, bool), True
        v1, term = self.with_outcomes(rows, vals, o)
        return rows, v1, term, len(rows) == 1 and bool((rows[0] == c).all())

    def lane(self, s28, mover, d1, d2, params, r3_fn=S3.r3, pass_by_net=False, deep_rank_by_v1=False):
        """search3_model.lane over this tree -> (its result, the lane's afterstates, their terminal flags)"""
        top_k, margin, deep_k, deep_margin, rk, rmg = params
        mover = int(mover)
        rows, vals = self.scored(s28, mover, d1, d2)
        v1, term = self.with_outcomes(rows, vals, mover)

        def r3_of(c):
            out = np.empty(21, np.float32)
            for r in range(21):
                rr, rv1, rterm, no_move = self.replies(rows[c], 1 - mover, r)
                if pass_by_net and no_move:            # WRONG: the roll without a move at the net's value of c
                    out[r] = rv1[0]
                else:
                    out[r] = r3_fn(rv1, rterm, lambda d: self.v2(rr[d], 1 - mover), 1 - mover, rk, rmg)[0]
            return out
        res = S3.lane(v1, term, mover, top_k, margin, deep_k, deep_margin, lambda c: self.v2(rows[c], mover), r3_of,
                      deep_rank_by_v1=deep_rank_by_v1)
        return res, rows, term


# ---- the whole tree in plain Python: no numpy arithmetic, no sort of arrays, no model ---------------------------------------------------

_f32 = F._f32


def _mean21(R):
    sd = so = 0.0
    for (a, b), x in zip(S.ROLLS, R):
        if a == b:
            sd = _f32(sd + x)
        else:
            so = _f32(so + x)
    return _f32(_f32(sd + _f32(2.0 * so)) * _f32(1.0 / 36.0))


def _filter(items, side, k, margin):
    """items: [(index, value)] -> the indices kept, best first: rank by (value for side, smaller index) < k (0: no limit) and one fp32
    subtraction from rank 0 <= margin; rank 0 always"""
    order = sorted(items, key=lambda t: (-t[1] if side == 0 else t[1], t[0]))
    out = []
    for rank, (i, v) in enumerate(order):
        d = _f32(order[0][1] - v) if side == 0 else _f32(v - order[0][1])
        assert d >= 0.0
        if (k == 0 or rank < k) and (rank == 0 or d <= float(np.float32(margin))):
            out.append(i)
    return out


def _best(items, side):
    """[(index, value)] -> the (index, value) best for side, the smaller index on a tie"""
    return sorted(items, key=lambda t: (-t[1] if side == 0 else t[1], t[0]))[0]


def whole_tree(tree, s28, mover, d1, d2, params):
    """bgamd_env_step_search3's items 1-5 restated -> (choice, value, {c: V3})"""
    top_k, margin, deep_k, deep_margin, rk, rmg = params
    mover = int(mover)

    def valued(pos, side, a, b):                           # [(row, v1, terminal)]: outcomes in place
        rows, vals = tree.scored(pos, side, a, b)
        out = []
        for row, v in zip(rows, vals):
            t = int(row[26 + side]) == 15
            out.append((row, (1.0 if side == 0 else 0.0) if t else float(v), t))
        return out

    def V2(c, mv):                                         # c: an afterstate of mv
        opp, R = 1 - mv, []
        for a, b in S.ROLLS:
            rows, vals = tree.scored(c, opp, a, b)
            if len(rows) == 0:
                R.append(float(tree.net1(c, opp)))
            else:
                R.append(max(float(v) for v in vals) if opp == 0 else min(float(v) for v in vals))
        return _mean21(R)

    cands = valued(s28, mover, d1, d2)
    L1 = _filter([(i, v) for i, (_, v, _) in enumerate(cands)], mover, top_k, margin)
    if not L1:
        return -1, None, {}
    if len(L1) == 1:
        return L1[0], cands[L1[0]][1], {}
    v2 = {c: cands[c][1] if cands[c][2] else V2(cands[c][0], mover) for c in L1}
    L2 = _filter([(c, v2[c]) for c in L1], mover, deep_k, deep_margin)
    if len(L2) == 1:
        return L2[0], v2[L2[0]], {}
    o, v3 = 1 - mover, {}
    for c in L2:
        if cands[c][2]:
            v3[c] = cands[c][1]
            continue
        R3 = []
        for a, b in S.ROLLS:
            replies = valued(cands[c][0], o, a, b)
            if not replies:                                # the pass: c itself, at the net's value with o's turn bit
                replies = [(cands[c][0], float(tree.net1(cands[c][0], o)), False)]
            kept = _filter([(i, v) for i, (_, v, _) in enumerate(replies)], o, rk, rmg)
            searched = [(i, replies[i][1] if replies[i][2] else V2(replies[i][0], o)) for i in kept]       # a single one too
            R3.append(_best(searched, o)[1])
        v3[c] = _mean21(R3)
    choice, value = _best(list(v3.items()), mover)
    return choice, value, v3


# ---- (1), (2) --------------------------------------------------------------------------------------------------------------------------

TREE_LANES = tuple(range(0, 20, 2))                        # 10 G10 boards and the hand-built ones


def _tree_lanes():
    st, tu, dice = lane_set()
    idx = list(TREE_LANES) + list(range(N_G10, len(st)))
    return st[idx], tu[idx], dice[idx]


_trees = {}


def tree_of(net, weights):
    if net not in _trees:
        _trees[net] = Tree(weights if net == "ckpt" else L.dyadic())
    return _trees[net]


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _agrees(tree, st, tu, dice, params, **wrong):
    """lanes on which the model (or a wrong one) gives the restatement's choice, value and V3 list, bit for bit -> bool [n]"""
    ok = []
    for s, t, d in zip(st, tu, dice):
        res, _, _ = tree.lane(s, t, d[0], d[1], params, **wrong)
        choice, value, v3 = whole_tree(tree, s, t, d[0], d[1], params)
        same = res["choice"] == choice
        if choice >= 0:
            same = same and _u32(res["value"]) == _u32(value)
            same = same and sorted(v3) == sorted(res["deep"].tolist() if len(res["v3"]) else [])
            same = same and all(_u32(v3[c]) == _u32(x) for c, x in zip(res["deep"].tolist(), res["v3"]))
        ok.append(bool(same))
    return np.array(ok)


@pytest.mark.parametrize("net", ["ckpt", "dyadic"])
def test_model_against_the_whole_tree(weights, net):
    tree = tree_of(net, weights)
    st, tu, dice = _tree_lanes()
    deep = 0
    for params in TREE_PARAMS:
        ok = _agrees(tree, st, tu, dice, params)
        assert ok.all(), (net, params, np.where(~ok)[0].tolist())
        deep += sum(len(tree.lane(s, t, d[0], d[1], params)[0]["v3"]) >= 2 for s, t, d in zip(st, tu, dice))
    assert deep >= 10                                      # lanes that reached the third level


WRONG = {"single_reply_at_v1": dict(r3_fn=S3.r3_single_at_v1), "no_move_by_the_net": dict(pass_by_net=True),
         "deep_set_by_v1": dict(deep_rank_by_v1=True)}


@pytest.mark.parametrize("name", sorted(WRONG))
def test_wrong_models_fail(weights, name):
    tree = tree_of("ckpt", weights)
    st, tu, dice = _tree_lanes()
    ok = np.concatenate([_agrees(tree, st, tu, dice, params, **WRONG[name]) for params in TREE_PARAMS])
    assert not ok.all(), name


# ---- (3) the census ----------------------------------------------------------------------------------------------------------------------

def census(tree, st, tu, dice, params):
    """Lane and mid-lane classes of a lane set under one parameter set, by the tree's own values -> dict of counts: deep (|L2| >= 2),
    deep_cut (searched at 2 plies, the deep filter leaves one), singleton (one candidate kept of two or more, or forced), no_move (a lane
    without a move), terminal_candidate (in L2 of a deep lane), and over the mid lanes of the deep lanes: pass_plain / pass_doubles (the
    opponent has no move on a non-doubles / doubles roll), terminal_reply (a kept reply is terminal)."""
    out = dict(deep=0, deep_cut=0, singleton=0, no_move=0, terminal_candidate=0, pass_plain=0, pass_doubles=0, terminal_reply=0)
    _, _, _, _, rk, rmg = params
    for s, t, d in zip(st, tu, dice):
        res, rows, term = tree.lane(s, t, d[0], d[1], params, r3_fn=lambda v1, *a: (np.float32(0), None))       # (no third level here)
        out["no_move"] += len(res["kept"]) == 0
        out["singleton"] += len(res["kept"]) == 1
        out["deep_cut"] += len(res["kept"]) >= 2 and len(res["deep"]) == 1
        if len(res["deep"]) < 2:
            continue
        out["deep"] += 1
        out["terminal_candidate"] += bool(term[res["deep"]].any())
        for c in res["deep"]:
            if term[c]:
                continue
            for r, (a, b) in enumerate(S.ROLLS):
                _, rv1, rterm, no_move = tree.replies(rows[c], 1 - int(t), r)
                out["pass_doubles" if a == b else "pass_plain"] += no_move
                out["terminal_reply"] += bool(rterm[S3.reply_set(rv1, 1 - int(t), rk, rmg)].any())
    return out


def test_census_of_the_gpu_lane_set(weights):
    tree = tree_of("ckpt", weights)
    st, tu, dice = lane_set()
    seen = {}
    for params in PARAMS:
        c = census(tree, st, tu, dice, params)
        print("CENSUS", params, c)
        for k, v in c.items():
            seen[k] = seen.get(k, 0) + v
    assert all(seen[k] >= 1 for k in seen), seen
    assert seen["deep"] >= 200 and seen["deep_cut"] >= 20 and seen["singleton"] >= 20
