"""An exact model of the move filter of the filtered 2-ply search step (bgamd_env_step_search_filtered, csrc/bg_filter.h): which of a
lane's distinct afterstates flt_select_kernel keeps.  Built on tests/search_model.py's ordering and ONE float32 subtraction per
candidate; numpy float32 and integers only -- the values come from the caller, so what is modelled is the RULE, bit for bit.

  d(c) = v1(rank 0) - v1(c) for mover PLAYER1, v1(c) - v1(rank 0) for mover PLAYER2: one fp32 subtraction, never negative;
  kept iff rank < top_k (0 = no limit) and d(c) <= margin; rank 0 is always kept; the kept list stays best v1 first.

Also the classes of lanes the tests must meet (census) and the margins that hit d(c) == margin exactly on a lane set (equality_margins)."""
import struct

import numpy as np

import search_model as M


def margin_distances(order_index, v1_bits, mover, top_k):
    """-> (the indices select() of search_model keeps, best first; d of each as float32)"""
    idx = np.asarray(order_index, np.int64)
    v = np.ascontiguousarray(v1_bits)
    v = v.view(np.float32) if v.dtype == np.uint32 else v.astype(np.float32)
    pos = M._best_first(idx, v, mover)
    pos = pos[:top_k] if top_k else pos
    assert np.array_equal(idx[pos], M.select(idx, v, mover, top_k))
    vk = v[pos]
    if len(vk) == 0:
        return idx[pos], np.zeros(0, np.float32)
    d = (vk[0] - vk) if int(mover) == 0 else (vk - vk[0])              # float32 - float32 -> float32: one rounding
    assert d.dtype == np.float32
    return idx[pos], d


def select(order_index, v1_bits, mover, top_k, margin):
    """order_index [m], v1_bits [m], mover, top_k as search_model.select; margin: a float >= 0 (may be inf), taken as float32
    -> the kept indices, best first."""
    kept, d = margin_distances(order_index, v1_bits, mover, top_k)
    keep = d <= np.float32(margin)
    if len(keep):
        keep[0] = True
    return kept[keep]


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def select_plain(order_index, v1, mover, top_k, margin):
    """The header's sentence restated in plain Python, candidate by candidate: no sort, no numpy arithmetic.  The difference of two
    float32 values in [0, 1] is formed in double precision (exact whenever their exponents differ by less than 29) and rounded to
    float32 once: the fp32 subtraction."""
    idx = [int(i) for i in order_index]
    v = [float(np.float32(x)) for x in np.asarray(v1, np.float32)]
    mover = int(mover)
    margin = float(np.float32(margin))

    def beats(a, b):                                   # candidate a stands before candidate b
        if v[a] != v[b]:
            return v[a] > v[b] if mover == 0 else v[a] < v[b]
        return idx[a] < idx[b]
    rank = [sum(beats(b, a) for b in range(len(idx))) for a in range(len(idx))]
    if not idx:
        return np.zeros(0, np.int64)
    top = rank.index(0)
    out = []
    for a in range(len(idx)):
        d = _f32(v[top] - v[a]) if mover == 0 else _f32(v[a] - v[top])
        assert d >= 0.0
        if (top_k == 0 or rank[a] < top_k) and (rank[a] == 0 or d <= margin):
            out.append((rank[a], idx[a]))
    return np.array([i for _, i in sorted(out)], np.int64)


# ---- deliberately wrong models: the tests must tell each from select() on their lane sets ---------------------------------------------
# (A subtraction in float64 is not among them: on the reference values of the G10 boards, under the checkpoint and the dyadic table, it
# keeps the same candidates as the float32 one on every lane for every top_k and margin of the tests, so nothing could tell it apart.)

def select_strict(order_index, v1_bits, mover, top_k, margin):
    """`<` in place of `<=`: a candidate exactly at the margin is dropped"""
    kept, d = margin_distances(order_index, v1_bits, mover, top_k)
    keep = d < np.float32(margin)
    if len(keep):
        keep[0] = True
    return kept[keep]


def select_from_last_place(order_index, v1_bits, mover, top_k, margin):
    """the margin is taken from the last place of the top_k cut instead of rank 0: whoever lies within it of THAT value is kept"""
    kept, d = margin_distances(order_index, v1_bits, mover, top_k)
    if len(kept) == 0:
        return kept
    keep = (d[-1] - d).astype(np.float32) <= np.float32(margin)
    keep[0] = True
    return kept[keep]


def select_mover_blind(order_index, v1_bits, mover, top_k, margin):
    """d is formed as for PLAYER1 whoever moves: for PLAYER2 it is never positive and nothing is cut"""
    kept, d = margin_distances(order_index, v1_bits, mover, top_k)
    keep = (d if int(mover) == 0 else -d) <= np.float32(margin)
    if len(keep):
        keep[0] = True
    return kept[keep]


WRONG = {"strict": select_strict, "from_last_place": select_from_last_place, "mover_blind": select_mover_blind}


# ---- the lane sets ----------------------------------------------------------------------------------------------------------------------

def equality_margins(v1_lists, movers, n=2):
    """The n positive values of d that occur on the most lanes (at full width; of equally frequent ones the smaller): margins that a
    candidate sits on EXACTLY.  Under a table whose values tie exactly (nets.dyadic_table) the same differences recur on dozens of lanes."""
    count = {}
    for v1, mover in zip(v1_lists, movers):
        if len(v1) < 2:
            continue
        _, d = margin_distances(np.arange(len(v1)), v1, mover, 0)
        for x in np.unique(d[d > 0]).tolist():
            count[x] = count.get(x, 0) + 1
    best = sorted(count, key=lambda x: (-count[x], x))[:n]
    assert len(best) == n
    return [float(x) for x in best]


def census(v1_lists, movers, terminal, top_k, margin):
    """Over the lanes with a move -> dict of lane counts: lanes, cut (the margin leaves fewer than the top_k cut alone), at_margin (a
    candidate inside the top_k cut has d == margin exactly, margin > 0), made_single (two or more candidates, the top_k cut leaves two or
    more, the margin leaves one), forced (one distinct afterstate), terminal (a terminal candidate among the afterstates; terminal[i]:
    bool [m_i])."""
    out = dict(lanes=0, cut=0, at_margin=0, made_single=0, forced=0, terminal=0)
    for v1, mover, term in zip(v1_lists, movers, terminal):
        m = len(v1)
        if m == 0:
            continue
        kept_k, d = margin_distances(np.arange(m), v1, mover, top_k)
        kept = select(np.arange(m), v1, mover, top_k, margin)
        out["lanes"] += 1
        out["cut"] += len(kept) < len(kept_k)
        out["at_margin"] += bool(margin > 0 and (d == np.float32(margin)).any())
        out["made_single"] += len(kept_k) >= 2 and len(kept) == 1
        out["forced"] += m == 1
        out["terminal"] += bool(np.asarray(term).any())
    return out
