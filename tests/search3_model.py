"""An exact model of what the 3-ply search step adds to the filtered 2-ply one (bgamd_env_step_search3, csrc/bg_search3.h): the deep set
L2 of a searched lane, the replies a mid lane keeps -- with the pass reply of an opponent who cannot move, and a single kept reply searched
like any other --, R3, V3 and the choice.  Built on tests/search_model.py (order, the 21-roll sum, the choice) and tests/filter_model.py (the
margin rule), which are not restated; numpy float32 and integers only.  No net is evaluated here: every value comes from the caller -- the
device's own, or a reference's cast to float32 -- so what is modelled is the RULE, bit for bit.

A lane's candidates are its distinct afterstates in reference order, and so are a mid lane's replies; `index` arrays hold reference-order
indices, which order equal values as the device's keys do."""
import numpy as np

import filter_model as F
import search_model as M


def deep_set(kept, v2, mover, deep_k, deep_margin):
    """Item 2.  kept [k]: the kept candidates' reference-order indices; v2 [k]: their float32 2-ply values -> L2, best V2 first: ranked by
    (V2 for the mover, smaller index), rank < deep_k (0 = no limit) and one fp32 subtraction from rank 0 <= deep_margin; rank 0 always."""
    return F.select(kept, v2, mover, deep_k, deep_margin)


def reply_set(v1, o, reply_top_k, reply_margin):
    """Item 4's kept replies.  v1 [m]: the float32 1-ply values of a mid lane's replies in reference order (m >= 1: an opponent without a
    move has ONE reply, the pass, which the caller lists) -> their indices, best v1 for o first: the filter's rule with o as the mover."""
    assert len(v1) >= 1
    return F.select(np.arange(len(v1)), v1, o, reply_top_k, reply_margin)


def best_for(values, side):
    """the best float32 value for `side`: max for PLAYER1, min for PLAYER2 (through the bit patterns, as srch_pack orders them)"""
    v = np.ascontiguousarray(values, dtype=np.float32)
    b = M.bits(v)
    return v[int(np.argmax(b) if int(side) == 0 else np.argmin(b))]


def r3(v1, terminal, v2_of, o, reply_top_k, reply_margin):
    """R3 of one mid lane.  v1 [m], terminal [m] (o has borne off its 15th checker: v1 is the outcome) of its replies in reference order;
    v2_of(d) -> the float32 V2 of reply d (m's 21 rolls, roles swapped).  EVERY kept reply is searched, a single one too; a terminal one
    keeps its outcome -> (R3 float32, the kept replies' indices)."""
    kept = reply_set(v1, o, reply_top_k, reply_margin)
    v2 = np.array([v1[d] if terminal[d] else v2_of(int(d)) for d in kept], np.float32)
    return best_for(v2, o), kept


v3_from_r3 = M.v2_from_replies          # item 3: srch_reduce_kernel's expression over the 21 values of R3 in roll order


def lane(v1, terminal, mover, top_k, margin, deep_k, deep_margin, v2_of, r3_of, deep_rank_by_v1=False):
    """One lane, all three levels.  v1 [m], terminal [m]: its distinct afterstates' float32 1-ply values (a terminal one: the outcome) in
    reference order; v2_of(c) -> float32 V2 of candidate c; r3_of(c) -> float32 [21], R3(c, r) in roll order.  -> dict:
      kept   L1, best v1 first            v2     of L1 (a singleton: its v1)
      deep   L2, best V2 first ([] unless the lane was searched at 2 plies)
      v3     of L2 ([] unless |L2| >= 2)
      choice the index played (-1: no move), value: its deepest value, depth [len(kept)]: 1, 2 or 3 per kept candidate.
    deep_rank_by_v1: the WRONG model that ranks the deep set by v1."""
    v1 = np.ascontiguousarray(v1, dtype=np.float32)
    kept = F.select(np.arange(len(v1)), v1, mover, top_k, margin)
    none = np.zeros(0, np.float32)
    out = dict(kept=kept, v2=none, deep=np.zeros(0, np.int64), v3=none, choice=-1, value=np.float32(0), depth=np.zeros(0, np.int32))
    if len(kept) == 0:
        return out
    if len(kept) == 1:
        out.update(v2=v1[kept], choice=int(kept[0]), value=v1[kept[0]], depth=np.ones(1, np.int32))
        return out
    v2 = np.array([v1[c] if terminal[c] else v2_of(int(c)) for c in kept], np.float32)
    deep = deep_set(kept, v1[kept] if deep_rank_by_v1 else v2, mover, deep_k, deep_margin)
    out.update(v2=v2, deep=deep, depth=np.full(len(kept), 2, np.int32))
    if len(deep) == 1:
        j = int(np.where(kept == deep[0])[0][0])
        out.update(choice=int(deep[0]), value=v2[j])
        return out
    v3 = np.array([v1[c] if terminal[c] else v3_from_r3(r3_of(int(c))) for c in deep], np.float32)
    j = M.choose(deep, v3, mover)
    out["depth"][np.isin(kept, deep)] = 3
    out.update(v3=v3, choice=int(deep[j]), value=v3[j])
    return out


def info(lanes, terminal_lists):
    """bgamd_env_search3_info's first five counts from lane() results and each lane's terminal [m]: lanes with a move, searched at 2 plies,
    searched at 3 plies, deep candidates, mid lanes"""
    out = [0, 0, 0, 0, 0]
    for r, term in zip(lanes, terminal_lists):
        out[0] += len(r["kept"]) >= 1
        out[1] += len(r["kept"]) >= 2
        if len(r["deep"]) >= 2:
            out[2] += 1
            out[3] += len(r["deep"])
            out[4] += 21 * int((~np.asarray(term, bool)[r["deep"]]).sum())
    return [int(x) for x in out]


# ---- deliberately wrong models: the whole-tree check must tell each from the model -------------------------------------------------------

def r3_single_at_v1(v1, terminal, v2_of, o, reply_top_k, reply_margin):
    """a single kept reply is left at its v1, as the filtered step leaves a singleton lane"""
    kept = reply_set(v1, o, reply_top_k, reply_margin)
    if len(kept) == 1:
        return np.float32(v1[kept[0]]), kept
    return r3(v1, terminal, v2_of, o, reply_top_k, reply_margin)
