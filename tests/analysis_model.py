"""An exact model of the move analysis' rule (bgamd_env_analyze_moves, csrc/bg_analysis.h) on top of the search's model
(tests/search_model.py): which candidates are kept when the played one is forced in, where the played one stands at 1 and at 2 plies,
which candidate is best and what the error is.  No net is evaluated here: a lane's v1 and V2 come from the caller as float32 arrays
by REFERENCE INDEX (search_ref.distinct_afterstates' order), so what is modelled is the rule, bit for bit.

Also the played families of the tests: which candidate of a lane counts as played, by its v1 rank."""
import numpy as np

import search_model as M

FIELDS = ("status", "distinct", "rank1", "rank2", "v1_played", "v1_best", "v2_played", "v2_best", "error")
FAMILIES = ("best", "inside", "first_out", "worst", "v2best")
OK, IDLE, NO_MOVE, NOT_FOUND = 0, 1, 2, 3


def _zeros():
    out = {k: np.float32(0) if k.startswith("v") or k == "error" else 0 for k in FIELDS}
    out.update(best=-1, kept=np.zeros(0, np.int64))
    return out


def analyse(v1, v2, mover, top_k, played, takes_part=True):
    """One lane.  v1, v2: float32 [m] by reference index (m = 0: no move); mover 0 | 1; top_k (0 = all); played: the reference index of
    the played afterstate, -1 when it is none of the lane's.  -> dict: FIELDS as the device reports them, best (reference index of the
    afterstate with v2_best, -1: none) and kept (the kept reference indices, best v1 first)."""
    v1, v2 = np.ascontiguousarray(v1, np.float32), np.ascontiguousarray(v2, np.float32)
    m = len(v1)
    out = _zeros()
    if not takes_part:
        out["status"] = IDLE
        return out
    if m == 0:
        out["status"] = NO_MOVE
        return out
    idx = np.arange(m)
    order = M.select(idx, v1, mover, 0)
    kept = M.select(idx, v1, mover, top_k)
    out["distinct"] = m
    if played < 0:
        out.update(status=NOT_FOUND, rank1=-1, rank2=-1)
    else:
        out["rank1"] = int(np.where(order == played)[0][0])
        if played not in kept:
            kept = np.concatenate([kept, [played]])
    best = int(kept[M.choose(kept, v2[kept], mover)])
    out.update(kept=kept, best=best, v1_best=v1[order[0]], v2_best=v2[best])
    if played >= 0:
        by_v2 = M.select(kept, v2[kept], mover, 0)           # the kept candidates in the (V2 for the mover, smaller index) order
        out["rank2"] = int(np.where(by_v2 == played)[0][0])
        out.update(v1_played=v1[played], v2_played=v2[played])
        out["error"] = np.float32(v2[best] - v2[played]) if int(mover) == 0 else np.float32(v2[played] - v2[best])
    return out


def played_index(family, v1, v2, mover, top_k):
    """The reference index of the candidate a family plays on a lane with the values v1, v2 (m >= 1): best = v1 rank 0, inside = rank
    top_k - 1, first_out = rank top_k, worst = the last rank, v2best = the best V2 over all.  A lane without that rank plays its worst."""
    order = M.select(np.arange(len(v1)), v1, mover, 0)
    if family == "v2best":
        return int(order[M.choose(order, np.asarray(v2, np.float32)[order], mover)])
    r = {"best": 0, "inside": top_k - 1, "first_out": top_k, "worst": len(order) - 1}[family]
    return int(order[r] if 0 <= r < len(order) else order[-1])


def summary(results, movers):
    """the twelve numbers of d_summary from per-lane model results: counts exact, the sums by math.fsum"""
    import math
    out = [0.0] * 12
    for side in (0, 1):
        rs = [r for r, t in zip(results, movers) if r["status"] == OK and int(t) == side]
        err = [float(r["error"]) for r in rs]
        out[5 * side:5 * side + 5] = [len(rs), sum(r["distinct"] >= 2 for r in rs), sum(e > 0 for e in err), math.fsum(err), max(err, default=0.0)]
    out[10] = sum(r["status"] == NO_MOVE for r in results)
    out[11] = sum(r["status"] == NOT_FOUND for r in results)
    return out
