"""The lane sets of the search-rule tests (tests/test_search_model_cpu.py, tests/test_gpu_search_rules.py): fixture G10's arbitrary
boards with their mover and dice, each board's distinct afterstates from the oracle (computed once per process), and the census of
exact ties a list of 1-ply values holds.  A helper module, not a conftest; nothing is read from outside tests/golden."""
import os

import numpy as np

import nets as N
import search_model as M
import search_ref as S

SEARCH_CHUNK = 131072          # csrc/bg_search_plan.h: virtual lanes per scoring pass
DYADIC_SEED = 7


def dyadic():
    return N.dyadic_table(DYADIC_SEED)


_g10 = []


def g10():
    """-> (boards int32 [1500, 28], mover int32 [1500], dice int32 [1500, 2])"""
    if not _g10:
        g = np.load(os.path.join(N.GOLDEN, "g10_arbitrary_boards.npz"))
        _g10.extend((g["boards"].astype(np.int32), g["dice"][:, 0].astype(np.int32), g["dice"][:, 1:].astype(np.int32)))
    return tuple(_g10)


_after = {}


def afterstates(i):
    """board i's distinct afterstates in reference order, int32 [m, 28] (m = 0: no move)"""
    if i not in _after:
        st, tu, dice = g10()
        _after[i] = np.ascontiguousarray(S.distinct_afterstates(st[i], int(tu[i]), int(dice[i, 0]), int(dice[i, 1])), dtype=np.int32).reshape(-1, 28)
    return _after[i]


def counts(n=1500):
    return np.array([len(afterstates(i)) for i in range(n)])


def index_of(cands):
    """state bytes -> reference-order index"""
    return {c.tobytes(): k for k, c in enumerate(np.ascontiguousarray(cands, dtype=np.int32))}


def terminal(cands, mover):
    """the mover has borne off its 15th checker"""
    return np.asarray(cands).reshape(-1, 28)[:, 26 + int(mover)] == 15


def tie_across(v1, mover, place):
    """Do the values (float32 [m], in reference order) tie EXACTLY across the place-th rank -- the place-th best and the next one are
    bit-equal, so the index decides who is kept at top_k = place -- while not all m values are equal?"""
    b = M.bits(v1)
    if len(b) <= place or (b == b[0]).all():
        return False
    srt = np.sort(b)[::-1] if int(mover) == 0 else np.sort(b)
    return bool(srt[place - 1] == srt[place])


def census(v1_lists, movers):
    """over lanes with at least two candidates -> dict: lanes, partial (some but not all values tie), across3, across8 (tie_across),
    complete (all tie), none (no two values tie)"""
    out = dict(lanes=0, partial=0, across3=0, across8=0, complete=0, none=0)
    for v1, mover in zip(v1_lists, movers):
        if len(v1) < 2:
            continue
        b = M.bits(v1)
        u = len(np.unique(b))
        out["lanes"] += 1
        out["complete"] += u == 1
        out["none"] += u == len(b)
        out["partial"] += 1 < u < len(b)
        out["across3"] += tie_across(v1, mover, 3)
        out["across8"] += tie_across(v1, mover, 8)
    return out


def np32_values(w, boards):
    """the numpy float32 forward pass (nets.forward_np32's arithmetic) over the afterstates of each board of `boards`, terminal candidates
    at their outcome -> list of float32 [m_i] in reference order"""
    tu = g10()[1]
    boards = list(boards)
    rows = np.concatenate([afterstates(i) for i in boards])
    mover = np.concatenate([np.full(len(afterstates(i)), tu[i], np.int32) for i in boards])
    # rows with the same hidden pre-activations are evaluated ONCE: a BLAS product may sum two equal rows of one batch in different orders
    w = np.asarray(w, np.float32)
    pre = N.encode(rows, mover) @ w[:N.O1].reshape(N.N_HID, N.N_IN).T + w[N.O1:N.O2]
    uniq, inv = np.unique(pre, axis=0, return_inverse=True)
    one = np.float32(1)
    v = (one / (one + np.exp(-((one / (one + np.exp(-uniq))) @ w[N.O2:N.O3] + w[N.O3]))))[np.asarray(inv).ravel()].astype(np.float32)
    term = rows[np.arange(len(rows)), 26 + mover] == 15
    v[term] = np.where(mover[term] == 0, 1.0, 0.0).astype(np.float32)
    return np.split(v, np.cumsum([len(afterstates(i)) for i in boards])[:-1])
