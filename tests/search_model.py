"""An exact model of stages B and D of the 2-ply search (csrc/bg_search.h): which candidates srch_select_kernel keeps and in which
order, how srch_reduce_kernel forms V2 from the 21 reply values, and which kept candidate it plays.  numpy float32 and integers only:
no net is evaluated here -- the values come from the caller (the device's own, or a reference's cast to float32), so what is modelled is
the RULE, bit for bit.

A lane's candidates are its distinct afterstates in reference order (search_ref.distinct_afterstates): the index in that list orders
them as the device's key does (smaller key = earlier reference-order index).  Values are float32 in [0, 1]; they are compared through
their bit patterns, as srch_pack does (for values >= +0.0 the two orders are the same)."""
import numpy as np

N_ROLLS = 21
DOUBLES = np.array([a == b for a in range(1, 7) for b in range(a, 7)])          # (1,1), (1,2), ..., (6,6)


def bits(v):
    """float32 values (or their uint32 bit patterns) -> int64 bit patterns"""
    v = np.ascontiguousarray(v)
    if v.dtype != np.uint32:
        assert v.dtype == np.float32, v.dtype
        v = v.view(np.uint32)
    return v.astype(np.int64)


def _best_first(index, value_bits, mover):
    """positions of the candidates, best for the mover first (PLAYER1: larger value, PLAYER2: smaller), then the smaller index"""
    b = bits(value_bits)
    return np.lexsort((np.asarray(index, np.int64), -b if int(mover) == 0 else b))


def select(order_index, v1_bits, mover, top_k):
    """Stage B.  order_index [m]: the reference-order index of each distinct afterstate of one lane (any order, no index twice);
    v1_bits [m]: its float32 1-ply value (a terminal candidate's is its outcome, exactly 1.0 or 0.0); mover 0 | 1; top_k (0 = keep all)
    -> the kept indices, best first: ranked by (v1 for the mover, smaller index), the first top_k of them."""
    idx = np.asarray(order_index, np.int64)
    assert len(np.unique(idx)) == len(idx)
    kept = idx[_best_first(idx, v1_bits, mover)]
    return kept[:top_k] if top_k else kept


def v2_from_replies(f21):
    """Stage D's V2 of a non-terminal candidate from its 21 reply values R(c, r) in roll order, float32 [..., 21] -> float32 [...]:
    sd = the running float32 sum over the six doubles in roll order, so = the running sum over the other fifteen in roll order,
    V2 = float32(float32(sd + 2 so) * float32(1 / 36)).  2 so is exact, so contracting sd + 2 so to an fma changes no bit."""
    f = np.asarray(f21, np.float32)
    assert f.shape[-1] == N_ROLLS
    sd = np.zeros(f.shape[:-1], np.float32)
    so = np.zeros(f.shape[:-1], np.float32)
    for r in range(N_ROLLS):
        if DOUBLES[r]:
            sd = (sd + f[..., r]).astype(np.float32)
        else:
            so = (so + f[..., r]).astype(np.float32)
    s = (sd + (np.float32(2) * so).astype(np.float32)).astype(np.float32)
    return (s * (np.float32(1) / np.float32(36))).astype(np.float32)


def choose(kept, v2_bits, mover):
    """Stage D's choice.  kept [k]: the kept candidates' reference-order indices (any order); v2_bits [k]: their float32 2-ply values
    -> the POSITION in kept of the candidate played: the best V2 for the mover, the smaller index on a tie (-1: nothing kept)."""
    if len(kept) == 0:
        return -1
    return int(_best_first(kept, v2_bits, mover)[0])
