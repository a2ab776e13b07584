"""CPU 2-ply expectimax reference in fp64 (the semantics pinned in include/bgamd.h, bgamd_env_step_search), built from the oracle's
move generator, encoder and fp64 forward pass."""
import numpy as np

from oracle import oracle as O

ROLLS = [(a, b) for a in range(1, 7) for b in range(a, 7)]          # (1,1), (1,2), ..., (6,6)
ROLL_W = [1.0 / 36.0 if a == b else 2.0 / 36.0 for a, b in ROLLS]


def distinct_afterstates(s28, player, d1, d2):
    """Distinct afterstates of a turn in reference order (the first copy stands for all: the greedy step's tie rule)."""
    _, _, st = O.evaluate_turn_sequences(O.State.from28(s28, player), player, d1, d2)
    if len(st) == 0:
        return st
    _, first = np.unique(st, axis=0, return_index=True)
    return st[np.sort(first)]


def net(weights, states, turn):
    states = np.asarray(states, dtype=np.int32).reshape(-1, 28)
    if len(states) == 0:
        return np.zeros(0)
    return O.forward_f64(weights, O.encode(states, turn))


def outcome(s28, mover):
    """1.0 / 0.0 when the mover has borne off the 15th checker, else None."""
    if mover == 0 and s28[26] == 15:
        return 1.0
    if mover == 1 and s28[27] == 15:
        return 0.0
    return None


def reply_values(weights, c28, opp):
    """R(c, r) for the 21 rolls: the greedy reply's value, or the net's value of c with the opponent's turn bit (no move).
    -> (list of 21 values, number of rolls with no move)"""
    lists = [distinct_afterstates(c28, opp, a, b) for a, b in ROLLS]
    rows = [l for l in lists if len(l)]
    allrows = np.concatenate(rows) if rows else np.zeros((0, 28), np.int32)
    uniq, inv = (np.unique(allrows, axis=0, return_inverse=True) if len(allrows) else (allrows, np.zeros(0, np.int64)))
    vals = net(weights, uniq, opp)[np.asarray(inv).ravel()] if len(uniq) else np.zeros(0)
    pass_v = None
    out, k = [], 0
    for l in lists:
        if len(l) == 0:
            if pass_v is None:
                pass_v = float(net(weights, c28, opp)[0])
            out.append(pass_v)
            continue
        v = vals[k:k + len(l)]
        k += len(l)
        out.append(float(v.min() if opp == 1 else v.max()))
    # (a doubles roll with no legal move is ONE empty sequence whose afterstate is c itself: the same value, counted as a pass)
    return out, sum(1 for l in lists if len(l) == 0 or (len(l) == 1 and (l[0] == c28).all()))


def search(weights, s28, mover, d1, d2, top_k):
    """-> dict(states [K,28], v1 [K], v2 [K], choice (index into states, -1 = no move), terminal [K], passes (rolls with no reply))."""
    s28 = np.asarray(s28, dtype=np.int32)
    cand = distinct_afterstates(s28, mover, d1, d2)
    if len(cand) == 0:
        return {"states": cand, "v1": np.zeros(0), "v2": np.zeros(0), "choice": -1, "terminal": np.zeros(0, bool), "passes": 0}
    v = net(weights, cand, mover)
    term = np.array([outcome(c, mover) is not None for c in cand])
    v1 = np.array([outcome(c, mover) if t else v[i] for i, (c, t) in enumerate(zip(cand, term))])
    order = sorted(range(len(cand)), key=lambda i: ((-v1[i]) if mover == 0 else v1[i], i))
    keep = order[:top_k] if top_k else order
    v2, passes = [], 0
    for i in keep:
        if term[i]:
            v2.append(v1[i])
            continue
        opp = 1 - mover
        R, n_pass = reply_values(weights, cand[i], opp)
        passes += n_pass
        v2.append(sum(w * r for w, r in zip(ROLL_W, R)))
    v2 = np.array(v2)
    best = sorted(range(len(keep)), key=lambda j: ((-v2[j]) if mover == 0 else v2[j], keep[j]))[0]
    return {"states": cand[keep], "v1": v1[keep], "v2": v2, "choice": best, "terminal": term[keep], "passes": passes,
            "keys": np.array(keep)}
