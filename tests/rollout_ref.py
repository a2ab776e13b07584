"""CPU Monte Carlo rollout reference in fp64 (the semantics pinned in include/bgamd.h, bgamd_env_rollout), built from the oracle's move
generator, TURN-stream dice (turn_randoms), encoder and fp64 forward pass, with the greedy step's first-index tie rule."""
import numpy as np

import search_ref as S
from oracle import oracle as O

TIE_EPS = 2e-5


def over_code(s28):
    """0 = not over, 1 = PLAYER1 has borne off 15, 2 = PLAYER2 has (PLAYER1 checked first, as the env does)."""
    if s28[26] == 15:
        return 1
    if s28[27] == 15:
        return 2
    return 0


def trial(weights, s28, turn, seed, j, i, max_plies=0, rotate=False):
    """One trial: game id j, trial index i (rotation: first dice = ordered pair i % 36).
    -> (value, turns, truncated, near_tie): near_tie when some decision had its best two distinct values within TIE_EPS."""
    s = np.asarray(s28, dtype=np.int32).copy()
    mover = int(turn)
    oc = over_code(s)
    if oc:
        return (1.0 if oc == 1 else 0.0), 0, False, False
    near = False
    k = 0
    while True:
        if max_plies and k == max_plies:
            return float(S.net(weights, s, mover)[0]), k, True, near
        if rotate and k == 0:
            d1, d2 = 1 + (i % 36) // 6, 1 + (i % 36) % 6
        else:
            d1, d2, _, _ = O.turn_randoms(seed, j, k)
        cand = S.distinct_afterstates(s, mover, d1, d2)
        if len(cand):
            v = S.net(weights, cand, mover)
            b = int(np.argmax(v) if mover == 0 else np.argmin(v))          # first index on ties
            u = np.unique(v)
            if len(u) > 1:
                second = u[-2] if mover == 0 else u[1]
                near |= abs(float(v[b]) - float(second)) < TIE_EPS
            s = cand[b].copy()
        k += 1
        oc = over_code(s)
        if oc:
            return (1.0 if oc == 1 else 0.0), k, False, near
        mover ^= 1
        if k > 100000:
            raise RuntimeError("trial did not end")


def rollout(weights, states28, turns, trials, seed, max_plies=0, rotate=False, position_offset=0):
    """-> dict of arrays: value [P,T], turns [P,T], truncated [P,T], near_tie [P,T]"""
    P = len(states28)
    out = {k: np.zeros((P, trials), dt) for k, dt in (("value", np.float64), ("turns", np.int64), ("truncated", bool),
                                                      ("near_tie", bool))}
    for p in range(P):
        for i in range(trials):
            j = (position_offset + p) * trials + i
            r = trial(weights, states28[p], turns[p], seed, j, i, max_plies, rotate)
            for k, x in zip(("value", "turns", "truncated", "near_tie"), r):
                out[k][p, i] = x
    return out
