"""CPU reference in fp64 of the 1-ply pre-roll evaluation and of the luck-adjusted rollout (the semantics pinned in include/bgamd.h,
bgamd_env_evaluate_preroll and BGAMD_ROLLOUT_VR), built on search_ref.reply_values and the trial rules of rollout_ref."""
import numpy as np

import rollout_ref as R
import search_ref as S
from oracle import oracle as O

ROLL_INDEX = {r: k for k, r in enumerate(S.ROLLS)}


def roll_index(d1, d2):
    """Index of the unordered roll of dice (d1, d2) in S.ROLLS."""
    return ROLL_INDEX[(min(d1, d2), max(d1, d2))]


def preroll(weights, s28, turn):
    """-> (f [21] float64, mean): f[r] = the value of the greedy choice of `turn` for roll S.ROLLS[r] (the net's value of the position
    when the roll has no move); a position that is over gives its outcome for every roll.  mean = sum of w_r f[r] in roll order."""
    s = np.asarray(s28, dtype=np.int32)
    oc = R.over_code(s)
    if oc:
        f = [1.0 if oc == 1 else 0.0] * len(S.ROLLS)
    else:
        f, _ = S.reply_values(weights, s, int(turn))
    f = np.asarray(f, dtype=np.float64)
    mean = 0.0
    for w, x in zip(S.ROLL_W, f):
        mean = mean + w * x
    return f, mean


def trial(weights, s28, turn, seed, j, i, max_plies=0, rotate=False):
    """rollout_ref.trial plus the trial's luck total L = sum over its turns of f(s_k, r_k) - mean(s_k), in turn order.
    -> (value, turns, truncated, near_tie, luck)"""
    s = np.asarray(s28, dtype=np.int32).copy()
    mover = int(turn)
    oc = R.over_code(s)
    if oc:
        return (1.0 if oc == 1 else 0.0), 0, False, False, 0.0
    near = False
    luck = 0.0
    k = 0
    while True:
        if max_plies and k == max_plies:
            return float(S.net(weights, s, mover)[0]), k, True, near, luck
        if rotate and k == 0:
            d1, d2 = 1 + (i % 36) // 6, 1 + (i % 36) % 6
        else:
            d1, d2, _, _ = O.turn_randoms(seed, j, k)
        f, mean = preroll(weights, s, mover)
        luck = luck + (f[roll_index(d1, d2)] - mean)
        cand = S.distinct_afterstates(s, mover, d1, d2)
        if len(cand):
            v = S.net(weights, cand, mover)
            b = int(np.argmax(v) if mover == 0 else np.argmin(v))          # first index on ties
            u = np.unique(v)
            if len(u) > 1:
                second = u[-2] if mover == 0 else u[1]
                near |= abs(float(v[b]) - float(second)) < R.TIE_EPS
            s = cand[b].copy()
        k += 1
        oc = R.over_code(s)
        if oc:
            return (1.0 if oc == 1 else 0.0), k, False, near, luck
        mover ^= 1
        if k > 100000:
            raise RuntimeError("trial did not end")


def rollout(weights, states28, turns, trials, seed, max_plies=0, rotate=False, position_offset=0):
    """-> dict of arrays: value, turns, truncated, near_tie, luck [P,T]"""
    P = len(states28)
    keys = ("value", "turns", "truncated", "near_tie", "luck")
    out = {k: np.zeros((P, trials), dt) for k, dt in zip(keys, (np.float64, np.int64, bool, bool, np.float64))}
    for p in range(P):
        for i in range(trials):
            j = (position_offset + p) * trials + i
            r = trial(weights, states28[p], turns[p], seed, j, i, max_plies, rotate)
            for k, x in zip(keys, r):
                out[k][p, i] = x
    return out
