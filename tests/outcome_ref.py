"""CPU reference of a finished game in points (the rule pinned in include/bgamd.h above bgamd_outcomes), in numpy on the int32[28] state,
and rollout_ref.trial's loop returning the final board too.  Shared by tests/test_outcome_cpu.py and tests/test_gpu_outcome.py: the
forced positions whose one-turn results the GPU tests rest on are listed here."""
import numpy as np

import rollout_ref as R
import search_ref as S
from oracle import oracle as O

START = np.array([2, 0, 0, 0, 0, -5, 0, -3, 0, 0, 0, 5, -5, 0, 0, 0, 3, 0, 5, 0, 0, 0, 0, -2, 0, 0, 0, 0], np.int32)


def points(s28):
    """0 = not over; +1 / +2 / +3 = PLAYER1 won a single game / gammon / backgammon; -1 / -2 / -3 = PLAYER2 did (PLAYER1 checked first)."""
    s = np.asarray(s28)
    off1, off2, bar1, bar2 = int(s[26]), int(s[27]), int(s[24]), int(s[25])
    if off1 == 15:
        if off2 > 0:
            return 1
        return 3 if bar2 > 0 or bool((s[18:24] < 0).any()) else 2
    if off2 == 15:
        if off1 > 0:
            return -1
        return -3 if bar1 > 0 or bool((s[0:6] > 0).any()) else -2
    return 0


def points_many(states28):
    return np.array([points(s) for s in np.asarray(states28).reshape(-1, 28)], np.int32)


def _state(p1=(), p2=(), bar1=0, bar2=0, off1=0, off2=0):
    """p1 / p2: (point 1..24, count) pairs"""
    s = np.zeros(28, np.int32)
    for pt, c in p1:
        s[pt - 1] += c
    for pt, c in p2:
        s[pt - 1] -= c
    s[24:28] = (bar1, bar2, off1, off2)
    assert int(s[:24][s[:24] > 0].sum()) + bar1 + off1 == 15 and int(-s[:24][s[:24] < 0].sum()) + bar2 + off2 == 15, s
    return s


def probe_family():
    """For each winner: the loser's 15 checkers as 14 parked in its own home plus one probe checker on each of the 24 points and on its
    bar, with off = 0; and the same with off = 1 (13 parked).  -> (states [100, 28], expected points [100])"""
    st, want = [], []
    for winner in (0, 1):
        for off in (0, 1):
            for probe in list(range(1, 25)) + ["bar"]:
                park = 14 - off
                if winner == 0:                      # PLAYER2 lost: its home is points 1..6
                    p2 = [(1, 5), (2, 5), (3, park - 10)] + ([(probe, 1)] if probe != "bar" else [])
                    s = _state(p2=p2, bar2=1 if probe == "bar" else 0, off1=15, off2=off)
                    deep = probe == "bar" or probe >= 19
                    want.append(1 if off else (3 if deep else 2))
                else:                                # PLAYER1 lost: its home is points 19..24
                    p1 = [(24, 5), (23, 5), (22, park - 10)] + ([(probe, 1)] if probe != "bar" else [])
                    s = _state(p1=p1, bar1=1 if probe == "bar" else 0, off2=15, off1=off)
                    deep = probe == "bar" or probe <= 6
                    want.append(-1 if off else (-3 if deep else -2))
                st.append(s)
    return np.array(st, np.int32), np.array(want, np.int32)


def forced_positions():
    """The ten positions that end in one turn (position 8: only for the rolls holding a 1), with the side to move and the points every
    roll (8: every roll with a 1) gives.  -> (states [10, 28], turn [10], points [10], names)"""
    p1_last = [(24, 1)]
    p2_home = [(1, 5), (2, 5), (3, 4)]
    p2_last = [(1, 1)]
    p1_home = [(24, 5), (23, 5), (22, 4)]
    rows = [
        ("1a", _state(p1=p1_last, p2=[(1, 5), (2, 5), (3, 5)], off1=14), 0, 2),
        ("1b", _state(p1=p1_last, p2=p2_home + [(18, 1)], off1=14), 0, 2),
        ("2a", _state(p1=p1_last, p2=p2_home + [(19, 1)], off1=14), 0, 3),
        ("2b", _state(p1=p1_last, p2=p2_home + [(20, 1)], off1=14), 0, 3),
        ("3", _state(p1=p1_last, p2=p2_home, bar2=1, off1=14), 0, 3),
        ("4", _state(p1=p1_last, p2=p2_home, off1=14, off2=1), 0, 1),
        ("5", _state(p2=p2_last, p1=[(24, 5), (23, 5), (22, 5)], off2=14), 1, -2),
        ("6", _state(p2=p2_last, p1=p1_home, bar1=1, off2=14), 1, -3),
        ("7", _state(p2=p2_last, p1=p1_home, off2=14, off1=1), 1, -1),
        ("8", _state(p2=p2_last, p1=p1_home + [(6, 1)], off2=14), 1, -3),
    ]
    return (np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], np.int32),
            np.array([r[3] for r in rows], np.int32), [r[0] for r in rows])


def over_boards():
    """Two boards that are already over: 15 off on both sides (PLAYER1's single game), and a PLAYER2 gammon."""
    both = np.zeros(28, np.int32)
    both[26] = both[27] = 15
    return np.array([both, _state(p1=[(24, 5), (23, 5), (12, 5)], off2=15)], np.int32), np.array([1, -2], np.int32)


def trial_with_board(weights, s28, turn, seed, j, i, max_plies=0, rotate=False):
    """rollout_ref.trial's loop -> (value, turns, truncated, near_tie, final board int32[28])."""
    s = np.asarray(s28, dtype=np.int32).copy()
    mover = int(turn)
    oc = R.over_code(s)
    if oc:
        return (1.0 if oc == 1 else 0.0), 0, False, False, s
    near = False
    k = 0
    while True:
        if max_plies and k == max_plies:
            return float(S.net(weights, s, mover)[0]), k, True, near, s
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
                near |= abs(float(v[b]) - float(second)) < R.TIE_EPS
            s = cand[b].copy()
        k += 1
        oc = R.over_code(s)
        if oc:
            return (1.0 if oc == 1 else 0.0), k, False, near, s
        mover ^= 1
        if k > 100000:
            raise RuntimeError("trial did not end")


def trial_points(weights, s28, turn, seed, j, i, max_plies=0, rotate=False):
    """-> (points of the trial: 0 when truncated, near_tie)"""
    _, _, trunc, near, board = trial_with_board(weights, s28, turn, seed, j, i, max_plies, rotate)
    return (0 if trunc else points(board)), near
