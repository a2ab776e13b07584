"""The cases of the cube tests and their fp64 reference.  No device, no torch.  Shared by tests/test_cube_model_cpu.py, which computes
under the reference the conditions the GPU tests rest on (every class of cube history occurs, with room to spare), and
tests/test_gpu_rollout_cube.py, which asserts the same census on the device.

The positions follow tests/test_gpu_rollout_2ply.py's shapes -- a contact position, a bear-off that ends inside the turn limit, a
position that is already over -- but are fixed boards, so that the reference can play them without a device."""
import functools
import itertools
import os

import numpy as np

import cube_model as CM
import outcome_ref as OR
import rollout_ref as R
import rollout_vr_ref as V
import search_ref as S
from oracle import oracle as O

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SEED = 20240603
LANES = 256
OFFSET = 3                                         # position_offset of the replayed calls
SHAPES = [(True, 36), (False, 40)]                 # (rotate, T)
HORIZON = 4                                        # the turn limit of the truncated calls (M = 0: the bear-off alone, played out)

# The thresholds of the tests.  The header's suggested defaults (0.70 / 0.78 / 1.0, max_cube 64) do not give every class on three
# small positions within four turns -- the start position's roller stands at 0.59, and a redouble needs the lead to change hands
# between two takes -- so the tests use these:
#   RULE         a side doubles as soon as it is a little ahead (0.52), the other takes up to 0.80, nobody is ever too good, and the
#                cube stops at 4, so that a redouble reaches max_cube: takes and redoubles in the contact position (its roller stands
#                at 0.5945, the replies between 0.43 and 0.60), PLAYER1 passing at turn 0 of the bear-off (its roller at 0.98);
#   RULE_TIGHT   the same with passes above 0.58: PLAYER2 passes at turn 0 of the contact position; with the cube in PLAYER2's hands
#                instead ("no access") PLAYER1's roller must hold, and PLAYER2's doubles at turn 1 are taken or passed;
#   RULE_JACOBY  RULE with a side above 0.97 too good to double, and the Jacoby rule: the bear-off's roller plays on, and the gammons
#                it wins with a doubles roll count as single games.
# tests/test_cube_model_cpu.py asserts the census under the fp64 reference, counting a trial for a class only if it stays in it
# however its means move by MEAN_TOL, each on its own (the bear-off's 0.9712 against 0.97 is the nearest a class comes to a threshold).
RULE = CM.Rule(double_at=0.52, pass_at=0.80, too_good_at=1.0, max_cube=4)
RULE_TIGHT = CM.Rule(double_at=0.52, pass_at=0.58, too_good_at=1.0, max_cube=4)
RULE_JACOBY = CM.Rule(double_at=0.52, pass_at=0.80, too_good_at=0.97, max_cube=4, jacoby=True)
MEAN_TOL = 1e-5                                    # the project's value tolerance: the classes must survive every mean moving by it

# (name, rule, start table): the calls of the GPU tests whose census is taken
CONFIGS = [("take", RULE, "centre"), ("tight", RULE_TIGHT, "centre"), ("no access", RULE_TIGHT, "no access"), ("owned", RULE, "owned"),
           ("jacoby", RULE_JACOBY, "centre")]
CLASSES = ("never doubled", "double / take", "pass by PLAYER1", "pass by PLAYER2", "redouble", "reached max_cube",
           "gammon reduced by Jacoby", "drop at turn 0", "no access")


def weights():
    return np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)


def positions():
    """-> (states [3, 28], turn [3]): contact (the start position, PLAYER1 to roll), a bear-off with PLAYER2 to roll that ends within
    four turns and in which PLAYER1 may still be gammoned, a position that is over (PLAYER2 has won a gammon)"""
    bear = OR._state(p1=[(19, 3), (20, 3), (21, 3), (22, 3), (23, 2), (24, 1)], p2=[(1, 1), (2, 1), (3, 1)], off2=12)
    over = np.zeros(28, np.int32)
    over[27] = 15; over[19:24] = 3
    return np.stack([OR.START, bear, over]).astype(np.int32), np.array([0, 1, 0], np.int32)


# start tables of the calls: (value, owner) per position
TABLES = {
    "centre": ([1, 1, 1], [0, 0, 0]),
    "owned": ([2, 2, 2], [1, 2, 0]),                 # a cube of 2 owned by PLAYER1, by PLAYER2, centred
    "no access": ([1, 1, 1], [2, 1, 1]),             # the roller of the contact position and of the bear-off does not own the cube
    "at max": ([4, 4, 4], [0, 1, 2]),                # max_cube equal to the start value: no decision is ever made
}


def ref_trial(weights, s28, turn, seed, j, i, max_plies=0, rotate=False):
    """rollout_vr_ref.trial's loop, keeping what the cube needs: -> (turns [(mover, mean, over)], points, value, truncated).  A position
    that is over has one entry (mover, outcome, True) and no turn."""
    s = np.asarray(s28, dtype=np.int32).copy()
    mover = int(turn)
    oc = R.over_code(s)
    if oc:
        return [(mover, 1.0 if oc == 1 else 0.0, True)], OR.points(s), (1.0 if oc == 1 else 0.0), False
    seq = []
    k = 0
    while True:
        if max_plies and k == max_plies:
            return seq, 0, float(np.float32(S.net(weights, s, mover)[0])), True
        if rotate and k == 0:
            d1, d2 = 1 + (i % 36) // 6, 1 + (i % 36) % 6
        else:
            d1, d2, _, _ = O.turn_randoms(seed, j, k)
        _, mean = V.preroll(weights, s, mover)
        seq.append((mover, float(mean), False))
        cand = S.distinct_afterstates(s, mover, d1, d2)
        if len(cand):
            v = S.net(weights, cand, mover)
            s = cand[int(np.argmax(v) if mover == 0 else np.argmin(v))].copy()
        k += 1
        oc = R.over_code(s)
        if oc:
            return seq, OR.points(s), (1.0 if oc == 1 else 0.0), False
        mover ^= 1


@functools.lru_cache(maxsize=None)
def reference(rotate, T, max_plies):
    """the trials of the call (positions(), T, rotate, max_plies, position_offset OFFSET) under the fp64 reference: [P][T] of ref_trial's
    tuples (computed once per process)"""
    st, tu = positions()
    w = weights()
    return [[ref_trial(w, st[p], tu[p], SEED, (OFFSET + p) * T + i, i, max_plies, rotate) for i in range(T)] for p in range(len(st))]


def full_census(trials_of, tol=0.0):
    """the union over CONFIGS and SHAPES: trials_of(rotate, T) -> [P][T] of ref_trial's tuples.  -> {class: count}; drops at turn 0 are
    counted in the rotated shape only (the class is a drop at a ROTATED turn 0)"""
    out = {}
    for _, rule, table in CONFIGS:
        values, owners = TABLES[table]
        for rotate, T in SHAPES:
            for c, n in census(trials_of(rotate, T), rule, values, owners, tol).items():
                if c != "drop at turn 0" or rotate:
                    out[c] = out.get(c, 0) + n
    return out


def census(trials, rule, values, owners, tol=0.0):
    """trials [P][T] of (turns, points, value, truncated) -> {class name: count} under the rule and the start tables.  tol > 0: a trial
    counts for a class only if it belongs to it however its means move, each on its own, by -tol, 0 or +tol (every decision is monotone
    in its mean, so the three values cover the interval)"""
    out = {}
    for p, row in enumerate(trials):
        for turns, points, value, _ in row:
            live = [k for k, t in enumerate(turns) if not t[2]]
            sure = None
            for moves in itertools.product((0.0,) if tol == 0.0 else (-tol, 0.0, tol), repeat=len(live)):
                moved = list(turns)
                for k, d in zip(live, moves):
                    moved[k] = (turns[k][0], turns[k][1] + d, False)
                rec = CM.play(moved, rule, values[p], owners[p])
                cl = CM.classes(rec, moved, points, rule, values[p], owners[p])
                sure = cl if sure is None else sure & cl
            for c in sure:
                out[c] = out.get(c, 0) + 1
    return out
