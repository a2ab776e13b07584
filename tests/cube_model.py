"""The doubling cube of the rollouts (include/bgamd.h, bgamd_env_rollout_cube) as an exact model in plain Python: a trial's record is a
value that `offer` maps to the next one, turn by turn; `equity` pays it out.  No device, no torch; every number is a Python float
(fp64) or int, so what the model returns is what the kernels must return bit for bit when they are fed the same means.

  a trial    turns = [(mover, mean, over), ...]: before turn k the side `mover` (0 PLAYER1, 1 PLAYER2) is to roll, mean = mean(s_k) of
             the pre-roll evaluation, over = the position is over (no decision; the rollouts never play such a turn, the flag is there
             for a position that is over at turn 0)
  its end    points (+-1, +-2, +-3 from PLAYER1's side, 0 = truncated), value (the fp32 net value of a truncated trial)

Shared by tests/test_cube_model_cpu.py, which checks the model against a second statement of the rule and against wrong ones, and
tests/test_gpu_rollout_cube.py, which feeds it the device's own means."""
import collections
import math

import numpy as np

Rule = collections.namedtuple("Rule", "double_at pass_at too_good_at max_cube jacoby hold_turn0",
                              defaults=(0.70, 0.78, 1.0, 64, False, False))
# cube: the value; owner: 0 centre, 1 PLAYER1, 2 PLAYER2; dropped: the turn of the drop or -1; passed: the side that passed (0 none);
# doubles: the times the cube was turned in the trial
Record = collections.namedtuple("Record", "cube owner dropped passed doubles")

WAVE = 64


def start(value=1, owner=0):
    return Record(int(value), int(owner), -1, 0, 0)


def has_decision(rec, k, mover, over, rule):
    return (rec.dropped < 0 and not over and rec.cube < rule.max_cube and rec.owner in (0, mover + 1)
            and not (rule.hold_turn0 and k == 0))


def offer(rec, k, mover, mean, over, rule):
    """the record after the decision before turn k (unchanged when none is made)"""
    if not has_decision(rec, k, mover, over, rule):
        return rec
    w = float(mean) if mover == 0 else 1.0 - float(mean)
    if not (rule.double_at <= w <= rule.too_good_at):
        return rec
    opponent = 2 - mover
    if w > rule.pass_at:
        return rec._replace(dropped=k, passed=opponent)
    return rec._replace(cube=2 * rec.cube, owner=opponent, doubles=rec.doubles + 1)


def play(turns, rule, value=1, owner=0):
    rec = start(value, owner)
    for k, (mover, mean, over) in enumerate(turns):
        rec = offer(rec, k, int(mover), mean, bool(over), rule)
    return rec


def equity(rec, points, value, rule):
    """the trial's cubeful equity from PLAYER1's side (fp64)"""
    c = float(rec.cube)
    if rec.dropped >= 0:
        return c if rec.passed == 2 else -c
    if points == 0:
        return c * (2.0 * float(np.float32(value)) - 1.0)
    if rule.jacoby and rec.doubles == 0:
        points = 1 if points > 0 else -1
    return c * float(points)


def trial(turns, points, value, rule, start_value=1, start_owner=0):
    """-> (record, cubeful equity)"""
    rec = play(turns, rule, start_value, start_owner)
    return rec, equity(rec, int(points), value, rule)


# ---- the statistics of bgamd_env_rollout_cube_read -------------------------------------------------------------------------------------

def wave_sum(vals):
    """vals[i], i < T, summed as a wave does: lane k adds vals[k], vals[k + 64], ... to 0.0 in order, then the xor butterfly"""
    s = [0.0] * WAVE
    for k in range(WAVE):
        for i in range(k, len(vals), WAVE):
            s[k] = s[k] + float(vals[i])
    m = WAVE // 2
    while m >= 1:
        s = [s[k] + s[k ^ m] for k in range(WAVE)]
        m //= 2
    return s[0]


def statistics(eq):
    """eq [T] -> (mean, stderr) in the fixed order, every operation a rounded fp64 one (no fused multiply-add on the device either)"""
    T = len(eq)
    m = wave_sum(eq) / float(T)
    q = wave_sum([(float(e) - m) * (float(e) - m) for e in eq])
    return m, (math.sqrt(q / (float(T) * float(T - 1))) if T > 1 else 0.0)


def paired(eq_p, eq_r):
    """the paired read's which = 3 of a position against a reference of its dice group -> (diff_mean, diff_stderr)"""
    T = len(eq_p)
    d = [float(a) - float(b) for a, b in zip(eq_p, eq_r)]
    m = wave_sum(d) / float(T)
    q = wave_sum([(x - m) * (x - m) for x in d])
    return m, (math.sqrt(q / (float(T) * float(T - 1))) if T > 1 else 0.0)


def counts(records, rule):
    """[trials PLAYER1 passed, trials PLAYER2 passed, cube turns, trials whose final cube is >= max_cube]"""
    return [sum(r.passed == 1 for r in records), sum(r.passed == 2 for r in records), sum(r.doubles for r in records),
            sum(r.cube >= rule.max_cube for r in records)]


def classes(rec, turns, points, rule, start_value=1, start_owner=0):
    """the classes of the census a trial belongs to (a set of names)"""
    out = set()
    if rec.doubles == 0 and rec.dropped < 0:
        out.add("never doubled")
    if rec.doubles >= 1:
        out.add("double / take")
    if rec.doubles >= 2:
        out.add("redouble")
    if rec.passed:
        out.add("pass by PLAYER%d" % rec.passed)
    if rec.cube >= rule.max_cube > start_value:
        out.add("reached max_cube")
    if rule.jacoby and rec.dropped < 0 and rec.doubles == 0 and abs(points) >= 2:
        out.add("gammon reduced by Jacoby")
    if rec.dropped == 0:
        out.add("drop at turn 0")
    if turns and not turns[0][2] and start_owner not in (0, turns[0][0] + 1):
        w = turns[0][1] if turns[0][0] == 0 else 1.0 - turns[0][1]
        if rule.double_at <= w <= rule.too_good_at and start_value < rule.max_cube:
            out.add("no access")                          # the roller would have doubled had it had the cube
    return out
