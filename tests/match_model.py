"""Match play on the cubeful rollouts (include/bgamd.h, bgamd_env_rollout_match) as an exact model in plain Python, on top of
tests/cube_model.py: the threshold table, the decision before a turn, a trial's match-winning chance, the statistics.  No device, no
torch; every number is a Python float (fp64) or int and every operation is one rounded fp64 operation, so what the model returns is
what the kernels and the host's table must return bit for bit.

  a table    Table(M, met, met_pc): met[a-1][b-1], met_pc[k-1] as lists of floats
  a score    Score(away1, away2, state): PLAYER1's and PLAYER2's points to go; 0 normal, 1 the Crawford game, 2 post-Crawford
  a trial    cube_model's turns [(mover, mean, over)], points, value

Shared by tests/test_match_model_cpu.py and tests/test_gpu_rollout_match.py, which feeds it the device's own means and thresholds."""
import collections
import math

import numpy as np

import cube_model as CM

Table = collections.namedtuple("Table", "M met met_pc")
Score = collections.namedtuple("Score", "away1 away2 state")
# rec: cube_model's Record; dead: some decision was withheld by a dead cube; events: [(turn, mover, "take" | "pass")];
# degenerate: some decision met an entry of the table without thresholds
Played = collections.namedtuple("Played", "rec dead events degenerate")

INF = float("inf")


def table(met, met_pc):
    met = [[float(x) for x in row] for row in np.asarray(met, dtype=np.float64)]
    return Table(len(met), met, [float(x) for x in np.asarray(met_pc, dtype=np.float64)])


def levels(M):
    l = 0
    while (1 << l) < M:
        l += 1
    return l


def after(tab, a1, a2, state):
    """the MWC of the side needing a1 when the next game starts against a side needing a2"""
    if a1 <= 0:
        return 1.0
    if a2 <= 0:
        return 0.0
    if state != 0 and a2 == 1:
        return tab.met_pc[a1 - 1]
    if state != 0 and a1 == 1:
        return 1.0 - tab.met_pc[a2 - 1]
    return tab.met[a1 - 1][a2 - 1]


def thresholds(tab, window_share, state, c, a, b):
    """(double_at, pass_at) of a roller needing a against a side needing b with the cube on c; (inf, inf): no decision"""
    W1, L1 = after(tab, a - c, b, state), after(tab, a, b - c, state)
    W2, L2 = after(tab, a - 2 * c, b, state), after(tab, a, b - 2 * c, state)
    d1 = W2 - L2
    n2 = L1 - L2
    d2 = n2 + (W2 - W1)
    if not d1 > 0.0 or not d2 > 0.0:
        return INF, INF
    pass_at = (W1 - L2) / d1
    opens = n2 / d2
    double_at = opens + window_share * (pass_at - opens)
    if not (math.isfinite(pass_at) and math.isfinite(opens) and math.isfinite(double_at)):
        return INF, INF
    return double_at, pass_at


def threshold_table(tab, window_share):
    """{(state, cube, a, b): (double_at, pass_at)} for state 0 and 2, every cube 2^l < M and every a, b in 1 .. M"""
    return {(s, 1 << l, a, b): thresholds(tab, window_share, s, 1 << l, a, b)
            for s in (0, 2) for l in range(levels(tab.M)) for a in range(1, tab.M + 1) for b in range(1, tab.M + 1)}


def valid(score, M):
    a1, a2, st = score
    return 1 <= a1 <= M and 1 <= a2 <= M and st in (0, 1, 2) and ((min(a1, a2) == 1) == (st != 0))


def offer(played, k, mover, mean, over, rule, score, thr):
    """the trial after the decision before turn k; thr(state, cube, a, b) -> (double_at, pass_at).  rule: cube_model's Rule, of which
    too_good_at, max_cube and hold_turn0 count"""
    rec = played.rec
    if not CM.has_decision(rec, k, mover, over, rule) or score.state == 1:
        return played
    a, b = (score.away1, score.away2) if mover == 0 else (score.away2, score.away1)
    if rec.cube >= a:
        return played._replace(dead=True)
    double_at, pass_at = thr(score.state, rec.cube, a, b)
    if double_at == INF:
        played = played._replace(degenerate=True)
    w = float(mean) if mover == 0 else 1.0 - float(mean)
    if not (double_at <= w <= rule.too_good_at):
        return played
    opponent = 2 - mover
    if w > pass_at:
        return played._replace(rec=rec._replace(dropped=k, passed=opponent), events=played.events + [(k, mover, "pass")])
    return played._replace(rec=rec._replace(cube=2 * rec.cube, owner=opponent, doubles=rec.doubles + 1),
                           events=played.events + [(k, mover, "take")])


def play(turns, rule, score, thr, value=1, owner=0):
    played = Played(CM.start(value, owner), False, [], False)
    for k, (mover, mean, over) in enumerate(turns):
        played = offer(played, k, int(mover), mean, bool(over), rule, score, thr)
    return played


def payoff(tab, rec, points, value, score):
    """-> (PLAYER1's MWC, ended: +1 the trial ended the match for PLAYER1, -1 for PLAYER2, 0 neither or truncated)"""
    c = int(rec.cube)
    a1, a2, st = score
    if rec.dropped >= 0:
        r = c if rec.passed == 2 else -c
    elif points == 0:
        x = float(np.float32(value))
        return x * after(tab, a1 - c, a2, st) + (1.0 - x) * after(tab, a1, a2 - c, st), 0
    else:
        r = c * int(points)
    b1, b2 = a1 - max(r, 0), a2 - max(-r, 0)
    return after(tab, b1, b2, st), (1 if b1 <= 0 else (-1 if b2 <= 0 else 0))


def trial(tab, turns, points, value, rule, score, thr, start_value=1, start_owner=0):
    """-> (Played, mwc, ended)"""
    played = play(turns, rule, score, thr, start_value, start_owner)
    mwc, ended = payoff(tab, played.rec, int(points), value, score)
    return played, mwc, ended


statistics = CM.statistics                             # the fixed order of bgamd_env_rollout_cube_read, on the trials' MWC
paired = CM.paired                                     # the paired read's which = 4


def counts(results):
    """results: [(Played, mwc, ended)] of a position -> [ended for PLAYER1, ended for PLAYER2, a decision withheld by a dead cube]"""
    return [sum(e > 0 for _, _, e in results), sum(e < 0 for _, _, e in results), sum(bool(p.dead) for p, _, _ in results)]


def classes(played, turns, points, score, start_value=1):
    """the classes of the census a trial belongs to (a set of names)"""
    rec = played.rec
    out = set()
    if score.state == 1 and any(not t[2] for t in turns):
        out.add("Crawford game")
    if played.dead:
        out.add("dead cube")
    if rec.doubles >= 1:
        out.add("double / take")
    if rec.doubles >= 2:
        out.add("redouble")
    if rec.passed:
        out.add("pass by PLAYER%d" % rec.passed)
    if score.state == 2 and score.away1 != score.away2:
        trailer = 0 if score.away1 > score.away2 else 1
        first = [k for k, t in enumerate(turns) if t[0] == trailer and not t[2]]
        if first and any(k == first[0] and m == trailer for k, m, _ in played.events):
            out.add("post-Crawford trailer doubling at its first turn")
    if rec.dropped < 0 and points != 0:
        need = score.away1 if points > 0 else score.away2
        if abs(points) >= 2 and rec.cube >= 2 and need - rec.cube > 0 >= need - rec.cube * abs(points):
            out.add("match ended by a gammon times the cube")
        if rec.cube * abs(points) > need:
            out.add("points beyond the match length")
    if rec.dropped < 0 and points == 0:
        out.add("truncated payoff")
    if played.degenerate:
        out.add("degenerate entry")
    return out
