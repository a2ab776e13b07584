#!/usr/bin/env python3
"""Double or not, take or pass: the cube action of a handful of positions by cubeful rollout (backgammon_env.analysis.cube_action).

    python examples/cube_action.py [--trials 1296] [--max-plies 0] [--plies 1] [--match-to N --score A,B [--crawford | --post-crawford]]

Every position is rolled out twice on the same dice -- as it stands with the roller holding the cube this turn ("no double"), and with
the cube doubled in the opponent's hands ("double / take") -- and the three cubeful equities nd, dt and dp = the cube are put through
GNU Backgammon's table.  The trials handle the cube by a plain money-play rule of thumb (double from 0.70 of the pre-roll evaluation,
pass above 0.78), no measured optimum; the net knows wins only, so the checker play is the cubeless one.

--match-to N --score A,B: the same in a match to N points that PLAYER1 leads or trails A to B.  The three numbers are then the
roller's match-winning chances, and the trials handle the cube by the thresholds of the score (backgammon_env.Match).  The match
equity table is MatchTable.janowski(N), an approximation; bring a published one with MatchTable.load.  When a side is one point
from the match, say whether this is the Crawford game (--crawford) or a later one (--post-crawford)."""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "backgammon-engine_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import backgammon_env as bg  # noqa: E402
from backgammon_env import _capi  # noqa: E402
from backgammon_env.analysis import cube_action  # noqa: E402


def board(p1=(), p2=(), bar1=0, bar2=0, off1=0, off2=0):
    """int32[28]: p1 / p2 as (point 1..24, count); PLAYER1 moves up and bears off from 19..24, PLAYER2 moves down and bears off from 1..6"""
    s = np.zeros(28, np.int32)
    for pt, c in p1:
        s[pt - 1] += c
    for pt, c in p2:
        s[pt - 1] -= c
    s[24:28] = (bar1, bar2, off1, off2)
    return s


POSITIONS = [
    ("start position, PLAYER1 to roll", board(p1=[(1, 2), (12, 5), (17, 3), (19, 5)], p2=[(24, 2), (13, 5), (8, 3), (6, 5)]), 0, 1, 0),
    ("PLAYER1 ahead in a race", board(p1=[(19, 4), (20, 4), (21, 3), (22, 2), (23, 2)], p2=[(6, 4), (5, 4), (4, 3), (7, 2), (8, 2)]), 0, 1, 0),
    ("the same race, PLAYER2 owns a 2-cube", board(p1=[(19, 4), (20, 4), (21, 3), (22, 2), (23, 2)], p2=[(6, 4), (5, 4), (4, 3), (7, 2), (8, 2)]), 0, 2, 2),
    ("two checkers against three, PLAYER2 to roll", board(p1=[(24, 1), (23, 1), (22, 1)], p2=[(1, 1), (2, 1)], off1=12, off2=13), 1, 1, 0),
    ("PLAYER2 to roll and win a gammon", board(p1=[(19, 5), (20, 5), (21, 5)], p2=[(1, 1), (2, 1), (3, 1)], off2=12), 1, 1, 0),
    ("already over", board(p1=[(19, 5), (20, 5), (21, 5)], off2=15), 0, 1, 0),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=1296)
    ap.add_argument("--max-plies", type=int, default=0)
    ap.add_argument("--plies", type=int, default=1, choices=(1, 2))
    ap.add_argument("--match-to", type=int, default=0)
    ap.add_argument("--score", default="0,0")
    ap.add_argument("--crawford", action="store_true")
    ap.add_argument("--post-crawford", action="store_true")
    a = ap.parse_args()
    match = None
    if a.match_to:
        won1, won2 = (int(x) for x in a.score.split(","))
        state = 1 if a.crawford else (2 if a.post_crawford else None)
        match = bg.Match(bg.MatchTable.janowski(a.match_to), a.match_to - won1, a.match_to - won2, state)
    env = bg.VecGame(64, seed=1)
    env.load_weights(np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32))
    res = cube_action(env, np.stack([p[1] for p in POSITIONS]), [p[2] for p in POSITIONS], cube_value=[p[3] for p in POSITIONS],
                      cube_owner=[p[4] for p in POSITIONS], trials=a.trials, max_plies=a.max_plies, plies=a.plies, match=match)
    print("%-46s %8s %17s %17s %6s %17s %7s  %s" % ("position", "cubeless", "no double", "double / take", "pass", "dt - nd (paired)", "win", "action"))
    for (name, *_), r in zip(POSITIONS, res):
        pm = lambda k: "%+.3f +- %.3f" % (r[k], r[k + "_stderr"])
        if "dt" in r and match is not None:
            print("%-46s %+8.3f %17s %17s %6.3f %17s %7.3f  %s" % (name, r["cubeless"], pm("nd"), pm("dt"), r["dp"],
                                                                    "%+.3f +- %.3f" % (r["diff"], r["diff_stderr"]), r["shares"]["win"], r["action"]))
        elif "dt" in r:
            print("%-46s %+8.3f %17s %17s %+6.0f %17s %7.3f  %s" % (name, r["cubeless"], pm("nd"), pm("dt"), r["dp"],
                                                                     "%+.3f +- %.3f" % (r["diff"], r["diff_stderr"]), r["shares"]["win"], r["action"]))
        else:
            print("%-46s %+8.3f %17s %17s %6s %17s %7.3f  %s" % (name, r["cubeless"], pm("nd"), "-", "-", "-", r["shares"]["win"], r["action"]))
    print("lane-turns played, and of those after the trial's drop:", env.rollout_cube_info())
    print("package", os.path.dirname(os.path.abspath(bg.__file__)), "library", os.path.abspath(_capi.LIB_PATH))
    env.close()


if __name__ == "__main__":
    main()
