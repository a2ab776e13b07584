#!/usr/bin/env python3
"""How good are a net's moves?  A player's greedy moves over --turns turns of --games games, each judged against a 2-ply search by
the judge's net over the player's top --top-k moves and the one it played (analysis.error_rate, bgamd_env_analyze_moves): the error of
a move is what the judge's best move is worth at 2 plies minus what the played one is, in win probability.  Every unforced turn
counts -- not one bit per game, as in an arena.  One run is one run: the figures move with the seed.

    python examples/error_rate.py --player CKPT --judge CKPT --games 4096 --turns 64 --top-k 4 [--epsilon 0.1 | --temperature 0.05]

CKPT: a file of 25 601 float32 (W1 | b1 | W2 | b2); left out: the bundled checkpoint.
"""
import argparse
import os
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")      # before the HIP runtime starts: backgammon_env/__init__.py says why
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "backgammon-engine_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import backgammon_env as bg  # noqa: E402
from backgammon_env import analysis  # noqa: E402

BUNDLED = os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32")


def table(path):
    w = np.fromfile(path or BUNDLED, dtype=np.float32)
    if w.size != 25601:
        sys.exit("%s: expected 25 601 float32" % (path or BUNDLED))
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--player", default=None, help="weights of the net that plays (default: the bundled checkpoint)")
    ap.add_argument("--judge", default=None, help="weights of the net that judges at 2 plies (default: the bundled checkpoint)")
    ap.add_argument("--games", type=int, default=4096, help="lanes: games played side by side (a finished game restarts)")
    ap.add_argument("--turns", type=int, default=64, help="turns played and judged per lane")
    ap.add_argument("--top-k", type=int, default=4, help="the judge searches the player's K best moves by 1-ply value and the played one (0 = all)")
    ap.add_argument("--epsilon", type=float, default=0.0, help="the player explores: a random move with this probability")
    ap.add_argument("--temperature", type=float, default=None,
                    help="the player draws every move with probability ~ exp(value / T) over its afterstates (not beside --epsilon)")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    player, judge = bg.VecGame(a.games, seed=a.seed), bg.VecGame(a.games, seed=a.seed)
    player.load_weights(table(a.player))
    judge.load_weights(table(a.judge))
    r = analysis.error_rate(player, judge, a.turns, top_k=a.top_k, epsilon=a.epsilon, temperature=a.temperature)
    print("player %s  judge %s (2-ply, top_k %d)  games %d  turns %d  epsilon %g  seed %d" %
          (os.path.basename(a.player or "bundled"), os.path.basename(a.judge or "bundled"), a.top_k, a.games, a.turns, a.epsilon, a.seed) +
          ("" if a.temperature is None else "  temperature %g" % a.temperature))
    cols = ("decisions", "unforced", "mistakes", "error_sum", "error_rate", "agreement", "passes", "illegal")
    print("%-8s" % "" + "".join("%14s" % c for c in cols))
    for side in ("player1", "player2", "total"):
        print("%-8s" % side + "".join(("%14.6f" if isinstance(r[side][c], float) else "%14d") % r[side][c] for c in cols))
    print("error_rate = error_sum / unforced (win probability lost per unforced move); agreement = 1 - mistakes / unforced")
    player.close()
    judge.close()
    if r["total"]["illegal"]:
        sys.exit("the judge does not list %d played boards" % r["total"]["illegal"])


if __name__ == "__main__":
    main()
