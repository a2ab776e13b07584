"""Head-to-head evaluation: the reference's `_play_head_to_head` /
`evaluate_parallel` (pysrc/TD(λ) model/train.py:262-302) and `play_vs_random` / `play_vs_model`
(pysrc/benchmark.py:64-130) on the batched env: all games of a match-up advance together, PLAYER1's
lanes are stepped with one policy and PLAYER2's with the other."""
from __future__ import annotations

import torch

from . import F32, VecGame


def _play(env: VecGame, p1_policy, p2_policy, max_turns: int, precision, temperature=None):
    """policies: ("net", slot), ("search", slot, top_k), ("search3", slot, top_k, margin, deep_k, deep_margin, reply_top_k, reply_margin)
    or ("random",).  The constructor seats the first mover by game parity
    (`Game(i % 2)`, train.py:265), no opening roll.
    -> (games finished, PLAYER1 wins, points int64 [7]: lanes by VecGame.outcomes() + 3, i.e. PLAYER2 backgammon, gammon, single game,
    not finished, PLAYER1 single game, gammon, backgammon)"""
    env.reset()
    env.set_states(None, torch.arange(env.n, dtype=torch.int32) % 2)
    for t in range(max_turns):
        for player, pol in ((0, p1_policy), (1, p2_policy)):
            if pol[0] == "net" and temperature is not None:
                env.step_sampled(temperature, auto_reset=False, only_player=player, slot=pol[1], precision=precision)
            elif pol[0] == "net":
                env.step_greedy(auto_reset=False, only_player=player, slot=pol[1], precision=precision)
            elif pol[0] == "search":
                env.step_search(top_k=pol[2], auto_reset=False, only_player=player, slot=pol[1])
            elif pol[0] == "search3":
                env.step_search(top_k=pol[2], auto_reset=False, only_player=player, slot=pol[1], margin=pol[3], plies=3, deep_k=pol[4],
                                deep_margin=pol[5], reply_top_k=pol[6], reply_margin=pol[7])
            else:
                env.step_random(auto_reset=False, only_player=player)
        if t % 16 == 15 and bool(((env.flags() & 4) != 0).all()):
            break
    f = env.flags()
    done = (f & 4) != 0
    p1_won = done & (((f >> 1) & 1) == 0)
    pts = torch.bincount((env.outcomes() + 3).to(torch.int64), minlength=7).cpu().tolist()
    return int(done.sum()), int(p1_won.sum()), pts


def head_to_head(env: VecGame, weights_a, weights_b=None, max_turns: int = 2000, precision=F32, plies_a: int = 1, plies_b: int = 1,
                 top_k: int = 8, epsilon: float = 0.0, temperature=None, margin=None, deep_k: int = 2, deep_margin: float = float("inf"),
                 reply_top_k: int = 2, reply_margin: float = float("inf")):
    """Win rate of A vs B (B = None: a uniformly random mover), sides alternated 50/50 as in
    evaluate_parallel (train.py:296-302): every lane plays one game with A as PLAYER1 and one with A as
    PLAYER2.  plies_a / plies_b = 2: that side moves by the 2-ply search (VecGame.step_search, top_k candidates, fp32 net); = 3: by the
    3-ply step (step_search(plies=3)) with (top_k, margin, deep_k, deep_margin, reply_top_k, reply_margin).
    temperature (None = greedy): a side that moves by its net (1 ply) draws every move with probability ~ exp(value / temperature) over
    its afterstates (VecGame.step_sampled): varied games from one opening.  epsilon is accepted for symmetry with the self-play drivers
    and must be 0 beside a temperature (ValueError); the arena does not explore uniformly.
    -> dict(games, a_wins, win_rate, a_as_p1, a_as_p2) and the match in points (a single game 1, a gammon 2, a backgammon 3;
    include/bgamd.h, bgamd_env_outcomes): a_points (A's points minus B's over both passes; a lane not finished at max_turns gives 0),
    ppg (a_points / games), a_gammons, a_backgammons, b_gammons, b_backgammons (games won by that much)."""
    if plies_a not in (1, 2, 3) or plies_b not in (1, 2, 3):
        raise ValueError("plies must be 1, 2 or 3")
    if temperature is not None and epsilon:
        raise ValueError("epsilon and temperature are two ways to leave the greedy line: pass one of them")
    if epsilon:
        raise ValueError("the arena does not explore uniformly: epsilon must be 0")
    if plies_b >= 2 and weights_b is None:
        raise ValueError("a random mover does not search")
    env.load_weights(weights_a, slot=0)
    if weights_b is not None:
        env.load_weights(weights_b, slot=1)
    def policy(plies, slot):
        if plies == 3:
            return ("search3", slot, top_k, margin, deep_k, deep_margin, reply_top_k, reply_margin)
        return ("net", slot) if plies == 1 else ("search", slot, top_k)
    a = policy(plies_a, 0)
    b = policy(plies_b, 1) if weights_b is not None else ("random",)
    n1, w1, h1 = _play(env, a, b, max_turns, precision, temperature)      # A is PLAYER1
    n2, w2, h2 = _play(env, b, a, max_turns, precision, temperature)      # A is PLAYER2
    a_wins = w1 + (n2 - w2)
    h = [x + y for x, y in zip(h1, reversed(h2))]            # from A's side: the second pass sign-flipped
    a_points = sum((k - 3) * c for k, c in enumerate(h))
    return {"games": n1 + n2, "a_wins": a_wins, "win_rate": a_wins / max(n1 + n2, 1),
            "a_as_p1": (n1, w1), "a_as_p2": (n2, n2 - w2),
            "a_points": a_points, "ppg": a_points / max(n1 + n2, 1),
            "a_gammons": h[5], "a_backgammons": h[6], "b_gammons": h[1], "b_backgammons": h[0]}
