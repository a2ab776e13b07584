"""Move analysis on top of the env: which of a turn's moves is best by rollout (include/bgamd.h, bgamd_env_rollout), and how much a
player's moves lose against a 2-ply judge (bgamd_env_analyze_moves)."""
from __future__ import annotations

import math

import numpy as np


def rollout_moves(env, state28, turn, dice, top_k=8, trials=1296, max_plies=0, seed=20240603, variance_reduction=False, outcomes=False,
                  plies=1, rollout_top_k=4, rollout_margin=float("inf")):
    """Rolls out the candidates a 2-ply search keeps for one turn and ranks them by rollout.

    env: a one-lane VecGame with weights in slot 0.  Its lane is set to the position and searched; its board, turn and dice are
    restored afterwards (last_choice / search_candidates then describe this search).
    The kept candidates of one search step (step_search(top_k) with the given dice, no_flip) are each rolled out with the
    opponent to move: `trials` rotated trials, turn limit max_plies (0 = to the end).  Every candidate is rolled out with the
    same trial ids (position_offset 0): common dice, so their difference is measured more tightly than either mean.

    -> list of dicts, best rollout mean for the mover first (PLAYER1: highest share of PLAYER1 wins; PLAYER2: lowest; ties keep
    the search's order): index (first reference-order index of the move in `enumerate`), seq (the move's (origin, dest) pairs),
    state (afterstate, int32[28]), v1, v2 (the search's 1- and 2-ply values), mean, stderr, turns (rollout statistics).
    variance_reduction: every candidate also carries vr_mean, vr_stderr (luck-adjusted rollouts, BGAMD_ROLLOUT_VR), and the list is
    ranked by vr_mean instead.
    outcomes: every candidate also carries equity, equity_stderr (PLAYER1's cubeless equity in points: gammons 2, backgammons 3) and
    counts (trials that ended as PLAYER1 single game, gammon, backgammon, PLAYER2 single game, gammon, backgammon).  The ranking does
    not change: it stays by mean (or vr_mean), the share of wins.
    plies = 2: the trials are played by the filtered 2-ply search with (rollout_top_k, rollout_margin) instead of the greedy step
    (VecGame.rollout(plies=2)): "roll it out at 2 plies"."""
    if env.n != 1:
        raise ValueError("rollout_moves needs a one-lane VecGame")
    mover = int(turn)
    s28 = np.asarray(state28, dtype=np.int32).reshape(28)
    d = np.asarray(dice, dtype=np.int32).reshape(1, 2)
    saved = env.snapshot().cpu().numpy()[0]
    try:
        env.set_states(s28[None], [mover])
        env.set_dice(d)
        _, _, st, sq, ln = env.enumerate()
        st, sq, ln = st.cpu().numpy(), sq.cpu().numpy(), ln.cpu().numpy()
        env.step_search(top_k=top_k, roll=False, auto_reset=False, no_flip=True)
        cst, v1, v2, kept = (x.cpu().numpy() for x in env.search_candidates())
    finally:
        env.set_states(saved[None, :28], [int(saved[28])])
        env.set_dice(saved[None, 29:31])
    out = []
    for k in range(int(kept[0])):
        after = cst[0, k]
        idx = int(np.flatnonzero((st == after).all(axis=1))[0])
        r = env.rollout(after[None], [1 - mover], trials, max_plies=max_plies, rotate=True, seed=seed,
                        variance_reduction=variance_reduction, outcomes=outcomes, plies=plies, top_k=rollout_top_k,
                        margin=rollout_margin)
        out.append({"index": idx, "seq": [tuple(int(x) for x in sq[idx, m]) for m in range(int(ln[idx]))], "state": after,
                    "v1": float(v1[0, k]), "v2": float(v2[0, k]), "mean": float(r["mean"][0]), "stderr": float(r["stderr"][0]),
                    "turns": int(r["turns"][0])})
        if variance_reduction:
            out[-1].update(vr_mean=float(r["vr_mean"][0]), vr_stderr=float(r["vr_stderr"][0]))
        if outcomes:
            out[-1].update(equity=float(r["equity"][0]), equity_stderr=float(r["equity_stderr"][0]),
                           counts=[int(x) for x in r["counts"][0].cpu().tolist()])
    key = "vr_mean" if variance_reduction else "mean"
    out.sort(key=lambda c: -c[key] if mover == 0 else c[key])
    return out


def error_rate(player, judge, turns, top_k=4, epsilon=0.0, player_slot=0, judge_slot=0, on_turn=None, temperature=None):
    """How much the player's moves lose by the judge's 2-ply search, over `turns` turns of every lane of `player`.

    player, judge: two VecGames with the same lane count; the player's weights in its slot player_slot play (one greedy step per turn
    with rolled dice, exploring with probability epsilon), the judge's weights in its slot judge_slot judge.  Each turn the judge's lanes
    are set to the player's boards, sides to move and the dice the step played, and analyze_moves(top_k) scores the boards the step
    reached (a game that ends stays on its final board for this, then restarts).  The judge is never stepped; the player plays on from
    wherever it stands and is left wherever the last turn took it.
    on_turn(turn, player, result): called after every turn's analysis with the analyze_moves result (device tensors).
    temperature (None = greedy / epsilon): the player's moves are drawn with probability ~ exp(value / temperature) over its afterstates
    (VecGame.step_sampled) instead; with epsilon > 0 as well: ValueError.

    -> dict: player1 / player2 / total, each a dict of
         decisions (moves analysed), unforced (of those: more than one afterstate), mistakes (error > 0), error_sum,
         error_rate = error_sum / unforced, agreement = 1 - mistakes / unforced (nan without an unforced decision),
         passes (turns without a legal move), illegal (played boards the judge does not list: must be 0), idle (lanes that took no part)
       and lane_turns = lanes x turns = decisions + passes + illegal + idle of total."""
    if player.n != judge.n:
        raise ValueError("error_rate needs two VecGames of equal lane count")
    if temperature is not None and epsilon:
        raise ValueError("epsilon and temperature are two ways to leave the greedy line: pass one of them")
    import torch
    counts = np.zeros((2, 6), np.int64)                    # per mover: decisions, unforced, mistakes, passes, illegal, idle
    sums = ([], [])
    for t in range(int(turns)):
        pre, mover = player.states(), player.turns()
        if temperature is not None:
            player.step_sampled(temperature, roll=True, auto_reset=False, slot=player_slot)
        else:
            player.step_greedy(roll=True, auto_reset=False, epsilon=epsilon, slot=player_slot)
        judge.set_states(pre, mover)
        judge.set_dice(player.dice())
        res = judge.analyze_moves(player.states(), top_k=top_k, slot=judge_slot)
        by = torch.bincount(res["status"].long() * 2 + mover.long(), minlength=8).cpu().numpy().reshape(4, 2)
        for side, name in enumerate(("player1", "player2")):
            s = res["summary"][name]
            counts[side] += (s["decisions"], s["unforced"], s["mistakes"], by[2, side], by[3, side], by[1, side])
            sums[side].append(s["error_sum"])
        if on_turn is not None:
            on_turn(t, player, res)
        player.reset(mask=(player.flags() & 4) != 0)

    def side(c, err):
        unforced = int(c[1])
        return {"decisions": int(c[0]), "unforced": unforced, "mistakes": int(c[2]), "error_sum": err,
                "error_rate": err / unforced if unforced else math.nan, "agreement": 1.0 - int(c[2]) / unforced if unforced else math.nan,
                "passes": int(c[3]), "illegal": int(c[4]), "idle": int(c[5])}
    return {"player1": side(counts[0], math.fsum(sums[0])), "player2": side(counts[1], math.fsum(sums[1])),
            "total": side(counts.sum(0), math.fsum(sums[0] + sums[1])), "lane_turns": player.n * int(turns)}
