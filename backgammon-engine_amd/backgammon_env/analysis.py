"""Move analysis on top of the env: which of a turn's moves is best by rollout (include/bgamd.h, bgamd_env_rollout)."""
from __future__ import annotations

import numpy as np


def rollout_moves(env, state28, turn, dice, top_k=8, trials=1296, max_plies=0, seed=20240603, variance_reduction=False, outcomes=False):
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
    not change: it stays by mean (or vr_mean), the share of wins."""
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
                        variance_reduction=variance_reduction, outcomes=outcomes)
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
