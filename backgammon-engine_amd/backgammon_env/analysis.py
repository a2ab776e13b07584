"""Move analysis on top of the env: which of a turn's moves is best by rollout (include/bgamd.h, bgamd_env_rollout), how much a
player's moves lose against a 2-ply judge (bgamd_env_analyze_moves), and the cube action of a position by cubeful rollout
(bgamd_env_rollout_cube)."""
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


def rollout_decisions(env, top_k=8, trials=1296, max_plies=0, seed=20240603, variance_reduction=False, outcomes=False, plies=1,
                      rollout_top_k=4, rollout_margin=float("inf"), group_offset=0):
    """rollout_moves for every lane of an env at once: one search step, ONE rollout call over all candidates of all decisions, and the
    paired statistics that common dice are for.

    env: an n-lane VecGame with weights in slot 0.  Its lanes hold the decisions as they stand: board, side to move, set dice
    (set_states / set_dice, or wherever play left them).  One step_search(top_k, roll=False, auto_reset=False, no_flip=True) over all
    lanes lists every lane's kept candidates; afterwards every lane's board, side to move and dice are put back with set_states /
    set_dice, as rollout_moves does for its one lane (last_choice / search_candidates then describe this search).
    All kept candidates of all lanes form one position list, the opponent to move, the lane index as dice group: VecGame.rollout(groups=
    lane, group_offset=group_offset) rolls them out in one call -- `trials` rotated trials, turn limit max_plies --, trial i of every
    candidate of lane g on the dice of game id (group_offset + g) * trials + i.  Lane 0 at group_offset 0 therefore plays exactly the
    trials rollout_moves plays for that decision.  plies / rollout_top_k / rollout_margin: who plays the trials, as there.

    -> one list per lane, best first by the rule of rollout_moves (mean, or vr_mean under variance_reduction, for the lane's mover; ties
    keep the search's order).  Every entry carries rollout_moves' fields -- index, seq, state, v1, v2, mean, stderr, turns, with
    variance_reduction vr_mean, vr_stderr, with outcomes equity, equity_stderr, counts -- and, against the lane's best entry b over the
    same trials (VecGame.rollout_paired; of the values, or of the luck-adjusted values under variance_reduction):
      diff         mean of the per-trial differences q_i(candidate) - q_i(b): <= 0 for PLAYER1's rivals, >= 0 for PLAYER2's (up to ties);
      diff_stderr  their standard error -- the paired one, which credits the shared dice;
      jsd          |diff| / diff_stderr, the joint standard deviations the candidate lies behind the best: 0.0 for the best itself and
                   where diff is 0, inf where diff_stderr is 0 and diff is not.
    A lane whose search keeps no candidate gives an empty list.  By the search step's contract (bgamd_env_search_info: "lanes that had
    a move" are those with kept >= 1) that is a lane whose mover has no legal move with its two different dice (a pass), and a frozen
    lane -- a game that finished without auto_reset takes no part in any step.  A DOUBLES roll without a move is not such a lane: the
    reference's enumeration lists one empty sequence for it, the board itself, the search keeps it, and the lane's list is that one
    entry (seq [], the board rolled out with the opponent to move).  Every lane's board, side to move and dice are put back alike;
    set_states lifts a frozen lane's frozen mark (flags bit 2), here as everywhere."""
    n = env.n
    saved = env.snapshot().cpu().numpy()
    movers = saved[:, 28].astype(np.int64)
    try:
        offs, cnts, st, sq, ln = (x.cpu().numpy() for x in env.enumerate())
        env.step_search(top_k=top_k, roll=False, auto_reset=False, no_flip=True)
        cst, v1, v2, kept = (x.cpu().numpy() for x in env.search_candidates())
    finally:
        env.set_states(saved[:, :28], saved[:, 28])
        env.set_dice(saved[:, 29:31])
    lanes = [g for g in range(n) for _ in range(int(kept[g]))]
    slots = [k for g in range(n) for k in range(int(kept[g]))]
    out = [[] for _ in range(n)]
    if not lanes:
        return out
    after = cst[lanes, slots]
    r = env.rollout(after, [1 - int(movers[g]) for g in lanes], trials, max_plies=max_plies, rotate=True, seed=seed,
                    variance_reduction=variance_reduction, outcomes=outcomes, plies=plies, top_k=rollout_top_k, margin=rollout_margin,
                    groups=lanes, group_offset=group_offset)
    key = "vr_mean" if variance_reduction else "mean"
    h = {k: v.cpu().numpy() for k, v in r.items()}
    flat = [[] for _ in range(n)]
    for q, g in enumerate(lanes):
        flat[g].append(q)
    for g in range(n):                                     # (a stable sort, as rollout_moves': ties keep the search's order)
        flat[g].sort(key=lambda q: -h[key][q] if movers[g] == 0 else h[key][q])
    ref = [flat[g][0] for g in lanes]
    dm, ds = (x.cpu().numpy() for x in env.rollout_paired(ref, "vr" if variance_reduction else "value"))
    for g in range(n):
        rows = st[offs[g]:offs[g] + cnts[g]]
        for q in flat[g]:
            a = after[q]
            idx = int(offs[g]) + int(np.flatnonzero((rows == a).all(axis=1))[0])
            c = {"index": idx - int(offs[g]), "seq": [tuple(int(x) for x in sq[idx, m]) for m in range(int(ln[idx]))], "state": a,
                 "v1": float(v1[g, slots[q]]), "v2": float(v2[g, slots[q]]), "mean": float(h["mean"][q]),
                 "stderr": float(h["stderr"][q]), "turns": int(h["turns"][q])}
            if variance_reduction:
                c.update(vr_mean=float(h["vr_mean"][q]), vr_stderr=float(h["vr_stderr"][q]))
            if outcomes:
                c.update(equity=float(h["equity"][q]), equity_stderr=float(h["equity_stderr"][q]), counts=[int(x) for x in h["counts"][q]])
            d, se = float(dm[q]), float(ds[q])
            c.update(diff=d, diff_stderr=se, jsd=0.0 if d == 0.0 else (math.inf if se == 0.0 else abs(d) / se))
            out[g].append(c)
    return out


CUBE_ACTIONS = ("no double, take", "double, take", "double, pass", "too good, pass", "too good, take")


def cube_decision(nd, dt, dp):
    """GNU Backgammon's cube action table on three cubeful equities from the roller's side: nd (no double), dt (double / take), dp
    (double / pass = the cube's value).  The opponent takes iff dt <= dp; the roller doubles iff the better of the opponent's answers
    still beats nd.  -> one of CUBE_ACTIONS"""
    if dt <= dp:                                           # the take is right
        if dt > nd:
            return "double, take"
        return "too good, take" if nd > dp else "no double, take"
    return "too good, pass" if nd > dp else "double, pass"


def cube_action(env, states28, turn, cube_value=1, cube_owner=0, trials=1296, max_plies=0, plies=1, rollout_top_k=4,
                rollout_margin=float("inf"), seed=20240603, group_offset=0, lanes=0, cube=None, match=None):
    """Double or not, take or pass: the cube action of each position by ONE grouped cubeful rollout.

    env: a VecGame with weights in slot 0 (its lanes are untouched).  states28 [P, 28] / turn [P]: the positions, `turn` to roll and
    to decide.  cube_value / cube_owner (scalars or [P]): the cube as it stands, c and 0 = centre, 1 = PLAYER1, 2 = PLAYER2.
    cube: the rule the trials handle the cube by afterwards (a backgammon_env.Cube or a dict of its fields; value, owner and hold_turn0
    are set here; jacoby is refused -- the rule counts cube turns inside a trial, and the double under analysis is made before it).
    Every position whose roller has access to the cube appears twice in the rollout, in the same dice group (its index, counted from
    group_offset): as it stands with no decision before turn 0 ("no double": the roller holds the cube this turn, and the rule applies
    from the opponent's turn on), and with cube 2 c owned by the opponent ("double / take").  `trials` rotated trials each, turn limit
    max_plies (0 = to the end), played by the greedy step or, plies = 2, by the filtered 2-ply search (rollout_top_k, rollout_margin).

    -> one dict per position, every equity in points from the ROLLER's side:
         nd, nd_stderr    cubeful equity of not doubling;  dt, dt_stderr  of double / take;  dp = +c  of double / pass;
         diff, diff_stderr, jsd   the paired dt - nd over the shared dice (VecGame.rollout_paired(which="cubeful")), its standard error,
                          and |diff| / diff_stderr (0.0 where diff is 0, inf where only diff_stderr is);
         cubeless, cubeless_stderr   the cubeless equity of the no-double copy's trials;  shares: win, win_gammon, win_backgammon,
                          lose, lose_gammon, lose_backgammon as fractions of the trials (gammons include backgammons; truncated
                          trials are in none);
         action           one of CUBE_ACTIONS by cube_decision(nd, dt, dp).
       A position whose roller has no access to the cube carries nd (and the cubeless fields) only, with action "no access"; a
       position that is already over likewise, with action "game over".

    match (a backgammon_env.Match, its scores scalars or one per position): the same at a match score (VecGame.rollout(match=...)).
    nd, dt, dp, diff and their standard errors are then the ROLLER's match-winning chances instead of points -- dp = W(c), the
    roller's chance after winning the cube's value, from the roller's own row of the table as the thresholds read it (nd and dt
    of a PLAYER2 roller are 1 - PLAYER1's chance, the payoff being PLAYER1's: on a table that is not complementary the two views
    differ); diff is the paired dt - nd of the trials' MWC
    (rollout_paired(which="mwc")) --, cube_decision is applied to them unchanged, and `mwc` is PLAYER1's chance of the no-double
    copy.  The cube's double_at and pass_at are ignored by the trials (the thresholds follow from the score).  A position in the
    Crawford game carries nd only with action "Crawford game", one whose cube is dead for the roller (c >= its points to go)
    likewise with action "dead cube"."""
    from . import Cube
    st = np.asarray(states28.cpu() if hasattr(states28, "cpu") else states28, dtype=np.int32).reshape(-1, 28)
    P = st.shape[0]
    tu = np.broadcast_to(np.asarray(turn.cpu() if hasattr(turn, "cpu") else turn, dtype=np.int64), (P,))
    cv = np.broadcast_to(np.asarray(cube_value, dtype=np.int64), (P,))
    co = np.broadcast_to(np.asarray(cube_owner, dtype=np.int64), (P,))
    rule = cube if isinstance(cube, Cube) else Cube(**(cube or {}))
    if rule.jacoby:
        raise ValueError("cube_action: the Jacoby rule counts cube turns inside a trial; the double under analysis is made before it")
    over = (st[:, 26] == 15) | (st[:, 27] == 15)
    access = ((co == 0) | (co == tu + 1)) & ~over
    label = {}
    if match is not None:
        a1, a2, ms = (x.astype(np.int64) for x in match.per_position(P))
        mine = np.where(tu == 0, a1, a2)
        for p in np.flatnonzero(access & ((ms == 1) | (cv >= mine))):
            label[int(p)] = "Crawford game" if ms[p] == 1 else "dead cube"
        access = access & ~((ms == 1) | (cv >= mine))
    nd_of = list(range(P))
    dt_of = {}
    rows, turns, values, owners, groups = list(range(P)), list(tu), list(cv), list(co), list(range(P))
    for p in np.flatnonzero(access):
        dt_of[int(p)] = len(rows)
        rows.append(int(p)); turns.append(tu[p]); values.append(2 * cv[p]); owners.append(2 - tu[p]); groups.append(int(p))
    rule = Cube(rule.double_at, rule.pass_at, rule.too_good_at, rule.max_cube, False, True, np.asarray(values), np.asarray(owners))
    if match is not None:
        from .match import Match
        match = Match(match.table, a1[rows], a2[rows], ms[rows], match.window_share)
    r = env.rollout(st[rows], np.asarray(turns), trials, max_plies=max_plies, rotate=True, seed=seed, lanes=lanes, variance_reduction=True,
                    outcomes=True, plies=plies, top_k=rollout_top_k, margin=rollout_margin, groups=groups, group_offset=group_offset,
                    cube=rule, match=match)
    ref = [nd_of[g] for g in groups]                       # every copy against its position's no-double copy
    dm, ds = (x.cpu().numpy() for x in env.rollout_paired(ref, "cubeful" if match is None else "mwc"))
    h = {k: v.cpu().numpy() for k, v in r.items()}
    T = float(int(trials))
    out = []
    for p in range(P):
        sg = 1.0 if tu[p] == 0 else -1.0
        cnt = h["counts"][p] if tu[p] == 0 else np.concatenate([h["counts"][p][3:], h["counts"][p][:3]])
        e = {"nd": sg * float(h["cubeful"][p]), "nd_stderr": float(h["cubeful_stderr"][p]),
             "cubeless": sg * float(h["equity"][p]), "cubeless_stderr": float(h["equity_stderr"][p]),
             "shares": {"win": int(cnt[:3].sum()) / T, "win_gammon": int(cnt[1:3].sum()) / T, "win_backgammon": int(cnt[2]) / T,
                        "lose": int(cnt[3:].sum()) / T, "lose_gammon": int(cnt[4:].sum()) / T, "lose_backgammon": int(cnt[5]) / T}}
        if match is not None:                              # the roller's match-winning chance: PLAYER2 sees 1 - PLAYER1's
            side = (lambda x: x) if tu[p] == 0 else (lambda x: 1.0 - x)
            e.update(nd=side(float(h["mwc"][p])), nd_stderr=float(h["mwc_stderr"][p]), mwc=float(h["mwc"][p]))
        if p in dt_of:
            q = dt_of[p]
            d, se = sg * float(dm[q]), float(ds[q])
            if match is None:
                e.update(dt=sg * float(h["cubeful"][q]), dt_stderr=float(h["cubeful_stderr"][q]), dp=float(cv[p]))
            else:
                c = int(cv[p])
                mine, yours = (int(a1[p]), int(a2[p])) if tu[p] == 0 else (int(a2[p]), int(a1[p]))
                e.update(dt=side(float(h["mwc"][q])), dt_stderr=float(h["mwc_stderr"][q]),
                         dp=match.table.after(mine - c, yours, int(ms[p])))      # W(c) from the roller's own row, as the thresholds read it
            e.update(diff=d, diff_stderr=se, jsd=0.0 if d == 0.0 else (math.inf if se == 0.0 else abs(d) / se))
            e["action"] = cube_decision(e["nd"], e["dt"], e["dp"])
        else:
            e["action"] = "game over" if over[p] else label.get(p, "no access")
        out.append(e)
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
