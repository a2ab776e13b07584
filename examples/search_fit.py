#!/usr/bin/env python3
"""Fit a value net to its own 2-ply search, on ONE GPU.  Every round: one game per lane played by the search step from the current
weights and logged by the search log (learner.play_round_search: VecGame.record_search_log, bgamd_env_set_search_log); optionally a
TD(lambda) replay of those games (--td); the supervised fit of the played afterstates to their 2-ply values V2
(DeviceTDLambdaLearner.fit_search) on the training lanes; a health line; and a report line: how far the lookahead disagrees with the net
(mean |V2 - v1| over the searched turns), the squared error between net and search target on the held-out lanes before and after, and
the turns the fit skipped (not searched: their target is NaN).  At the end: the error rate of the new table judged by the starting one
(analysis.error_rate) and the arena against the starting table.  A demonstration that the pieces compose: one run says nothing about
playing strength.

    python examples/search_fit.py --games 4096 --rounds 4 --top-k 5 --margin 0.04 --td
"""
import argparse
import os
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")      # before the HIP runtime starts: backgammon_env/__init__.py says why
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "backgammon-engine_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import backgammon_env as bg  # noqa: E402
from backgammon_env import health as nh  # noqa: E402
from backgammon_env.analysis import error_rate  # noqa: E402
from backgammon_env.arena import head_to_head  # noqa: E402
from backgammon_env.learner import DeviceTDLambdaLearner, play_round_search  # noqa: E402
from rollout_fit import unpack_rows  # noqa: E402  (examples/rollout_fit.py: the inverse of bg.pack_rows)


def search_mse(env, after, target):
    """mean squared error between the net in `env` and the search targets, over the entries whose target is a number"""
    ok = torch.isfinite(target)
    if not bool(ok.any()):
        return float("nan"), 0
    st, tu = unpack_rows(after[ok])
    v = env.evaluate(st, tu).double()
    return float(((v - target[ok].double()) ** 2).mean().item()), int(ok.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096, help="lanes: one searched game per lane and round")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--top-k", type=int, default=5, help="candidates the search keeps per turn (0 = every distinct afterstate)")
    ap.add_argument("--margin", type=float, default=0.04, help="the filtered step's margin; negative: the unfiltered step")
    ap.add_argument("--max-plies", type=int, default=400, help="log depth: a game still running after this many turns is left out")
    ap.add_argument("--td", action="store_true", help="also replay the round's games by TD(lambda) before the fit")
    ap.add_argument("--held-out", type=float, default=0.2, help="share of the lanes kept out of the fit")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--judge-turns", type=int, default=32, help="turns of the closing error-rate run")
    ap.add_argument("--arena", type=int, default=1024, help="lanes of the arena (2 games per lane, sides alternated)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--init-weights", default=None, help="a file of 25 601 float32 (W1 | b1 | W2 | b2); default: the reference's 100k-episode checkpoint")
    a = ap.parse_args()
    w0 = np.fromfile(a.init_weights or os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)
    margin = a.margin if a.margin >= 0 else None

    env = bg.VecGame(a.games, seed=a.seed)
    L = DeviceTDLambdaLearner(w0, max_games=a.games, alpha=a.alpha)
    perm = torch.randperm(a.games, generator=torch.Generator(device="cpu").manual_seed(a.seed)).to(env.device)
    held = torch.zeros(a.games, dtype=torch.bool, device=env.device)
    held[perm[:max(1, int(round(a.held_out * a.games)))]] = True
    w = w0
    for rnd in range(a.rounds):
        env.load_weights(w)
        rows, lengths, p1_won, after, target, v1 = play_round_search(env, max_plies=a.max_plies, top_k=a.top_k, margin=margin, episode=rnd)
        T = int(rows.shape[0])
        inside = torch.arange(T, device=rows.device)[:, None] < lengths[None, :]             # turn t of lane g was played and logged
        searched = inside & torch.isfinite(target)
        gap = float((target[searched] - v1[searched]).abs().mean()) if bool(searched.any()) else float("nan")
        h_in = inside & held[None, :]
        before, n_held = search_mse(env, after[h_in], target[h_in])
        td = ""
        if a.td:
            sq, cnt = L.replay_rows(rows, lengths, p1_won, batch_scale=24.0 / a.games)
            td = f", TD replay of {cnt} turns (mean delta^2 {sq / max(cnt, 1):.6g})"
        train_len = torch.where(held, torch.zeros_like(lengths), lengths)
        mse = L.fit_search(after, target, train_len, epochs=a.epochs, batch=a.batch, seed=a.seed + rnd)
        _, counted, skipped = L.last_fit_stats                 # what fit_stats reported over the epochs
        w = L.theta.cpu().numpy()
        env.load_weights(w)
        after_mse, _ = search_mse(env, after[h_in], target[h_in])
        print(nh.line(nh.net_health(L.theta, after[inside & ~held[None, :]])), flush=True)
        print(f"round {rnd}: {int((lengths > 0).sum())} games, {int(inside.sum())} turns, {int(searched.sum())} searched, mean |V2 - v1| {gap:.6f}; "
              f"held-out mse against the search targets {before:.6g} -> {after_mse:.6g} ({n_held} turns); fit: training mse per epoch "
              + " ".join(f"{m:.6g}" for m in mse) + f", {counted} rows counted, {skipped} skipped (not searched){td}", flush=True)

    player, judge = bg.VecGame(a.arena, seed=3), bg.VecGame(a.arena, seed=3)
    player.load_weights(w)
    judge.load_weights(w0)
    er = error_rate(player, judge, a.judge_turns, top_k=a.top_k or 8)["total"]
    print(f"the new table judged by the starting one over {a.judge_turns} turns: error rate {er['error_rate']:.6f}, agreement {er['agreement']:.4f} "
          f"({er['unforced']} unforced decisions)", flush=True)
    res = head_to_head(bg.VecGame(a.arena, seed=2), w, w0)
    print("arena, fitted vs starting weights:", {k: res[k] for k in ("games", "a_wins", "win_rate")}, f"{res['ppg']:+.4f} points per game", flush=True)
    print("done", flush=True)


if __name__ == "__main__":
    main()
