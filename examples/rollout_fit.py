#!/usr/bin/env python3
"""Refine a value net on rollout targets, on ONE GPU: positions sampled from a greedy self-play log, a Monte Carlo rollout of each
(VecGame.rollout: rotated trials, optionally truncated and luck-adjusted), a seeded split into training and held-out positions, the
supervised fit (DeviceTDLambdaLearner.fit: bgamd_td_fit_step, csrc/bg_fit.h), the held-out mean squared error between net and rollout
mean before and after, a health line, and the arena against the starting weights.  A demonstration that the pieces compose: one run
says nothing about playing strength.

    python examples/rollout_fit.py --games 2048 --positions 4096 --trials 144 --turn-limit 8 --epochs 4
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
from backgammon_env.arena import head_to_head  # noqa: E402
from backgammon_env.learner import DeviceTDLambdaLearner, play_round  # noqa: E402


def unpack_rows(rows):
    """int32 [m, 8] 32-byte rows (csrc/bg_board.h: planes 0..3 = PLAYER1's count bits, 4..7 = PLAYER2's, bit i = position i; the turn in
    plane 0 bit 31) -> (states int32 [m, 28] in the reference's getGameBoard layout, turn int32 [m]): the inverse of bg.pack_rows"""
    r = rows.to(torch.int64) & 0xFFFFFFFF
    bits = (r[:, :, None] >> torch.arange(26, device=rows.device)) & 1                  # [m, 8, 26]
    wt = torch.tensor([1, 2, 4, 8], device=rows.device)[None, :, None]
    c1, c2 = (bits[:, :4] * wt).sum(1), (bits[:, 4:] * wt).sum(1)                       # counts per position, [m, 26]
    st = torch.zeros((rows.shape[0], 28), dtype=torch.int64, device=rows.device)
    st[:, :24] = c1[:, 1:25] - c2[:, 1:25]
    st[:, 24], st[:, 25], st[:, 26], st[:, 27] = c1[:, 0], c2[:, 25], c1[:, 25], c2[:, 0]    # bars, then borne off
    return st.to(torch.int32), ((r[:, 0] >> 31) & 1).to(torch.int32)


def held_out_mse(env, st, tu, y):
    v = env.evaluate(st, tu).double()
    return float(((v - y.double()) ** 2).mean().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=2048, help="lanes of the greedy self-play round the positions are sampled from")
    ap.add_argument("--positions", type=int, default=4096, help="positions rolled out")
    ap.add_argument("--trials", type=int, default=144, help="trials per position (rotated: trial i starts with ordered dice pair i %% 36)")
    ap.add_argument("--turn-limit", type=int, default=8, help="a trial is cut after this many turns and scored by the net (0 = played to the end)")
    ap.add_argument("--variance-reduction", action="store_true", help="luck-adjusted rollouts: the target is vr_mean")
    ap.add_argument("--held-out", type=float, default=0.2, help="share of the positions kept out of the fit")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--max-plies", type=int, default=400, help="turn log depth of the self-play round")
    ap.add_argument("--arena", type=int, default=1024, help="lanes of the arena (2 games per lane, sides alternated)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--init-weights", default=None, help="a file of 25 601 float32 (W1 | b1 | W2 | b2); default: the reference's 100k-episode checkpoint")
    a = ap.parse_args()
    w0 = np.fromfile(a.init_weights or os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)

    # 1. positions of a greedy self-play round
    env = bg.VecGame(a.games, seed=a.seed)
    env.load_weights(w0)
    rows, lengths, _ = play_round(env, max_plies=a.max_plies)
    T = int(rows.shape[0])
    inside = torch.arange(T, device=rows.device)[:, None] < lengths[None, :]              # turn t of lane g was played
    pool = rows[inside]
    gen = torch.Generator(device="cpu").manual_seed(a.seed)
    pick = torch.randperm(int(pool.shape[0]), generator=gen)[:a.positions].to(rows.device)
    st, tu = unpack_rows(pool[pick])
    assert torch.equal(bg.pack_rows(st, tu), pool[pick])
    P = int(st.shape[0])
    print(f"{int(pool.shape[0])} turns logged by {int((lengths > 0).sum())} finished games; {P} positions sampled", flush=True)

    # 2. the targets: a rollout of every position under the starting weights
    r = env.rollout(st, tu, a.trials, max_plies=a.turn_limit, rotate=True, seed=a.seed, variance_reduction=a.variance_reduction)
    y = (r["vr_mean"] if a.variance_reduction else r["mean"]).float()
    se = r["vr_stderr"] if a.variance_reduction else r["stderr"]
    print(f"rollouts: {a.trials} trials per position, turn limit {a.turn_limit}, {'luck-adjusted, ' if a.variance_reduction else ''}"
          f"median standard error {float(se.median()):.4f}, {int(r['truncated'].sum())} of {P * a.trials} trials cut", flush=True)

    # 3. training and held-out positions
    perm = torch.randperm(P, generator=torch.Generator(device="cpu").manual_seed(a.seed + 1)).to(rows.device)
    n_held = max(1, int(round(a.held_out * P)))
    held, train = perm[:n_held], perm[n_held:]

    # 4. the held-out error before, the fit, the held-out error after
    before = held_out_mse(env, st[held], tu[held], y[held])
    print(f"held-out mse before the fit: {before:.6g} ({n_held} positions)", flush=True)
    L = DeviceTDLambdaLearner(w0, max_games=64, alpha=a.alpha)
    mse = L.fit(st[train], tu[train], y[train], epochs=a.epochs, batch=a.batch, seed=a.seed)
    print("training mse per epoch: " + " ".join(f"{m:.6g}" for m in mse) + f" ({int(train.numel())} positions, batch {a.batch})", flush=True)
    w1 = L.theta.cpu().numpy()
    env.load_weights(w1)
    after = held_out_mse(env, st[held], tu[held], y[held])
    print(f"held-out mse after the fit: {after:.6g}", flush=True)

    # 5. the net's health on the training rows, 6. the arena against the starting weights
    print(nh.line(nh.net_health(L.theta, bg.pack_rows(st[train], tu[train]))), flush=True)
    res = head_to_head(bg.VecGame(a.arena, seed=2), w1, w0)
    print("arena, fitted vs starting weights:", {k: res[k] for k in ("games", "a_wins", "win_rate")}, f"{res['ppg']:+.4f} points per game", flush=True)
    print("done", flush=True)


if __name__ == "__main__":
    main()
