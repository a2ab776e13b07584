#!/usr/bin/env python3
"""What profiles/net_health_rounds.txt holds ("net health"):
  1. the health lines of examples/selfplay_train.py for the classic loop from xavier_init at --max-plies 400 (the gate's healthy
     configuration) and at --max-plies 600 (the collapsing one: once with the all-tied limit off, once as the example stops it),
     65 536 games per round, each in a child process of its own;
  2. the checkpoint tdgammonNEW100k on one round's rows, with the choice spread of a mid-game step;
  3. the time of one bgamd_net_health call on 65 536 rows and of one bgamd_env_choice_spread at 65 536 lanes (HIP events, median of
     --reps), beside the time of one training round (self-play + streamed replay) of the same run.

    python tools/net_health_profile.py [--rounds 16] [--games 65536] > profiles/net_health_rounds.txt
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "backgammon-engine_amd")):
    sys.path.insert(0, p)


def loop(a, max_plies, *more):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "selfplay_train.py"), "--games", str(a.games), "--rounds", str(a.rounds),
           "--max-plies", str(max_plies), "--slots", "2048", "--scale-games", "96", "--verbose", *more]
    print("$ python examples/selfplay_train.py " + " ".join(cmd[2:]), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    for ln in (r.stdout + r.stderr).splitlines():
        if ln.strip() and "amdgpu.ids" not in ln:             # (libdrm's complaint about a missing id table: not the example's)
            print("    " + ln)
    print("    exit code %d" % r.returncode, flush=True)
    if r.returncode not in (0, 3):                            # 3 = stopped by the health check; anything else: nothing more is started
        sys.exit("the loop failed: profile abandoned")


def events_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=16, help="rounds of each loop (the gate's 16: the exploration schedule is the gate's)")
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    print("# net health per round: the classic loop from xavier_init, %d games per round" % a.games)
    print("## --max-plies 400 (healthy)")
    loop(a, 400)
    print("## --max-plies 600 (collapsing), the all-tied limit off so that every round is on record")
    loop(a, 600, "--max-all-tied-share", "1")
    print("## --max-plies 600 as the example runs it: stopped by the all-tied limit")
    loop(a, 600)

    import ctypes as C
    import numpy as np
    import torch
    import backgammon_env as bg
    from backgammon_env import _capi, health
    from backgammon_env.learner import DeviceTDLambdaLearner, play_round
    lib = _capi.load()
    print("## the checkpoint tdgammonNEW100k on one round's rows (source digest %s)" % _capi.source_hash())
    w = np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)
    env = bg.VecGame(a.games, seed=1)
    env.load_weights(w)
    env.run_greedy(20, auto_reset=True)                       # a mid-game step of every lane
    sp_mid = env.choice_spread()
    torch.cuda.synchronize()
    t0 = time.time()
    traj, lengths, won = play_round(env, max_plies=400)
    torch.cuda.synchronize()
    t_play = time.time() - t0
    sp_last = env.choice_spread()
    rows = health.round_rows(traj, lengths, a.games)          # spread over all the round's turns
    h = health.net_health(w, rows)
    print("    " + health.line(h, sp_last) + " (the round's last step)")
    print("    mid-game step (env step 20 of every lane): all-tied share %.4f of %d lanes with a choice, %d rows"
          % (health.all_tied_share(sp_mid), sp_mid["choice_lanes"], sp_mid["rows"]))
    L = DeviceTDLambdaLearner(w, max_games=a.games)
    L.update_learning_params(0)
    torch.cuda.synchronize()
    t0 = time.time()
    L.replay_rows(traj, lengths, won, batch_scale=96.0 / 2048, slots=2048)
    torch.cuda.synchronize()
    t_replay = time.time() - t0

    print("## cost (HIP events, median [min, max] of %d calls)" % a.reps)
    theta = torch.from_numpy(w).cuda()
    out = torch.empty(C.sizeof(_capi.NetHealth), dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = int(rows.shape[0])
    t_h = events_ms(lambda: lib.bgamd_net_health(C.c_void_p(theta.data_ptr()), C.c_void_p(rows.data_ptr()), n, 15.0,
                                                 C.c_void_p(out.data_ptr()), s), a.reps)
    t_w = events_ms(lambda: lib.bgamd_net_health(C.c_void_p(theta.data_ptr()), None, 0, 15.0, C.c_void_p(out.data_ptr()), s), a.reps)
    env.reset()
    env.run_greedy(20, auto_reset=True)
    cnt, tied = torch.empty(a.games, dtype=torch.int32, device="cuda"), torch.empty(a.games, dtype=torch.int32, device="cuda")
    best, worst = torch.empty(a.games, device="cuda"), torch.empty(a.games, device="cuda")
    summ = torch.empty(4, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    t_s = events_ms(lambda: lib.bgamd_env_choice_spread(env._h, p(cnt), p(best), p(worst), p(tied), p(summ), s), a.reps)
    rnd = 1e3 * (t_play + t_replay)
    print("    bgamd_net_health, %d rows          : %.4f ms [%.4f, %.4f]" % ((n,) + t_h))
    print("    bgamd_net_health, weights only        : %.4f ms [%.4f, %.4f]" % t_w)
    print("    bgamd_env_choice_spread, %d lanes  : %.4f ms [%.4f, %.4f]  (%d rows)" % ((a.games,) + t_s + (int(summ[2].item()),)))
    print("    one training round of the same run    : %.1f ms (self-play %.1f + replay through 2 048 slots %.1f, wall clock)"
          % (rnd, 1e3 * t_play, 1e3 * t_replay))
    print("    share of a round: health %.4f %%, spread %.4f %%" % (100 * t_h[0] / rnd, 100 * t_s[0] / rnd))


if __name__ == "__main__":
    main()
