"""Throughput of the 2-ply expectimax step (bgamd_env_step_search): searched moves/s and virtual roots/s at several env sizes and
top_k, set against the greedy step's env steps/s measured in the same run.  Every figure is the median of several timed regions
after a warm-up (HIP events around `--steps` back-to-back steps).  One JSON line per configuration, then a summary line.

--margin M[,M...]: after each unfiltered configuration, the filtered step (bgamd_env_step_search_filtered) with each margin from the same
starting positions: ms per step, the virtual roots scored, the lanes searched and the kept candidates of the last step
(bgamd_env_search_info), and the share of lanes whose choice differs from the unfiltered step's on one common set of positions and dice.

--log: what the search log's pass (bgamd_env_set_search_log, csrc/bg_search_log.h) costs a step -- the filtered step at 65 536 lanes,
top_k 5, margin 0.04, without auto-reset, from the same positions with and without the log set, alternating; one JSON line.

--plies 3: the 3-ply step (bgamd_env_step_search3) instead -- per size and top_k, with --margin's first margin (default 0.04) and
--deep-k / --deep-margin / --reply-k / --reply-margin: ms per step, ms per level-3 root, the mid lanes, the level-3 roots and the lanes
searched at 3 plies of the last step (bgamd_env_search3_info), and the share of lanes whose choice differs from the filtered 2-ply step's
on one common set of positions and dice.  The filtered 2-ply step with the same (top_k, margin) is timed in the same session from the same
starting positions: it is the yardstick."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "backgammon-engine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _time(fn, steps, warmup, regions):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    return statistics.median(ms), ms


def log_cost(a):
    """the filtered step with and without the search log, alternating: every region starts from the same positions (10 greedy steps past
    the opening; the log is set after them -- a greedy step is refused while it is set) and times `steps` back-to-back search steps"""
    import backgammon_env as bg
    n, top_k, margin, steps = 65536, 5, 0.04, a.steps
    w = np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)
    env = bg.VecGame(n, seed=1)
    env.load_weights(w)
    ms = {False: [], True: []}
    for region in range(-a.warmup, a.regions):
        for logged in ((False, True) if region % 2 == 0 else (True, False)):
            env.reset()
            env.run_greedy(10, auto_reset=False)
            if logged:
                env.record_search_log(10 + steps)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                env.step_search(top_k=top_k, auto_reset=False, margin=margin)
            t1.record()
            t1.synchronize()
            if logged:
                env.record_search_log(None)
            if region >= 0:
                ms[logged].append(t0.elapsed_time(t1) / steps)
    env.close()
    plain, logd = statistics.median(ms[False]), statistics.median(ms[True])
    print(json.dumps({"search_log_cost": {"n": n, "top_k": top_k, "margin": margin, "steps_per_region": steps, "regions": a.regions,
                                          "ms_per_step_without_log": round(plain, 4), "ms_per_step_with_log": round(logd, 4),
                                          "difference_ms": round(logd - plain, 4), "bytes_per_lane_and_step": 72,
                                          "regions_ms_without": [round(x, 4) for x in ms[False]],
                                          "regions_ms_with": [round(x, 4) for x in ms[True]]}}))


def three_plies(a):
    import backgammon_env as bg
    w = np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)
    mg = [float(x) for x in a.margin.split(",") if x][0] if a.margin else 0.04
    deep = dict(deep_k=a.deep_k, deep_margin=a.deep_margin, reply_top_k=a.reply_k, reply_margin=a.reply_margin)
    out = []
    for n in [int(x) for x in a.sizes.split(",")]:
        env = bg.VecGame(n, seed=1)
        env.load_weights(w)
        for k in [int(x) for x in a.ks.split(",")]:
            def start():
                env.reset()
                env.run_greedy(10)                     # positions past the opening
            start()
            f_ms, f_all = _time(lambda: env.step_search(top_k=k, margin=mg), a.steps, a.warmup, a.regions)
            f_info = env.search_info()
            start()
            ms, all_ms = _time(lambda: env.step_search(top_k=k, margin=mg, plies=3, **deep), a.steps, a.warmup, a.regions)
            info = env.search3_info()
            # the choices of both steps on one set of positions and dice (nothing flips or restarts: the boards are the choices)
            start()
            env.roll()
            st, tu, dice = env.states().clone(), env.turns().clone(), env.dice().clone()
            env.step_search(top_k=k, roll=False, auto_reset=False, no_flip=True, margin=mg)
            two = env.states().clone()
            env.set_states(st, tu)
            env.set_dice(dice)
            env.step_search(top_k=k, roll=False, auto_reset=False, no_flip=True, margin=mg, plies=3, **deep)
            differs = float((env.states() != two).any(1).float().mean())
            r = {"n": n, "plies": 3, "top_k": k, "margin": mg, **deep, "ms_per_search_step": round(ms, 4),
                 "filtered_2ply_ms_per_search_step": round(f_ms, 4), "times_the_2ply_step": round(ms / f_ms, 2),
                 "lanes_with_a_move": info[0], "lanes_searched_2_plies": info[1], "lanes_searched_3_plies": info[2],
                 "deep_candidates": info[3], "mid_lanes_last_step": info[4], "level3_roots_last_step": info[5],
                 "ns_per_level3_root": round(ms * 1e6 / max(info[5], 1), 3), "virtual_roots_2ply_last_step": f_info[3],
                 "ns_per_2ply_root": round(f_ms * 1e6 / max(f_info[3], 1), 3), "choice_differs_from_2ply_share": round(differs, 5),
                 "regions_ms": [round(x, 4) for x in all_ms], "filtered_2ply_regions_ms": [round(x, 4) for x in f_all]}
            print(json.dumps(r), flush=True)
            out.append(r)
        env.close()
    print(json.dumps({"search_bench_3_plies": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--ks", default="4,8,0")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--margin", default="", help="comma-separated margins of the filtered step (none: the unfiltered step only)")
    ap.add_argument("--log", action="store_true", help="the cost of the search log's pass instead (see above)")
    ap.add_argument("--plies", type=int, default=2, choices=(2, 3), help="3: the 3-ply step against the filtered 2-ply step (see above)")
    ap.add_argument("--deep-k", type=int, default=2)
    ap.add_argument("--deep-margin", type=float, default=0.04)
    ap.add_argument("--reply-k", type=int, default=2)
    ap.add_argument("--reply-margin", type=float, default=0.04)
    a = ap.parse_args()
    if a.plies == 3:
        return three_plies(a)
    if a.log:
        return log_cost(a)
    import backgammon_env as bg
    w = np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)
    out = []
    for n in [int(x) for x in a.sizes.split(",")]:
        env = bg.VecGame(n, seed=1)
        env.load_weights(w)
        g_ms, _ = _time(lambda: env.step_greedy(), max(a.steps, 20), a.warmup, a.regions)
        for k in [int(x) for x in a.ks.split(",")]:
            env.reset()
            env.run_greedy(10)                         # positions past the opening
            ms, all_ms = _time(lambda: env.step_search(top_k=k), a.steps, a.warmup, a.regions)
            _, _, _, kept = env.search_candidates()
            roots = int(kept.sum()) * 21
            r = {"n": n, "top_k": k, "ms_per_search_step": round(ms, 4), "searched_moves_per_s": round(n / ms * 1e3),
                 "virtual_roots_last_step": roots, "virtual_roots_per_s": round(roots / ms * 1e3),
                 "greedy_ms_per_step": round(g_ms, 4), "greedy_env_steps_per_s": round(n / g_ms * 1e3),
                 "regions_ms": [round(x, 4) for x in all_ms]}
            print(json.dumps(r), flush=True)
            out.append(r)
            for mg in [float(x) for x in a.margin.split(",") if x]:
                env.reset()
                env.run_greedy(10)
                f_ms, f_all = _time(lambda: env.step_search(top_k=k, margin=mg), a.steps, a.warmup, a.regions)
                info = env.search_info()
                # the choices of both steps on one set of positions and dice (nothing flips or restarts: the boards are the choices)
                env.reset()
                env.run_greedy(10)
                env.roll()
                st, tu, dice = env.states().clone(), env.turns().clone(), env.dice().clone()
                env.step_search(top_k=k, roll=False, auto_reset=False, no_flip=True)
                plain = env.states().clone()
                env.set_states(st, tu)
                env.set_dice(dice)
                env.step_search(top_k=k, roll=False, auto_reset=False, no_flip=True, margin=mg)
                differs = float((env.states() != plain).any(1).float().mean())
                r = {"n": n, "top_k": k, "margin": mg, "ms_per_search_step": round(f_ms, 4), "unfiltered_ms_per_search_step": round(ms, 4),
                     "speedup": round(ms / f_ms, 2), "lanes_with_a_move": info[0], "lanes_searched": info[1], "kept_candidates": info[2],
                     "virtual_roots_last_step": info[3], "choice_differs_share": round(differs, 5),
                     "regions_ms": [round(x, 4) for x in f_all]}
                print(json.dumps(r), flush=True)
                out.append(r)
        env.close()
    print(json.dumps({"search_bench": out}))


if __name__ == "__main__":
    main()
