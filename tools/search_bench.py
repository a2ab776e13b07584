"""Throughput of the 2-ply expectimax step (bgamd_env_step_search): searched moves/s and virtual roots/s at several env sizes and
top_k, set against the greedy step's env steps/s measured in the same run.  Every figure is the median of several timed regions
after a warm-up (HIP events around `--steps` back-to-back steps).  One JSON line per configuration, then a summary line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--ks", default="4,8,0")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--regions", type=int, default=5)
    a = ap.parse_args()
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
        env.close()
    print(json.dumps({"search_bench": out}))


if __name__ == "__main__":
    main()
