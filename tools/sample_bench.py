"""Cost of the temperature-sampled step (bgamd_env_run_sampled) beside the greedy step and the epsilon-exploring step of the SAME run:
ms per env step at --lanes lanes (default 65 536) for greedy, epsilon = 0.05 and sampled at T = 0.02 / 0.05 / 0.1, with the share of
lanes that left the arg-max in the last sampled step (bgamd_env_sample_info).  Every figure is the median of --regions timed regions of
--steps back-to-back steps in one run_* call (HIP events, the last one synchronised), after a warm-up of the same call; the variants
are measured in turn, --rounds times over, so that a drift of the machine shows as a spread between rounds and not as a difference
between variants.  One JSON line per variant and round, then a summary line with the medians and each variant's min / max."""
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
        fn(steps)
    torch.cuda.synchronize()
    ms = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(steps)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    return statistics.median(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200, help="env steps per timed region (one run_* call)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epsilon", type=float, default=0.05)
    ap.add_argument("--temperatures", default="0.02,0.05,0.1")
    a = ap.parse_args()
    import backgammon_env as bg
    if not torch.cuda.is_available():
        sys.exit("sample_bench needs the GPU: a time taken anywhere else says nothing")
    w = np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)
    env = bg.VecGame(a.lanes, seed=1)
    env.load_weights(w)
    variants = [("greedy", lambda k: env.run_greedy(k)), ("epsilon %g" % a.epsilon, lambda k: env.run_greedy(k, epsilon=a.epsilon))]
    for T in [float(x) for x in a.temperatures.split(",") if x]:
        variants.append(("sampled T %g" % T, lambda k, T=T: env.run_sampled(k, T)))
    seen = {name: [] for name, _ in variants}
    left = {}
    for rnd in range(a.rounds):
        for name, fn in variants:
            ms, all_ms = _time(fn, a.steps, a.warmup, a.regions)
            r = {"variant": name, "round": rnd, "lanes": a.lanes, "ms_per_step": round(ms, 5), "regions_ms": [round(x, 5) for x in all_ms]}
            if name.startswith("sampled"):
                env.run_sampled(1, float(name.split()[-1]))
                moved, off = env.sample_info()
                left[name] = r["left_argmax_share"] = round(off / max(moved, 1), 5)
            seen[name].append(ms)
            print(json.dumps(r), flush=True)
    base = statistics.median(seen["greedy"])
    summary = {name: {"ms_per_step": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5),
                      "over_greedy_us": round((statistics.median(v) - base) * 1e3, 2), **({"left_argmax_share": left[name]} if name in left else {})}
               for name, v in seen.items()}
    print(json.dumps({"sample_bench": summary, "lanes": a.lanes, "steps": a.steps, "regions": a.regions, "rounds": a.rounds,
                      "source_hash": bg._capi.source_hash()}))
    env.close()


if __name__ == "__main__":
    main()
