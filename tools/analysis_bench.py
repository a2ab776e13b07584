"""Throughput of the move analysis (bgamd_env_analyze_moves + bgamd_env_analysis_read): analysed decisions/s and virtual roots/s at
`--lanes` lanes and `--top-k`, set against the search step at top_k + 1 (the same bound on the virtual roots, plus its apply launch) timed
the way tools/search_bench.py times it, the two alternating `--runs` times in this one process.  The positions are mid-game ones as
tools/search_bench.py makes them (ten greedy turns past the opening); the played moves are the greedy step's.  Every figure is the median of
several timed regions after a warm-up (HIP events around `--steps` back-to-back calls, no host wait inside a region).  One JSON line per
run, then a summary line with the medians and the spread (max - min over the runs)."""
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

from search_bench import _time  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--top-k", type=int, default=4)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    import backgammon_env as bg
    from backgammon_env import _capi
    w = np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)
    n, k = a.lanes, a.top_k
    player, judge = bg.VecGame(n, seed=1), bg.VecGame(n, seed=1)
    for e in (player, judge):
        e.load_weights(w)
    player.run_greedy(10)
    pre, mover = player.states(), player.turns()
    player.step_greedy(auto_reset=False)
    played = player.states()
    judge.set_states(pre, mover)
    judge.set_dice(player.dice())
    res = judge.analyze_moves(played, top_k=k)
    st, distinct, rank1 = res["status"], res["distinct"], res["rank1"]
    kept = torch.where(st == 0, distinct.clamp(max=k) + (rank1 >= k).int(), torch.where(st == 3, distinct.clamp(max=k), 0))
    decisions, roots = int((st == 0).sum()), int(kept.sum()) * 21
    out = {f: judge._buf((n,), dt) for f, dt in judge.ANALYSIS_FIELDS}
    best, summ = judge._buf((n, 28), torch.int32), judge._buf((12,), torch.float64)
    ptrs = [bg._ptr(out[f]) for f, _ in judge.ANALYSIS_FIELDS] + [bg._ptr(best), bg._ptr(summ)]

    def analyse():
        _capi.check(judge._lib.bgamd_env_analyze_moves(judge._h, 0, k, bg._ptr(played), bg._stream()), "analyze_moves")
        _capi.check(judge._lib.bgamd_env_analysis_read(judge._h, *ptrs, bg._stream()), "analysis_read")
    runs = []
    for _ in range(a.runs):
        a_ms, a_all = _time(analyse, a.steps, a.warmup, a.regions)
        player.reset()
        player.run_greedy(10)
        s_ms, s_all = _time(lambda: player.step_search(top_k=k + 1), a.steps, a.warmup, a.regions)
        s_roots = int(player.search_candidates()[3].sum()) * 21
        r = {"n": n, "top_k": k, "analysis_ms": round(a_ms, 4), "decisions": decisions, "decisions_per_s": round(decisions / a_ms * 1e3),
             "virtual_roots": roots, "virtual_roots_per_s": round(roots / a_ms * 1e3), "analysis_regions_ms": [round(x, 4) for x in a_all],
             "search_top_k": k + 1, "search_ms": round(s_ms, 4), "search_virtual_roots_last_step": s_roots,
             "search_regions_ms": [round(x, 4) for x in s_all]}
        print(json.dumps(r), flush=True)
        runs.append(r)
    am, sm = [r["analysis_ms"] for r in runs], [r["search_ms"] for r in runs]
    print(json.dumps({"analysis_bench": {"n": n, "top_k": k, "analysis_ms_median": statistics.median(am), "analysis_ms_spread": round(max(am) - min(am), 4),
                                         "decisions_per_s": round(decisions / statistics.median(am) * 1e3),
                                         "virtual_roots_per_s": round(roots / statistics.median(am) * 1e3),
                                         "search_ms_median": statistics.median(sm), "search_ms_spread": round(max(sm) - min(sm), 4)}}))
    player.close()
    judge.close()


if __name__ == "__main__":
    main()
