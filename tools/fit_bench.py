"""Rows/s of the supervised step (DeviceTDLambdaLearner.fit_step, bgamd_td_fit_step) at 4 096 and 65 536 rows of a greedy self-play log,
set against the only route there was before it: the same rows as one-turn games of a T = 1 log, replayed lock-step by TD(λ)
(bgamd_td_begin + bgamd_td_step(t = 0), update applied) with the games' results as binary targets.  The two routes alternate inside one
run: per size and repeat, one region of fit steps and one of TD steps, each HIP-event-timed over at least --seconds of warmed work.
Prints a table (median, min and max over the repeats), the algorithmic flop and bytes per row computed from the shapes, and whether at
65 536 rows the fit step is not slower than the TD route beyond the spread of the repeats.

    python tools/fit_bench.py > profiles/fit_bench.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "backgammon-engine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_IN, N_HID, N_PARAMS, TD_LD = 198, 128, 25601, 25664


def _region(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _iters(fn, seconds):
    """warm-up, then the number of calls that fill `seconds`"""
    fn()
    torch.cuda.synchronize()
    ms = _region(fn, 4)
    return max(4, int(np.ceil(seconds * 1e3 / max(ms, 1e-3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--seconds", type=float, default=1.0, help="warmed work per timed region")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lanes", type=int, default=4096, help="lanes of the self-play round the rows come from")
    a = ap.parse_args()
    import backgammon_env as bg
    from backgammon_env import _capi
    from backgammon_env.learner import DeviceTDLambdaLearner, play_round
    w = np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)
    env = bg.VecGame(a.lanes, seed=1)
    env.load_weights(w)
    rows, lengths, p1_won = play_round(env, max_plies=400)
    inside = torch.arange(rows.shape[0], device=rows.device)[:, None] < lengths[None, :]
    pool = rows[inside].contiguous()
    won = p1_won[None, :].expand(rows.shape[0], -1)[inside].contiguous()
    print("supervised step against the T = 1 TD(lambda) route, alternating in one run (source digest %s)" % _capi.source_hash())
    print("rows: the first n of the %d turns of a greedy round of %d games; targets: the games' results (0 / 1)" % (pool.shape[0], a.lanes))
    print("each region: >= %.1f s of warmed calls between two HIP events; %d repeats per route and size, the routes alternating" % (a.seconds, a.repeats))
    print()
    print("%8s  %-9s %12s %12s %12s %14s" % ("rows", "route", "median ms", "min ms", "max ms", "rows/s (median)"))
    verdict = None
    for n in a.sizes:
        if n > pool.shape[0]:
            raise SystemExit("the round logged only %d turns: raise --lanes" % pool.shape[0])
        r = pool[:n].contiguous()
        y = won[:n].to(torch.float32).contiguous()
        alpha = 0.1 * 24.0 / n
        L = DeviceTDLambdaLearner(w, max_games=n, alpha=0.1)
        C, lib, chk = L._C, L._lib, _capi.check
        log = r.reshape(1, n, 8)
        order = torch.arange(n, dtype=torch.int32, device=L.device)
        ones = torch.ones(n, dtype=torch.int32, device=L.device)
        won8 = won[:n].to(torch.uint8).contiguous()

        def fit():
            chk(lib.bgamd_td_fit_step(L._h, L._p(r), L._p(y), n, alpha, None, L._s()), "td_fit_step")

        def td():
            chk(lib.bgamd_td_begin(L._h, L._p(log), 1, n, L._p(order), n, L._p(ones), L._p(won8), L._s()), "td_begin")
            chk(lib.bgamd_td_step(L._h, 0, n, alpha, 0.7, None, L._s()), "td_step")

        k_fit, k_td = _iters(fit, a.seconds), _iters(td, a.seconds)
        ms = {"fit_step": [], "td T=1": []}
        for _ in range(a.repeats):
            L.set_weights(w)
            ms["fit_step"].append(_region(fit, k_fit))
            L.set_weights(w)
            ms["td T=1"].append(_region(td, k_td))
        for route, v in ms.items():
            print("%8d  %-9s %12.4f %12.4f %12.4f %14.0f" % (n, route, statistics.median(v), min(v), max(v), n / statistics.median(v) * 1e3))
        f, t = ms["fit_step"], ms["td T=1"]
        spread = (max(f) - min(f)) + (max(t) - min(t))
        print("%8d  fit_step / td T=1 = %.3f of the time (spread of the repeats, both routes: %.4f ms; %d and %d calls per region)" % (
            n, statistics.median(f) / statistics.median(t), spread, k_fit, k_td))
        if n == 65536:
            verdict = statistics.median(f) <= statistics.median(t) + spread
        L.fit_stats()
        del L
    print()
    print("algorithmic work per row, from the shapes (198 inputs, 128 hidden units, 25 601 parameters):")
    fwd = 2 * N_IN * N_HID + 2 * N_HID
    grad = 2 * N_IN * N_HID + 2 * 2 * N_HID + 2
    print("  fit_step : %d flop forward + %d flop gradient sums = %d flop; %d B read (32 B row + 4 B target); written per launch,"
          " not per row: 256 x %d B of partial sums + the %d B update" % (fwd, grad, fwd + grad, 36, TD_LD * 4, N_PARAMS * 4))
    cols = 35
    tr = (cols * N_HID + 2 * N_HID + 1) * 4
    print("  td T=1   : 2 forward passes (s_t and the unused s_t+1 slot) = %d flop + %d flop of trace and sum; %d B read (row x 2 + length,"
          " winner, order) ; a factor row of %d B written and read; ~%d active columns x 512 B + %d B of b1 | W2 | b2 trace written"
          " = ~%d B of trace traffic" % (2 * fwd, 2 * (cols * N_HID + 2 * N_HID + 1) * 2, 64 + 9, 272 * 4, cols, (2 * N_HID + 1) * 4, tr))
    print("  shares of peak: not measured")
    if verdict is not None:
        print()
        print("condition (65 536 rows: fit_step not slower than the TD route beyond the spread): %s" % ("met" if verdict else "NOT met"))


if __name__ == "__main__":
    main()
