"""Throughput of the Monte Carlo rollout (bgamd_env_rollout) at 65 536 lanes: full rollouts (64 mid-game positions x 16 384 rotated
trials, played to the end) and truncated ones (the same positions at M = 7 and M = 0, as a pair), set against the greedy step's env
steps/s measured in the same run.  One JSON line per configuration: ms per call (median of --regions timed calls after a warm-up call),
trials/s, trial-turns/s (turns of all trials / time), their ratio to the greedy step, and the idle share (lane-steps on lanes without a
live trial / all lane-steps, from bgamd_env_rollout_info).

--vr: luck-adjusted rollouts (BGAMD_ROLLOUT_VR) instead, full (M = 0) and truncated (M = 7), --vr-trials rotated trials per position.  For
each: the plain call and the VR call of the same trials, ms per call, the VR pass's virtual roots/s (21 per trial-turn over the time the
VR call adds), the per-position variance ratio (stderr / vr_stderr)^2 (median, min, max, pooled) and effective trials/s (trials/s x the
median ratio; 1 for the plain call).

--cube (with --vr): beside every VR call the same call with the doubling cube on (bgamd_env_rollout_cube, the header's default rule, the
cube results read inside the timed region): ms per call with and without the cube, their ratio, and the share of lane-turns played
after the trial's drop (bgamd_env_rollout_cube_info) -- what not freeing a lane at a drop costs.

--match (with --vr --cube): beside every cube call the same call under a match (bgamd_env_rollout_match: 7-away / 7-away on
MatchTable.janowski(7), the default window share, the match results read inside the timed region): ms per call, its ratio to the cube
call, the match's counts, and match_setting_ms: the setting and its clearing alone, which every rollout(match=) call pays.

--outcomes: the same run with the games read in points after every call (bgamd_env_rollout_outcomes_read, inside the timed region):
every record also carries the six shares (PLAYER1 single game / gammon / backgammon, PLAYER2 the same) over the finished trials of all
positions and the mean equity of the positions in points.

--plies 2 [--top-k K --margin M]: the trials are played by the filtered 2-ply search (bgamd_env_rollout_policy) instead of the greedy
step; a 2-ply turn costs ~100 greedy steps, so give fewer --trials.  With --vr: the luck pass beside 2-ply turns.

--groups D,K: D decisions (mid-game positions with rolled dice whose 2-ply search keeps K candidates) of K candidates each, every
candidate rolled out with --group-trials rotated trials, twice on the same positions, seed and trials: as ONE grouped call
(bgamd_env_rollout_grouped, the decision as dice group) and as D x K single-position calls at position_offset = decision, which is what
analysis.rollout_moves does.  Both in ms (median of --regions runs after a warm-up run), whether the two agree bit for bit, and the
median over the non-best candidates of unpaired sqrt(se_a^2 + se_b^2) / paired diff_stderr against the decision's best candidate."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "backgammon-engine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


POLICY = {}                                            # --plies 2: the rollout policy every call is given


def _greedy_ms(env, steps, regions):
    env.run_greedy(steps)
    torch.cuda.synchronize()
    ms = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        env.run_greedy(steps)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    return statistics.median(ms)


def _positions(bg, w, n, seed):
    """n mid-game positions: greedy play from the start position, lane k stopped after 10 + k turns."""
    e = bg.VecGame(max(n, 64), seed=seed)
    e.load_weights(w)
    e.run_greedy(10)
    st, tu = [], []
    for k in range(n):
        e.step_greedy()
        st.append(e.states()[k].cpu().numpy()); tu.append(int(e.turns()[k]))
    e.close()
    return np.array(st, np.int32), np.array(tu, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--positions", type=int, default=64)
    ap.add_argument("--trials", type=int, default=16384)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--vr", action="store_true", help="luck-adjusted rollouts against plain ones")
    ap.add_argument("--vr-trials", type=int, default=2592)
    ap.add_argument("--cube", action="store_true", help="--vr: also the same VR calls with the doubling cube on")
    ap.add_argument("--match", action="store_true", help="--vr --cube: also the same cube calls under a match score")
    ap.add_argument("--outcomes", action="store_true", help="also read gammons / backgammons and the equity in points")
    ap.add_argument("--plies", type=int, default=1, choices=(1, 2), help="who plays the trials: 1 = the greedy step, 2 = the filtered 2-ply search")
    ap.add_argument("--top-k", type=int, default=5, help="--plies 2: the search's top_k")
    ap.add_argument("--margin", type=float, default=0.04, help="--plies 2: the search's margin")
    ap.add_argument("--groups", default=None, metavar="D,K", help="D decisions of K candidates: one grouped call against D x K single calls")
    ap.add_argument("--group-trials", type=int, default=1296)
    ap.add_argument("--max-plies", type=int, default=0, help="--groups: the turn limit of the trials (0 = to the end)")
    ap.add_argument("--configs", default="full,truncated,pair", help="which of full (M = 0), truncated (M = 7), pair (M = 0 again) to run")
    a = ap.parse_args()
    global POLICY
    POLICY = dict(plies=2, top_k=a.top_k, margin=a.margin) if a.plies == 2 else {}
    if a.cube and not a.vr:
        ap.error("--cube rides on the luck pass: give it with --vr")
    if a.match and not a.cube:
        ap.error("--match sets the cube's thresholds: give it with --vr --cube")
    if a.vr and a.outcomes:
        ap.error("--outcomes reads the plain run's games; it is not combined with --vr")
    import backgammon_env as bg
    w = np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)
    if a.groups:
        _groups(bg, w, a)
        return
    st, tu = _positions(bg, w, a.positions, 1)
    env = bg.VecGame(a.lanes, seed=1)
    env.load_weights(w)
    g_ms = _greedy_ms(env, 20, 5)
    greedy_sps = a.lanes / g_ms * 1e3
    if a.vr:
        _vr(env, st, tu, a, greedy_sps)
        env.close()
        return
    out = []
    configs = {"full": ("full", 0), "truncated": ("truncated", 7), "pair": ("truncated", 0)}
    for name, M in [configs[c] for c in a.configs.split(",")]:
        env.rollout(st, tu, a.trials, max_plies=M, rotate=True, seed=5, lanes=a.lanes, **POLICY)       # warm-up (scratch env, buffers)
        ms = []
        for _ in range(a.regions):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = env.rollout(st, tu, a.trials, max_plies=M, rotate=True, seed=5, lanes=a.lanes, outcomes=a.outcomes, **POLICY)
            if a.outcomes:
                torch.cuda.synchronize()                           # (the read is stream-ordered after the call)
            ms.append((time.perf_counter() - t0) * 1e3)            # (the call synchronises)
        info = env.rollout_info()
        m = statistics.median(ms)
        n_trials = a.positions * a.trials
        turns = int(r["turns"].sum())
        idle = 1.0 - info[2] / float(info[0] * info[1])
        rec = {"config": name, "max_plies": M, "plies": a.plies, "lanes": info[0], "positions": a.positions, "trials": a.trials, "ms": round(m, 2),
               "trials_per_s": round(n_trials / m * 1e3), "trial_turns_per_s": round(turns / m * 1e3),
               "greedy_env_steps_per_s": round(greedy_sps), "ratio_to_greedy": round(turns / m * 1e3 / greedy_sps, 3),
               "idle_share": round(idle, 4), "env_steps": info[1], "turns_per_run": info[3], "mean_turns": round(turns / n_trials, 2),
               "truncated": int(r["truncated"].sum()), "regions_ms": [round(x, 2) for x in ms]}
        if a.outcomes:
            c = r["counts"].sum(0).cpu().numpy().astype(np.float64)
            rec["outcome_shares"] = dict(zip(("p1_single", "p1_gammon", "p1_backgammon", "p2_single", "p2_gammon", "p2_backgammon"),
                                             [round(float(x), 5) for x in c / max(c.sum(), 1.0)]))
            rec["equity"] = round(float(r["equity"].mean()), 5)
            rec["equity_stderr_median"] = round(float(r["equity_stderr"].median()), 5)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    env.close()
    print(json.dumps({"rollout_bench": out}))


def _groups(bg, w, a):
    D, K = (int(x) for x in a.groups.split(","))
    # decisions: mid-game positions with rolled dice; the first D whose search keeps K candidates
    n = 4 * D + 16
    st, tu = _positions(bg, w, n, 1)
    dec = bg.VecGame(n, seed=2)
    dec.load_weights(w)
    dec.set_states(st, tu)
    dec.set_dice(np.random.RandomState(3).randint(1, 7, (n, 2)).astype(np.int32))
    dec.step_search(top_k=K, roll=False, auto_reset=False, no_flip=True)
    cst, _, _, kept = (x.cpu().numpy() for x in dec.search_candidates())
    dec.close()
    pick = np.flatnonzero(kept == K)[:D]
    if len(pick) < D:
        raise SystemExit("only %d of %d decisions keep %d candidates" % (len(pick), n, K))
    after = cst[pick].reshape(D * K, 28)
    turn = np.repeat(1 - tu[pick], K).astype(np.int32)
    group = np.repeat(np.arange(D), K)
    T, M = a.group_trials, a.max_plies
    env = bg.VecGame(64, seed=1)
    env.load_weights(w)
    kw = dict(max_plies=M, rotate=True, seed=5, **POLICY)

    def grouped():
        r = env.rollout(after, turn, T, groups=group, **kw)
        best = np.empty(D * K, np.int64)
        m = r["mean"].cpu().numpy().reshape(D, K)
        for d in range(D):                                 # the decision's best for its mover, as analysis.rollout_decisions ranks
            best[d * K:(d + 1) * K] = d * K + (np.argmax(m[d]) if tu[pick[d]] == 0 else np.argmin(m[d]))
        dm, ds = env.rollout_paired(best, "value")
        torch.cuda.synchronize()
        return r, best, dm.cpu().numpy(), ds.cpu().numpy()

    def singles():
        out = [env.rollout(after[q:q + 1], turn[q:q + 1], T, position_offset=int(group[q]), **kw) for q in range(D * K)]
        torch.cuda.synchronize()
        return out

    def timed(fn):
        fn()                                               # warm-up (the trial env of this lane count, buffers)
        ms = []
        for _ in range(a.regions):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), ms, res

    g_ms, g_all, (r, best, dm, ds) = timed(grouped)
    g_info = env.rollout_info()
    s_ms, s_all, one = timed(singles)
    s_info = env.rollout_info()
    mean, se = r["mean"].cpu().numpy(), r["stderr"].cpu().numpy()
    same = all(float(one[q]["mean"][0]) == mean[q] and float(one[q]["stderr"][0]) == se[q] for q in range(D * K))
    rival = np.flatnonzero((best != np.arange(D * K)) & (ds > 0))
    ratio = np.sqrt(se[rival] ** 2 + se[best[rival]] ** 2) / ds[rival]
    rec = {"decisions": D, "candidates": K, "positions": D * K, "trials": T, "max_plies": M, "plies": a.plies,
           "grouped_ms": round(g_ms, 2), "singles_ms": round(s_ms, 2), "speedup": round(s_ms / g_ms, 2),
           "grouped_lanes": g_info[0], "grouped_idle_share": round(1.0 - g_info[2] / float(g_info[0] * g_info[1]), 4),
           "single_lanes": s_info[0], "single_idle_share_last": round(1.0 - s_info[2] / float(s_info[0] * s_info[1]), 4),
           "bit_identical": bool(same), "rivals": int(len(rival)),
           "unpaired_over_paired_stderr_median": round(float(np.median(ratio)), 3),
           "unpaired_over_paired_stderr_min": round(float(ratio.min()), 3), "unpaired_over_paired_stderr_max": round(float(ratio.max()), 3),
           "jsd_median": round(float(np.median(np.abs(dm[rival]) / ds[rival])), 3),
           "grouped_regions_ms": [round(x, 2) for x in g_all], "singles_regions_ms": [round(x, 2) for x in s_all]}
    env.close()
    print(json.dumps({"rollout_groups_bench": rec}))


def _timed(env, st, tu, trials, M, lanes, regions, vr, cube=None, match=None):
    env.rollout(st, tu, trials, max_plies=M, rotate=True, seed=5, lanes=lanes, variance_reduction=vr, cube=cube, match=match, **POLICY)      # warm-up
    ms = []
    for _ in range(regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = env.rollout(st, tu, trials, max_plies=M, rotate=True, seed=5, lanes=lanes, variance_reduction=vr, cube=cube, match=match, **POLICY)
        if cube is not None:
            torch.cuda.synchronize()                               # (the cube read is stream-ordered after the call)
        ms.append((time.perf_counter() - t0) * 1e3)                # (the call synchronises; vr_read is stream-ordered after it)
    torch.cuda.synchronize()
    return statistics.median(ms), r, ms


def _vr(env, st, tu, a, greedy_sps):
    out = []
    for name, M in [c for c in (("full", 0), ("truncated", 7)) if c[0] in a.configs.split(",")]:
        ms_p, rp, _ = _timed(env, st, tu, a.vr_trials, M, a.lanes, a.regions, False)
        ms_v, rv, regions = _timed(env, st, tu, a.vr_trials, M, a.lanes, a.regions, True)
        info = env.rollout_info()
        se, vse = rv["stderr"].cpu().numpy(), rv["vr_stderr"].cpu().numpy()
        live = (se > 0) & (vse > 0)
        ratio = se[live] ** 2 / vse[live] ** 2
        med = float(np.median(ratio))
        n_trials = a.positions * a.vr_trials
        turns = int(rp["turns"].sum())
        roots = 21 * turns
        rec = {"config": name, "max_plies": M, "plies": a.plies, "lanes": info[0], "positions": a.positions, "trials": a.vr_trials,
               "plain_ms": round(ms_p, 2), "vr_ms": round(ms_v, 2), "cost_ratio": round(ms_v / ms_p, 2),
               "vr_virtual_roots_per_s": round(roots / (ms_v - ms_p) * 1e3),
               "greedy_env_steps_per_s": round(greedy_sps), "vr_roots_to_greedy": round(roots / (ms_v - ms_p) * 1e3 / greedy_sps, 3),
               "variance_ratio_median": round(med, 3), "variance_ratio_min": round(float(ratio.min()), 3),
               "variance_ratio_max": round(float(ratio.max()), 3), "variance_ratio_pooled": round(float((se[live] ** 2).sum() /
                                                                                                     (vse[live] ** 2).sum()), 3),
               "plain_effective_trials_per_s": round(n_trials / ms_p * 1e3),
               "vr_effective_trials_per_s": round(n_trials / ms_v * 1e3 * med),
               "mean_turns": round(turns / n_trials, 2), "vr_regions_ms": [round(x, 2) for x in regions]}
        if a.cube:
            import backgammon_env as bg
            ms_c, rc, cregions = _timed(env, st, tu, a.vr_trials, M, a.lanes, a.regions, True, cube=bg.Cube())
            played, after = env.rollout_cube_info()
            cc = rc["cube_counts"].sum(0).cpu().numpy()
            rec.update({"cube_ms": round(ms_c, 2), "cube_over_vr": round(ms_c / ms_v, 4), "cube_regions_ms": [round(x, 2) for x in cregions],
                        "cube_lane_turns": played, "cube_lane_turns_after_drop": after,
                        "cube_share_after_drop": round(after / max(played, 1), 4),
                        "cube_dropped_share": round(float(cc[0] + cc[1]) / n_trials, 4), "cube_turns_per_trial": round(float(cc[2]) / n_trials, 4),
                        "cubeful_mean": round(float(rc["cubeful"].mean()), 5), "cubeless_same_trials_unchanged": bool(
                            torch.equal(rc["mean"], rv["mean"]) and torch.equal(rc["vr_mean"], rv["vr_mean"]))})
        if a.match:
            ms_m, rm, mregions = _timed(env, st, tu, a.vr_trials, M, a.lanes, a.regions, True, cube=bg.Cube(),
                                        match=bg.Match(bg.MatchTable.janowski(7), 7, 7))
            mc = rm["match_counts"].sum(0).cpu().numpy()
            # what rollout(match=) pays per call outside the trials: the setting (a device synchronise, the threshold table built on the
            # host, one synchronous copy) and its clearing -- inside match_ms above, timed here on its own
            a1 = torch.full((a.positions,), 7, dtype=torch.int32, device=env.device)
            zero, table, sets = torch.zeros_like(a1), bg.MatchTable.janowski(7), []
            for _ in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                env._set_match(table, 0.5, a1, a1, zero)
                env._lib.bgamd_env_rollout_match(env._h, 0, 0, None, None, 0.0, None, None, None)
                sets.append((time.perf_counter() - t0) * 1e3)
            rec["match_setting_ms"] = round(statistics.median(sets), 3)
            rec.update({"match_ms": round(ms_m, 2), "match_over_cube": round(ms_m / ms_c, 4), "match_regions_ms": [round(x, 2) for x in mregions],
                        "match_ended_share": round(float(mc[0] + mc[1]) / n_trials, 4), "match_dead_cube_share": round(float(mc[2]) / n_trials, 4),
                        "mwc_mean": round(float(rm["mwc"].mean()), 5), "cubeless_same_trials_unchanged_by_match": bool(
                            torch.equal(rm["mean"], rv["mean"]) and torch.equal(rm["vr_mean"], rv["vr_mean"]))})
        print(json.dumps(rec), flush=True)
        out.append(rec)
    print(json.dumps({"rollout_vr_bench": out}))


if __name__ == "__main__":
    main()
