"""The history test's program as data: no GPU, no torch.

The rule under test (include/bgamd.h, "history rule"): the outputs of a call are a function of its arguments and of the env's documented
state, never of which calls came before, at which sizes, or whether they succeeded.  tests/test_gpu_history.py runs every PROBE on an env
created for it and again on an env that has been through all of SOIL, and compares bit for bit; tests/test_history_cases_cpu.py states,
without a device, the conditions that keep that comparison from passing vacuously.

An entry is a dict: name, op (what tests/test_gpu_history.py's runner does), kw (its arguments, plain data), reads (the read calls made
after it).  families(entry) -> {state family: size parameter}: the lanes an internal env is asked for, the rows a grown buffer is asked
for -- computed from the arguments with the restatement of search_lanes and of the rollout plan in tests/rollout_plan_ref.py.
Boards and positions are named by selectors that lanes() and positions() below resolve."""
import functools

import numpy as np

import outcome_ref as OR
import rollout_cases as RC
import rollout_plan_ref as PL
import search_lanes as L

N = 65                                                  # lanes of the envs; the second probe set has 1
SEED, OTHER_SEED = 20240603, 977                        # the constructor's seed; what SOIL reseeds to in between
RO_SEED, RO_OTHER_SEED = 4242, 99                       # the rollouts' seed argument: the probes', SOIL's
PROBE_NETS, SOIL_NETS = ("ckpt", "xavier"), ("normal", "ckpt_x4")        # tests/nets.py tables of slot 0, slot 1
FAMILIES = ("scratch", "mid", "rscratch", "search_buffers", "rollout_buffers", "arenas", "settings", "logs", "weights", "flags")
SIZED = ("scratch", "mid", "rscratch", "search_buffers", "rollout_buffers", "arenas")    # the families that have a size
# the issue's sizes: lanes of the internal envs, positions x trials and the horizon of a rollout (one probe is played out)
BUDGET = dict(scratch=16384, mid=4096, positions=8, trials=36, max_plies=6)
OK, E_INVALID, E_STATE, E_NOWEIGHTS = 0, -1, -5, -6
ROLLS = 21


# ---- boards -----------------------------------------------------------------------------------------------------------------------------

OVER = OR._state(p1=[(24, 5), (23, 5), (12, 5)], off2=15)              # a game that is over: such a lane takes no part in a step
DEAD_A = (7, 21, 35, 49, 63)                                            # lanes of set A that hold OVER


@functools.lru_cache(maxsize=None)
def lanes(sel):
    """-> (boards int32 [n, 28], mover int32 [n], dice int32 [n, 2]) of a selector:
    A   the probes' 65 lanes: the first 60 fixture boards whose dice are no doubles, OVER on the five lanes DEAD_A
    B   SOIL's 65 lanes: fixture boards 700 .. 764 as they come, doubles included, every lane live
    A3  the 3-ply probe's: A with OVER on every lane but 0, 8, ..., 64 (nine live lanes)
    B3  SOIL's 3-ply step's: B with OVER on every lane but 5, 10, ..., 60 (twelve live lanes)
    A1 / B1  one lane: A's lane 8 (17 afterstates) / the first fixture board from 700 on whose dice are doubles"""
    st, tu, dice = L.g10()
    nd = np.nonzero(dice[:, 0] != dice[:, 1])[0]
    if sel in ("A", "A3"):
        idx = nd[:N].copy()
        s, t, d = st[idx].copy(), tu[idx].copy(), dice[idx].copy()
        dead = DEAD_A if sel == "A" else [g for g in range(N) if g % 8]
        s[list(dead)] = OVER
    elif sel in ("B", "B3"):
        s, t, d = st[700:700 + N].copy(), tu[700:700 + N].copy(), dice[700:700 + N].copy()
        if sel == "B3":
            s[[g for g in range(N) if g % 5 or g == 0]] = OVER
    elif sel == "A1":
        s, t, d = (x[8:9].copy() for x in lanes("A"))
    elif sel == "B1":
        k = 700 + int(np.nonzero(dice[700:, 0] == dice[700:, 1])[0][0])
        s, t, d = st[k:k + 1].copy(), tu[k:k + 1].copy(), dice[k:k + 1].copy()
    else:
        raise KeyError(sel)
    return s.astype(np.int32), t.astype(np.int32), d.astype(np.int32)


def fixture_index(sel):
    """the fixture rows behind A / A1 (for the enumeration model of tests/search_lanes.py)"""
    dice = L.g10()[2]
    nd = np.nonzero(dice[:, 0] != dice[:, 1])[0]
    return nd[:N] if sel == "A" else nd[8:9]


def live(sel):
    return int((lanes(sel)[0] != OVER).any(axis=1).sum())


def moves_to_play(sel):
    """the checker moves the live lanes of a set have to play with their dice: 2 per lane, 4 with doubles -- the size of what a step on
    them leaves in the env's arenas"""
    st, _, d = lanes(sel)
    return int(np.where(d[:, 0] == d[:, 1], 4, 2)[(st != OVER).any(axis=1)].sum())


@functools.lru_cache(maxsize=None)
def positions(sel, n):
    """-> (states int32 [n, 28], turn int32 [n]): late = fixture boards late in the game (a played-out trial is short), picks = six
    boards spread over the fixture and the start position, bad = picks with |count| > 15 in the last one (BGAMD_E_STATE)"""
    if sel == "late":
        return RC.late_boards(n)
    gst, gtu = RC.g10_picks()
    st = np.concatenate([gst, OR.START[None], gst[:1]]).astype(np.int32)[:n]
    tu = np.concatenate([gtu, [0], 1 - gtu[:1]]).astype(np.int32)[:n]
    assert len(st) == n
    if sel == "bad":
        st = st.copy()
        st[-1, 5] = 16
    return st, tu


# ---- the entries -------------------------------------------------------------------------------------------------------------------------

def E(name, op, reads=(), **kw):
    return dict(name=name, op=op, kw=kw, reads=tuple(reads))


STATE = ("snapshot", "progress", "stats")
GREEDY_READS = ("last_choice", "unique_rows", "choice_spread") + STATE
SEARCH_READS = ("search_candidates", "search_info", "last_choice") + STATE
RO = dict(per_trial=True, seed=RO_SEED)
CUBE = dict(double_at=0.68, pass_at=0.76, too_good_at=0.97, max_cube=8, jacoby=True)


def _probes(s, s3):
    """the probes on lane set s (s3: the 3-ply step's)"""
    one = s == "A1"
    ro = dict(RO, lanes=32) if one else dict(RO, lanes=64)
    return [
        E("greedy", "greedy", GREEDY_READS, lanes=s, want_index=True),
        E("run_greedy", "run_greedy", ("last_choice",) + STATE, lanes=s, n_steps=5, epsilon=0.1),
        E("random", "random", STATE, lanes=s, walk=False),
        E("random_walk", "random", STATE, lanes=s, walk=True),
        E("sampled", "sampled", ("sample_info", "last_choice") + STATE, lanes=s, temperature=0.05),
        E("run_sampled", "run_sampled", ("sample_info", "last_choice") + STATE, lanes=s, n_steps=3, temperature=0.05),
        E("search_k3", "search", SEARCH_READS, lanes=s, top_k=3),
        E("search_all", "search", SEARCH_READS, lanes=s, top_k=0, only_player=None if one else 0, slot=1),
        E("search_filtered", "search", SEARCH_READS, lanes=s, top_k=3, margin=0.04),
        E("search3", "search", SEARCH_READS[:1] + ("search3_info",) + SEARCH_READS[1:], lanes=s3, top_k=2, plies=3, deep_k=2,
          reply_top_k=2),
        E("analyze", "analyze", ("analysis",) + STATE, lanes=s, top_k=4),
        E("preroll", "preroll", (), pos=("late", 2 if one else 8)),
        E("ro_plain", "rollout", ("rollout_info", "outcomes", "paired_value", "paired_equity"), pos=("late", 2 if one else 5),
          trials=3 if one else 7, max_plies=0, **ro),
        E("ro_vr", "rollout", ("rollout_info", "vr", "paired_vr"), pos=("late", 2 if one else 6), trials=5, max_plies=5,
          variance_reduction=True, **ro),
        E("ro_2ply", "rollout", ("rollout_info", "paired_value"), pos=("late", 2 if one else 3), trials=4, max_plies=3, plies=2, top_k=2,
          margin=0.1, **ro),
        E("ro_groups", "rollout", ("rollout_info", "outcomes", "vr", "paired_value", "paired_vr", "paired_equity"),
          pos=("late", 2 if one else 6), trials=6, max_plies=4, variance_reduction=True, groups=(0, 0) if one else (0, 0, 1, 1, 1, 2), **ro),
        E("ro_cube", "rollout", ("rollout_info", "cube", "cube_info", "paired_cubeful"), pos=("late", 2 if one else 4), trials=8,
          max_plies=6, variance_reduction=True, groups=(0, 0) if one else (0, 0, 1, 1), cube=CUBE, **ro),
        E("evaluate_f32", "evaluate", (), pos=("late", 1 if one else 8), precision="F32"),
        E("evaluate_f16x2", "evaluate", (), pos=("late", 1 if one else 8), precision="F16X2"),
        E("evaluate_bf16", "evaluate", (), pos=("late", 1 if one else 8), precision="BF16", slot=1),
        E("evaluate_incremental", "evaluate_incremental", (), lanes=s, roots=1 if one else 6),          # (its arenas are scratch: no read)
        E("encode", "encode", (), pos=("late", 8)),
        E("encode_rows", "encode_rows", (), pos=("late", 8)),
        E("enumerate", "enumerate", (), lanes=s),
        E("legal_moves", "legal_moves", (), lanes=s),
        E("try_move", "try_move", STATE, lanes=s),
        E("log_trajectory", "log_trajectory", STATE, lanes=s, max_plies=4, steps=3),
        E("log_ring", "log_ring", STATE, lanes=s, ring_steps=4, steps=5),
        E("log_search", "log_search", STATE, lanes=s, max_plies=3, steps=2, top_k=2),
    ]


PROBES = _probes("A", "A3")
PROBES_1 = [e for e in _probes("A1", "A1") if e["name"] in ("greedy", "sampled", "search_k3", "search_all", "search3", "analyze", "preroll",
                                                               "ro_plain", "ro_vr", "ro_2ply", "evaluate_incremental", "log_search")]

SRO = dict(per_trial=True, seed=RO_OTHER_SEED, rotate=True)
SOIL_CUBE = dict(double_at=0.6, pass_at=0.8, too_good_at=1.0, max_cube=64, hold_turn0=True)

# In this order.  `refuse`: the call must return that code and leave snapshot, progress, stats and dice as they were.  `big`: the names of
# the probes this step is the larger partner of (the targeted pairs run it directly before each of them).
SOIL = [
    E("reads_before_their_call", "refused_reads"),
    E("weights_slot0", "load", nets=(SOIL_NETS[0], None)),
    E("search_empty_slot", "search", lanes="B", top_k=2, slot=1, refuse=E_NOWEIGHTS),
    E("weights_slot1", "load", nets=(None, SOIL_NETS[1])),
    E("small_search", "search", SEARCH_READS, lanes="B3", top_k=1, margin=0.5),
    E("small_rollout", "rollout", ("rollout_info",), pos=("picks", 1), trials=2, max_plies=2, lanes=32, **SRO),
    E("small_search3", "search", SEARCH_READS, lanes="A3", top_k=2, plies=3, deep_k=2, reply_top_k=1, only_player=0),
    E("reseed_other", "reseed", seed=OTHER_SEED),
    E("time_kernels_on", "setting", what="time_kernels", on=True),
    E("big_greedy", "greedy", GREEDY_READS, lanes="B", want_index=False,
      big=("greedy", "evaluate_incremental", "enumerate", "legal_moves", "try_move")),
    E("big_run_greedy", "run_greedy", ("last_choice",) + STATE, lanes="B", n_steps=9, epsilon=0.3, big=("run_greedy",)),
    E("time_kernels_off", "setting", what="time_kernels", on=False),
    E("big_random", "random", STATE, lanes="B", walk=False, big=("random",)),
    E("big_random_walk", "random", STATE, lanes="B", walk=True, big=("random_walk",)),
    E("big_sampled", "sampled", ("sample_info", "last_choice") + STATE, lanes="B", temperature=1.5, big=("sampled",)),
    E("big_run_sampled", "run_sampled", ("sample_info", "last_choice") + STATE, lanes="B", n_steps=6, temperature=0.7, slot=1,
      big=("run_sampled",)),
    E("big_search", "search", SEARCH_READS, lanes="B", top_k=12, big=("search_k3", "search_all", "search_filtered", "log_search", "search3")),
    E("big_search3", "search", SEARCH_READS[:1] + ("search3_info",) + SEARCH_READS[1:], lanes="B3", top_k=3, plies=3, deep_k=3,
      reply_top_k=1, big=("search3",)),
    E("big_analyze", "analyze", ("analysis",) + STATE, lanes="B", top_k=10, big=("analyze",)),
    E("analyze_no_afterstates", "analyze", ("analysis",), lanes="B", top_k=2, played="start", status=3),
    E("big_preroll", "preroll", (), pos=("picks", 8), slot=1),
    E("preroll_bad_board", "preroll", (), pos=("bad", 8), refuse=E_STATE),
    E("big_ro_plain", "rollout", ("rollout_info", "outcomes", "paired_value", "paired_equity"), pos=("picks", 8), trials=36, max_plies=6,
      big=("ro_plain",), **SRO),
    E("rollout_bad_board", "rollout", (), pos=("bad", 8), trials=36, max_plies=6, variance_reduction=True, refuse=E_STATE, **SRO),
    E("reads_after_a_failed_rollout", "refused_reads", only=("rollout_vr_read", "rollout_outcomes_read", "rollout_paired_read",
                                                             "rollout_cube_read")),
    E("big_ro_vr", "rollout", ("rollout_info", "vr", "paired_vr"), pos=("picks", 8), trials=36, max_plies=6, variance_reduction=True,
      big=("ro_vr", "preroll"), **SRO),
    E("policy_set", "setting", what="rollout_policy", on=True),
    E("big_ro_2ply", "rollout", ("rollout_info", "paired_value"), pos=("picks", 4), trials=8, max_plies=4, lanes=96, policy_in_force=True,
      big=("ro_2ply",), **SRO),
    E("policy_cleared", "setting", what="rollout_policy", on=False),
    E("big_ro_groups", "rollout", ("rollout_info", "outcomes", "vr", "paired_value", "paired_vr", "paired_equity"), pos=("picks", 8),
      trials=36, max_plies=5, variance_reduction=True, groups=(3, 3, 3, 0, 0, 7, 7, 7), big=("ro_groups",), **SRO),
    E("cube_set", "setting", what="rollout_cube", on=True, rule=SOIL_CUBE, value=(2, 1, 4, 2, 1, 1, 8, 2), owner=(1, 0, 2, 1, 0, 0, 2, 1)),
    E("big_ro_cube", "rollout", ("rollout_info", "cube", "cube_info", "paired_cubeful"), pos=("picks", 8), trials=36, max_plies=6,
      variance_reduction=True, groups=(0, 0, 0, 0, 1, 1, 1, 1), cube_in_force=True, big=("ro_cube",), **SRO),
    E("cube_cleared", "setting", what="rollout_cube", on=False),
    E("big_evaluate", "evaluate", (), pos=("picks", 8), precision="F16X2", repeat=8,
      big=("evaluate_f32", "evaluate_f16x2", "evaluate_bf16", "encode", "encode_rows")),
    E("log_trajectory_set", "log_trajectory", STATE, lanes="B", max_plies=9, steps=7, big=("log_trajectory",)),
    E("search_with_a_log", "search", lanes="B", top_k=2, log="trajectory", refuse=E_INVALID),
    E("log_ring_set", "log_ring", STATE, lanes="B", ring_steps=3, steps=8, big=("log_ring",)),
    E("log_search_set", "log_search", STATE, lanes="B", max_plies=5, steps=4, top_k=4),
    E("greedy_with_a_search_log", "greedy", lanes="B", log="search", refuse=E_INVALID),
    E("reseed_back", "reseed", seed=SEED),
]

SOIL_1 = [
    E("weights", "load", nets=SOIL_NETS),
    E("big_greedy", "greedy", GREEDY_READS, lanes="B1", want_index=False, big=("greedy", "sampled", "evaluate_incremental", "search3")),
    E("big_analyze", "analyze", ("analysis",) + STATE, lanes="B1", top_k=36, big=("search_k3", "search_all", "analyze", "log_search")),
    E("big_search3", "search", SEARCH_READS, lanes="A1", top_k=0, plies=3, deep_k=0, reply_top_k=1, big=("search3",)),
    E("big_ro_vr", "rollout", ("rollout_info", "vr"), pos=("picks", 3), trials=12, max_plies=4, variance_reduction=True, lanes=64,
      big=("ro_plain", "ro_vr", "preroll"), **SRO),
    E("big_ro_2ply", "rollout", ("rollout_info",), pos=("picks", 3), trials=6, max_plies=3, plies=2, top_k=3, margin=0.2, lanes=48,
      big=("ro_2ply",), **SRO),
]

# every sticky setting of the C ABI: SOIL holds an entry that sets it and, later, one that clears it, with something run in between
SETTINGS = {"rollout_policy": ("policy_set", "policy_cleared"), "rollout_cube": ("cube_set", "cube_cleared"),
            "time_kernels": ("time_kernels_on", "time_kernels_off"), "reseed": ("reseed_other", "reseed_back")}
# the three logs are set, stepped under and unset inside ONE entry each (the log_* ops of the runner do all three): the table can only
# name that entry, and what the CPU test holds is that its op is the one that does so.  The weight slots are not set and cleared but
# loaded with SOIL's tables and loaded back by the runner's restore(): test_other_content holds the loads.
LOG_SETTINGS = {"trajectory": ("log_trajectory_set", "log_trajectory"), "ring": ("log_ring_set", "log_ring"),
                "search_log": ("log_search_set", "log_search")}
SOIL_POLICY = dict(plies=2, top_k=3, margin=0.05)


# ---- the reads that can be refused ---------------------------------------------------------------------------------------------------------

# read call of include/bgamd.h -> (the runner's read that makes it, the probe whose call it reads).  Each is BGAMD_E_INVALID before that
# call.  The read calls of the header that are never refused, with the reason, are in NEVER_REFUSED: the CPU test holds the two lists
# against the header.
REFUSABLE = {
    "bgamd_env_sample_info": ("sample_info", "sampled"),
    "bgamd_env_search_read": ("search_candidates", "search_k3"),
    "bgamd_env_search_info": ("search_info", "search_k3"),
    "bgamd_env_search3_read": ("search_candidates", "search3"),
    "bgamd_env_search3_info": ("search3_info", "search3"),
    "bgamd_env_analysis_read": ("analysis", "analyze"),
    "bgamd_env_rollout_vr_read": ("vr", "ro_vr"),
    "bgamd_env_rollout_outcomes_read": ("outcomes", "ro_plain"),
    "bgamd_env_rollout_paired_read": ("paired_value", "ro_groups"),
    "bgamd_env_rollout_cube_read": ("cube", "ro_cube"),
    "bgamd_env_choice_spread": ("choice_spread", "greedy"),
}
NEVER_REFUSED = {
    "bgamd_env_candidates_info": "reads the enumerate arena as it stands; bgamd_env_enumerate's own pair, compared by the enumerate probe",
    "bgamd_env_candidates_read": "as bgamd_env_candidates_info",
    "bgamd_env_last_choice": "per-lane words that exist from creation on",
    "bgamd_env_rollout_info": "host numbers, zeros before the first rollout",
    "bgamd_env_rollout_cube_info": "host numbers, zeros before the first cubeful rollout",
    "bgamd_env_stats": "the counters",
    "bgamd_env_unique_rows_info": "the arenas as they stand (cleared at creation)",
    "bgamd_env_unique_rows_read": "as bgamd_env_unique_rows_info",
    "bgamd_env_kernel_choice": "host numbers",
    "bgamd_env_kernel_times": "host numbers",
    "bgamd_env_scratch_info": "host numbers",
}
# the reads above that are not refused, compared in the same way: (read, probe)
ALSO_READ = (("last_choice", "greedy"), ("last_choice", "search_k3"), ("unique_rows", "greedy"), ("rollout_info", "ro_plain"),
             ("cube_info", "ro_cube"))

# Calls made between a probe's call and its reads.  `rewrites`: the reads this call is documented to answer anew or to rewrite (its own
# reads; bgamd_env_analyze_moves and bgamd_evaluate_incremental use the arenas as scratch and say so) -- those pairs are left out.  Every
# other read must then be refused with BGAMD_E_INVALID or return the bits it returned directly after its own call.
_STEP_ROWS = ("last_choice", "unique_rows", "choice_spread")
INTERVENING = [
    E("preroll", "preroll", pos=("picks", 7), rewrites=()),
    E("rollout", "rollout", pos=("picks", 3), trials=4, max_plies=3, lanes=32, seed=RO_OTHER_SEED,
      rewrites=("vr", "outcomes", "paired_value", "cube", "rollout_info")),
    E("analyze", "analyze", lanes="B", top_k=2, played="start", rewrites=("analysis", "unique_rows", "choice_spread", "search_candidates", "search_info",
                                                        "search3_info")),
    E("evaluate_incremental", "evaluate_incremental", lanes="A", roots=3, rewrites=("unique_rows", "choice_spread")),
    E("evaluate", "evaluate", pos=("picks", 8), precision="F32", rewrites=()),
    E("greedy", "greedy", lanes="B", rewrites=_STEP_ROWS),
    E("search", "search", lanes="B", top_k=2, rewrites=_STEP_ROWS + ("search_candidates", "search_info", "search3_info")),
    E("refused_rollout", "rollout", pos=("bad", 8), trials=4, max_plies=3, lanes=32, seed=RO_OTHER_SEED, refuse=E_STATE,
      rewrites=("vr", "outcomes", "paired_value", "cube")),
    E("refused_search", "search", lanes="B", top_k=2, log="trajectory", refuse=E_INVALID, rewrites=()),
]
# after these the read MUST be refused (a call that invalidates it): (read, probe, intervening call)
MUST_REFUSE = (("search_candidates", "search_k3", "analyze"), ("search_info", "search_k3", "analyze"),
               ("search3_info", "search3", "search"), ("search3_info", "search3", "analyze"),
               ("vr", "ro_vr", "rollout"), ("cube", "ro_cube", "rollout"),
               ("vr", "ro_vr", "refused_rollout"), ("outcomes", "ro_plain", "refused_rollout"),
               ("paired_value", "ro_groups", "refused_rollout"), ("cube", "ro_cube", "refused_rollout"))
LAZY = ("search_info", "search3_info")                 # counted when first asked for: also asked for the first time only after the call


def read_pairs():
    """-> [(read, probe name, intervening entry, lazy)]: lazy = the read is not made before the intervening call"""
    out = []
    for read, probe in list(REFUSABLE.values()) + list(ALSO_READ):
        for x in INTERVENING:
            if read in x["kw"]["rewrites"] and (read, probe, x["name"]) not in MUST_REFUSE:
                continue
            out.append((read, probe, x, False))
            if read in LAZY:
                out.append((read, probe, x, True))
    return out


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------

def search_lanes(n_virtual):
    return PL.scratch_lanes(n_virtual)


def _round256(x):
    return -(-x // 256) * 256


def rollout_request(e, policy=None, cube=False):
    """the request tuple of tests/rollout_plan_ref.py for a rollout entry"""
    kw = e["kw"]
    P = kw["pos"][1]
    flags = (PL.ROTATE if kw.get("rotate", True) else 0) | (PL.VR if kw.get("variance_reduction") else 0) | (PL.SLOT1 if kw.get("slot") else 0)
    plies, top_k = (kw.get("plies", 1), kw.get("top_k", 4)) if policy is None else (policy["plies"], policy["top_k"])
    return (flags, P, 0, kw["trials"], kw["max_plies"], kw.get("lanes", 0), True, "groups" in kw, plies, top_k,
            bool(cube or kw.get("cube") or kw.get("cube_in_force")), True, True)


def families(e):
    """{family: size} of an entry.  Sizes are what the call asks of the kept state -- an upper bound where the device decides (a filtered
    or top_k = 0 search reads its list's length back): scratch / mid / rscratch in lanes, search_buffers in candidate rows,
    rollout_buffers in trials, arenas in checker moves to play (moves_to_play) or rows handed over.  Families without a size map to 0."""
    op, kw = e["op"], e["kw"]
    f = {}
    if op in ("greedy", "run_greedy", "random", "sampled", "run_sampled", "enumerate", "legal_moves", "try_move", "log_trajectory", "log_ring"):
        f["arenas"] = moves_to_play(kw["lanes"])
        f["flags"] = 0
        if op.startswith("log"):
            f["logs"] = 0
    elif op in ("search", "analyze", "log_search"):
        k = kw.get("top_k", 0)
        kept = kept_bound(kw["lanes"], k, kw.get("only_player"))
        extra = 1 if op == "analyze" else 0                                # (the played afterstate beside the top_k)
        n_cand = sum(c + extra for c in kept)
        if k > 0 and "margin" not in kw and kw.get("plies", 2) == 2:
            n_cand = len(lanes(kw["lanes"])[0]) * (k + extra)              # sized up front: n (top_k [+ 1]), no list length is read back
        f.update(arenas=moves_to_play(kw["lanes"]), search_buffers=n_cand, scratch=search_lanes(n_cand * ROLLS), flags=0)
        if kw.get("plies") == 3:                                           # the deep set: lanes that kept two or more, at most deep_k each
            dk, rk = kw["deep_k"], kw["reply_top_k"]
            assert rk > 0
            n_mid = sum(min(dk, c) if dk > 0 else c for c in kept if c >= 2) * ROLLS
            f["mid"] = _round256(n_mid)
            f["scratch"] = max(f["scratch"], search_lanes(n_mid * rk * ROLLS))
            f["search_buffers"] = max(f["search_buffers"], n_mid * rk)
        if op == "log_search":
            f["logs"] = 0
    elif op == "preroll":
        f.update(scratch=search_lanes(kw["pos"][1] * ROLLS), rollout_buffers=kw["pos"][1])
    elif op == "rollout":
        p = PL.plan(rollout_request(e, SOIL_POLICY if kw.get("policy_in_force") else None))
        assert p["rc"] == 0, e["name"]
        f.update(rscratch=p["L"], rollout_buffers=p["N"], flags=0)
        lanes_wanted = max(p["search_scratch_lanes"], p["preroll_lanes"])
        if lanes_wanted:
            f["scratch"] = lanes_wanted
        if p["two_ply"]:
            f["search_buffers"] = p["L"] * (kw.get("top_k", 4) if not kw.get("policy_in_force") else SOIL_POLICY["top_k"])
        if p["two_ply"] or p["cube"]:
            f["settings"] = 0
    elif op == "evaluate":
        f["arenas"] = kw["pos"][1] * kw.get("repeat", 1)
    elif op == "evaluate_incremental":
        f["arenas"] = kw["roots"]
    elif op in ("encode", "encode_rows", "refused_reads"):
        pass
    elif op == "load":
        f["weights"] = 0
    elif op in ("setting", "reseed"):
        f["settings"] = 0
    else:
        raise KeyError(op)
    if "slot" in kw:
        f["weights"] = 0
    return f


@functools.lru_cache(maxsize=None)
def kept_bound(sel, top_k, only_player=None):
    """-> for every lane that takes part, a bound on the candidates it keeps: min(top_k, its distinct afterstates) on the probes' boards
    (the enumeration model of tests/search_lanes.py; top_k = 0: all of them), top_k on SOIL's boards, whose steps all have top_k > 0"""
    st, tu, _ = lanes(sel)
    part = [g for g in range(len(st)) if (st[g] != OVER).any() and only_player in (None, int(tu[g]))]
    if sel not in ("A", "A3", "A1"):
        assert top_k > 0, "top_k = 0 is sized by enumeration: only on the probes' boards"
        return tuple(top_k for _ in part)
    idx = fixture_index("A1" if sel == "A1" else "A")
    counts = [len(L.afterstates(int(idx[g]))) for g in part]
    return tuple(min(top_k, c) if top_k > 0 else c for c in counts)


def by_name(entries):
    return {e["name"]: e for e in entries}


def partner(probe_name, soil):
    """the SOIL entries that name the probe in `big`"""
    return [e for e in soil if probe_name in e["kw"].get("big", ())]
