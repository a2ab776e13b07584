"""An independent restatement of the greedy step's dispatch, for tests/test_step_plan_cpu.py to hold csrc/bg_step_plan.h against.

Transcribed from the host code of commit b4eb3c8 ("State the kernel order once (KERNEL_ORDER); launches stand where used"), the parent
of the change that introduced bg_step_plan.h -- from env_create (the two getenv blocks), env_allocate (the arena's default size),
GreedyRun::init / egrid / step, launch_eval, launch_root_pass, launch_sample_passes and bgamd_evaluate_incremental in csrc/bgamd.hip as
they stood there -- and NOT from the new header: it follows those functions' order of statements, one Python line per C line, so that
the two are two derivations."""
import re

# the constants of csrc/bg_staged.h, bg_staged_kernels.h, bg_eval.h, bg_root_resident.h, bg_eval_dense16.h, bg_search.h at that commit
XALL_NT = 512
LIST_SHARDS = 4
N_ARENAS = 4
DELTA_THREADS = 1024
EVAL_THREADS = 768
LANE_NT = 256
BROOT_THREADS = 256
ROOT3_THREADS = 512
BG_D16_WAVES = 3
SRCH_NT = 256
EXPAND_NT_PLY, EXPAND_NT_LEAF = 512, 1024
F32, BF16, F16X2, F32_DENSE = 0, 1, 2, 3          # include/bgamd.h


def _atoi(s):
    """C's atoi on text that fits: blanks, a sign, digits; anything else ends the number, none at all is 0"""
    m = re.match(r"[ \t\n\v\f\r]*([+-]?[0-9]+)", s)
    return int(m.group(1)) if m else 0


def default_cap_rows(n_games, arena_rows=0):
    """env_allocate: the row arena of an env"""
    cap = arena_rows if arena_rows > 0 else n_games * 256
    if cap < 65536:
        cap = 65536
    if cap > (1 << 31) - 64:
        cap = (1 << 31) - 64
    return cap


def tuning(env, experimental, n_games):
    """env_create: env is a dict of the variables that are set -> the members of bgamd_env they decide (the members' initialisers first)"""
    get = env.get
    u = dict(mfma_delta=0, d16=0, list_shards=1, split_arena=1, expand_merged=1, expand_parts=3, expand_dbl_npb=128, expand_dbl_pct=0,
             root_in_boundary=1, overlap=1, root_f32_mfma=0, root_resident=1)
    if experimental:
        on = lambda name: int(get(name) is not None and _atoi(get(name)) != 0)
        off = lambda name: get(name) is not None and _atoi(get(name)) == 0
        u["root_f32_mfma"] = on("BGAMD_ROOT_F32")
        u["root_resident"] = int(not off("BGAMD_ROOT_RESIDENT"))
        u["mfma_delta"] = on("BGAMD_MFMA_DELTA")
        u["d16"] = on("BGAMD_F16X2_RESIDENT")
    u["root_in_boundary"] = int(n_games >= 24576 and LANE_NT == BROOT_THREADS)
    u["overlap"] = 0
    if experimental:
        rib = get("BGAMD_ROOT_IN_BOUNDARY")
        if rib is not None:
            u["root_in_boundary"] = int(_atoi(rib) != 0 and LANE_NT == BROOT_THREADS)
        xm = get("BGAMD_EXPAND_MERGED")
        u["expand_merged"] = int(_atoi(xm) != 0) if xm is not None else 1
        xp = get("BGAMD_EXPAND_DBL_PCT")
        if xp is not None and _atoi(xp) >= 5 and _atoi(xp) <= 95:
            u["expand_dbl_pct"] = _atoi(xp)
        ls = get("BGAMD_LIST_SHARDS")
        u["list_shards"] = int(_atoi(ls) != 0) if ls is not None else 1
        sa = get("BGAMD_SPLIT_ARENA")
        u["split_arena"] = int(_atoi(sa) != 0) if sa is not None else 1
        xq = get("BGAMD_EXPAND_PARTS")
        if xq is not None and _atoi(xq) >= 1 and _atoi(xq) <= 3:
            u["expand_parts"] = _atoi(xq)
        xn = get("BGAMD_EXPAND_DBL_NPB")
        if xn is not None and _atoi(xn) >= 64 and _atoi(xn) <= XALL_NT:
            u["expand_dbl_npb"] = _atoi(xn) & ~63
        u["overlap"] = int(get("BGAMD_NO_OVERLAP") is None and get("BGAMD_OVERLAP") is not None and _atoi(get("BGAMD_OVERLAP")) != 0)
    return u


def _egrid(max_items, nt, n_cu):
    """GreedyRun::egrid"""
    b = (max_items + nt - 1) // nt
    lim = n_cu * (1 if nt >= 1024 else 2048 // nt)
    return 1 if b < 1 else (lim if b > lim else b)


def root_pass(u, n, n_cu, f32_chain, experimental):
    """launch_root_pass -> (kernel_choice code of the kernel it launches, its grid)"""
    if experimental and f32_chain and u["root_f32_mfma"]:
        return 3, n_cu
    if experimental and not u["root_resident"]:
        blocks = ((n + 31) // 32 + ROOT3_THREADS // 64 - 1) // (ROOT3_THREADS // 64)
        if blocks > n_cu:
            blocks = n_cu
        return 2, (1 if blocks < 1 else blocks)
    blocks = (n + 31) // 32
    if blocks > 2 * n_cu:
        blocks = 2 * n_cu
    return 1, (1 if blocks < 1 else blocks)


def eval_grids(est_rows, n_cu):
    """launch_eval -> (egrid, the d16 kernel's workgroups)"""
    eb = (est_rows + (EVAL_THREADS // 64) * 32 - 1) // ((EVAL_THREADS // 64) * 32)
    eb = 1 if eb < 1 else (n_cu if eb > n_cu else eb)
    tiles = (est_rows + 31) // 32
    per_cu = BG_D16_WAVES
    wg = 1 if tiles < 1 else (per_cu * n_cu if tiles > per_cu * n_cu else tiles)
    return eb, wg


def delta_blocks(rows, n_cu):
    """dblocks of GreedyRun::step (rows = n * 24) and of bgamd_evaluate_incremental (rows = n)"""
    dblocks = (rows + DELTA_THREADS - 1) // DELTA_THREADS
    return 1 if dblocks < 1 else (n_cu if dblocks > n_cu else dblocks)


def rnd_count_blocks(tasks, n_cu):
    """the rnd_count_kernel launches of bgamd_env_step_random (tasks = n * 64) and of the exploring greedy step (n * 4)"""
    b = (tasks + 255) // 256
    lim = n_cu * 8
    return lim if b > lim else b


def plan(u, n, n_cu, cap_rows, precision, wm_ok, experimental, pct_thresholds=(49152, 24576), shards_need_division=True, b_base_rounded=True):
    """GreedyRun::init and the launches of GreedyRun::step on an env of n lanes -> a dict named like the driver's output.
    The three keyword arguments exist for the test's deliberately wrong references."""
    r = {}
    incremental = precision == F32
    r["incremental"] = int(incremental)
    b_base = ((cap_rows // N_ARENAS) & (~63 if b_base_rounded else ~0)) if (incremental and u["split_arena"]) else 0
    slots = (1024 // XALL_NT) * n_cu
    nd = (n * 4 + 63) // 64
    pct = u["expand_dbl_pct"] if u["expand_dbl_pct"] > 0 else (62 if n >= pct_thresholds[0] else (70 if n >= pct_thresholds[1] else 50))
    nd_lim = slots * pct // 100
    if nd_lim >= LIST_SHARDS:
        nd_lim -= nd_lim % LIST_SHARDS
    nd = 1 if nd < 1 else (nd_lim if nd > nd_lim else nd)
    nl = (n * 16 + XALL_NT - 1) // XALL_NT
    nl_lim = 1 if slots - nd_lim < 1 else slots - nd_lim
    nl = 1 if nl < 1 else (nl_lim if nl > nl_lim else nl)
    r["xall_nd"], r["xall_nl"] = nd, nl
    divides = (nd % LIST_SHARDS == 0 and nl % LIST_SHARDS == 0) if shards_need_division else True
    r["shards"] = LIST_SHARDS if (u["expand_merged"] and u["list_shards"] and divides) else 1
    mdelta = bool(experimental and u["mfma_delta"] and wm_ok)
    if mdelta:
        b_base = 0
    r["b_base"] = b_base
    # step
    r["choice0"] = (1 if (u["mfma_delta"] and wm_ok) else 0) if incremental else (2 if precision == F32_DENSE else ((4 if u["d16"] else 3) if precision == F16X2 else 5))
    r["delta_mfma"] = int(incremental and mdelta)
    root_code, root_grid = root_pass(u, n, n_cu, True, experimental)
    for tag, root_ready in (("own", False), ("ready", True)):
        own_root_launch = incremental and not root_ready
        r["own_launch_" + ("first" if tag == "own" else "ready")] = int(own_root_launch)
        r["choice1_" + tag] = 0 if not incremental else (4 if not own_root_launch else (3 if u["root_f32_mfma"] else (1 if u["root_resident"] else 2)))
        r["forked_%s_2nd" % tag] = 1 if own_root_launch else 0          # ss.root != s
    r["forked_own_1st"] = 0                                              # ss.root == s
    r["root"] = root_code if incremental else 0
    r["root_grid"] = root_grid if incremental else 0
    r["ply2_grid"] = _egrid(n * 4, EXPAND_NT_PLY, n_cu)
    r["leaf_grid"] = _egrid(n * 16, EXPAND_NT_LEAF, n_cu)
    r["fused_with_more"] = int(incremental or bool(u["expand_merged"]))
    r["delta_grid"] = delta_blocks(n * 24, n_cu)
    r["eval_grid"], r["d16_grid"] = eval_grids(n * 24, n_cu)
    want = (n * 24 + SRCH_NT - 1) // SRCH_NT
    ga = want if want < n_cu * 8 else n_cu * 8
    gb = want if want < n_cu * 2 else n_cu * 2
    r["sample_score_grid"], r["sample_pick_grid"] = (1 if ga < 1 else ga), (1 if gb < 1 else gb)
    r["rnd_count_grid"] = rnd_count_blocks(n * 4, n_cu)
    root_ready = incremental and bool(u["root_in_boundary"])
    if experimental and (u["root_f32_mfma"] or not u["root_resident"]):
        root_ready = False
    r["root_may_run_in_boundary"] = int(root_ready)
    return r


def outside(u, n, n_cu, experimental):
    """the launches outside a run: bgamd_evaluate_incremental over n roots and n rows (its root pass does not honour BGAMD_ROOT_F32),
    bgamd_evaluate_slot over n rows, bgamd_env_step_random"""
    r = {}
    r["inc_root"], r["inc_root_grid"] = root_pass(u, n, n_cu, False, experimental)
    r["inc_delta_grid"] = delta_blocks(n, n_cu)
    r["imm_eval_grid"], r["imm_d16_grid"] = eval_grids(n, n_cu)
    r["random_count_grid"] = rnd_count_blocks(n * 64, n_cu)
    return r
