"""The greedy step's plan (csrc/bg_step_plan.h) without a GPU: the header, compiled into tests/sanitize/step_plan_driver.cpp, against the
independent restatement of the dispatch it replaced (tests/step_plan_ref.py), field by field over every env size at which a grid or a
threshold can change, three CU counts, both arena sizes, the four precisions and every tuning; three deliberately wrong references that
the comparison must catch; every rule of the environment parser in numbers; and the same sweep once more through a driver built with
AddressSanitizer + UBSan (its own program: nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

import step_plan_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1:abort_on_error=0", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
N_CUS = (256, 64, 304)
PRECISIONS = (R.F32, R.BF16, R.F16X2, R.F32_DENSE)
TUNING_FIELDS = ("mfma_delta", "d16", "list_shards", "split_arena", "expand_merged", "expand_parts", "expand_dbl_npb", "expand_dbl_pct",
                 "root_in_boundary", "overlap", "root_f32_mfma", "root_resident")
PLAN_FIELDS = ("incremental", "delta_mfma", "b_base", "xall_nd", "xall_nl", "shards", "ply2_grid", "leaf_grid", "delta_grid", "eval_grid", "d16_grid",
               "root", "root_grid", "root_may_run_in_boundary", "fused_with_more", "sample_score_grid", "sample_pick_grid", "rnd_count_grid",
               "choice0", "choice1_own", "choice1_ready", "forked_own_2nd", "forked_ready_2nd", "forked_own_1st", "own_launch_first",
               "own_launch_ready")
OUTSIDE_FIELDS = ("inc_root", "inc_root_grid", "inc_delta_grid", "imm_eval_grid", "imm_d16_grid", "random_count_grid")


def build_driver(out, flags=()):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "backgammon-engine_amd", "csrc"),
                           os.path.join(ROOT, "tests", "sanitize", "step_plan_driver.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("step_plan") / "step_plan_driver")


def run(exe, experimental, tuning_env, cases, extra_env=None):
    """the driver with ONLY tuning_env of the library's variables set -> its line per case: tuning | plan | the callers outside a run"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("BGAMD_")}
    env.update(tuning_env)
    env.update(extra_env or {})
    stdin = "".join("%d %d %d %d %d\n" % c for c in cases)
    r = subprocess.run([exe, str(int(experimental))], env=env, input=stdin, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    return lines


def parse(line):
    """-> (tuning, plan, outside) as dicts of int"""
    parts = []
    for part in line.split("|"):
        w = part.split()
        parts.append(dict(zip(w[0::2], map(int, w[1::2]))))
    return parts


def render(tuning, plan, outside):
    """the reference's three dicts as the driver prints them: every field, in the driver's order"""
    assert len(tuning) == len(TUNING_FIELDS) and len(plan) == len(PLAN_FIELDS) and len(outside) == len(OUTSIDE_FIELDS)
    return " | ".join(" ".join("%s %d" % (k, d[k]) for k in names)
                      for names, d in ((TUNING_FIELDS, tuning), (PLAN_FIELDS, plan), (OUTSIDE_FIELDS, outside)))


# ---- the sweep -------------------------------------------------------------------------------------------------------------------

def lane_counts(n_cu):
    """every size 1 .. 600; the size thresholds and the powers of two around them with both neighbours; the sizes at which the
    expansion launch's two counts meet their limits (nd = ceil(4 n / 64) at the doubles share of the 2 n_cu resident workgroups, rounded
    down to the list parts, for each share; nl = ceil(16 n / 512) at the rest)"""
    edges = [24576, 49152, 32768, 65536, 131072, 1 << 30]
    slots = 2 * n_cu
    for pct in (50, 70, 62, 25):
        nd_lim = slots * pct // 100
        nd_lim -= nd_lim % 4
        edges += [16 * nd_lim, 32 * (slots - nd_lim)]
    return sorted(set(range(1, 601)) | {e + d for e in edges for d in (-1, 0, 1)})


def cases(n_cu):
    return [(n, n_cu, cap, prec, wm) for n in lane_counts(n_cu) for cap in (R.default_cap_rows(n), 32768) for prec in PRECISIONS
            for wm in (0, 1)]


_VALUES = {"BGAMD_EXPAND_DBL_PCT": ("25", "96"), "BGAMD_EXPAND_PARTS": ("2", "4"), "BGAMD_EXPAND_DBL_NPB": ("200", "513")}
VARS = ("BGAMD_ROOT_F32", "BGAMD_ROOT_RESIDENT", "BGAMD_MFMA_DELTA", "BGAMD_F16X2_RESIDENT", "BGAMD_ROOT_IN_BOUNDARY", "BGAMD_EXPAND_MERGED",
        "BGAMD_EXPAND_DBL_PCT", "BGAMD_LIST_SHARDS", "BGAMD_SPLIT_ARENA", "BGAMD_EXPAND_PARTS", "BGAMD_EXPAND_DBL_NPB", "BGAMD_OVERLAP",
        "BGAMD_NO_OVERLAP")


def tunings():
    """the default; every variable alone at 0, 1, an in-range middle value, an out-of-range one, "" and "x"; the second stream with and
    without BGAMD_NO_OVERLAP; the combinations tests/test_gpu_experimental.py sets"""
    ts = [{}]
    ts += [{k: v} for k in VARS for v in ("0", "1", *_VALUES.get(k, ("2", "1000")), "", "x")]
    ts += [{"BGAMD_OVERLAP": "1", "BGAMD_NO_OVERLAP": "0"}, {"BGAMD_OVERLAP": "1"}]
    ts += [{"BGAMD_ROOT_IN_BOUNDARY": "0", "BGAMD_OVERLAP": "1"}, {"BGAMD_EXPAND_MERGED": "1", "BGAMD_EXPAND_DBL_PCT": "25"},
           {"BGAMD_NO_OVERLAP": "1"}]                          # (the single switches of that module are among the lines above)
    return ts


_expected = {}


def expected(env, experimental, cs, **wrong):
    """the reference's answers for the cases as the driver's lines, computed once per distinct tuning (most values parse alike)"""
    small, large = R.tuning(env, experimental, 1), R.tuning(env, experimental, 1 << 20)
    key = (experimental, tuple(small.values()), tuple(large.values()), cs[0][1], tuple(sorted(wrong.items())))
    if key not in _expected:
        out = []
        for n, n_cu, cap, prec, wm in cs:
            u = R.tuning(env, experimental, n)
            out.append(render(u, R.plan(u, n, n_cu, cap, prec, bool(wm), experimental, **wrong), R.outside(u, n, n_cu, experimental)))
        _expected[key] = out
    return _expected[key]


@pytest.mark.parametrize("n_cu", N_CUS)
def test_plan_is_the_dispatch_it_replaced(driver, n_cu):
    """Every field of every tuning and plan equals what the parent commit's env_create, GreedyRun::init / step and launch_* decided inline;
    the default build (experimental false) reads no variable."""
    cs = cases(n_cu)
    default_lines = run(driver, False, {}, cs)
    n_plans = 0
    for env in tunings():
        for experimental in (False, True):
            lines = run(driver, experimental, env, cs)
            if not experimental:
                assert lines == default_lines, env
            for c, line, want in zip(cs, lines, expected(env, experimental, cs)):
                if line != want:                               # field by field: the fields that differ
                    diff = [sorted(set(g.items()) ^ set(w.items())) for g, w in zip(parse(line), parse(want))]
                    raise AssertionError((env, experimental, c, diff, line, want))
            n_plans += len(lines)
    assert n_plans == 2 * len(tunings()) * len(cs)


@pytest.mark.parametrize("wrong,field", [(dict(pct_thresholds=(49153, 24577)), "xall_nd"), (dict(shards_need_division=False), "shards"),
                                         (dict(b_base_rounded=False), "b_base")])
def test_a_wrong_reference_fails_the_comparison(driver, wrong, field):
    """The sweep can tell: the doubles share's size thresholds shifted by one, `shards` without the divisibility condition, b_base
    without its rounding to 64 rows -- each differs from the header somewhere in the default tuning's sweep, in its own field."""
    cs = cases(256)
    lines = run(driver, False, {}, cs)
    differing = set()
    for line, want in zip(lines, expected({}, False, cs, **wrong)):
        if line != want:
            got, ref = parse(line)[1], parse(want)[1]
            differing |= {k for k in got if got[k] != ref[k]}
    assert field in differing, differing


def _tuning(exe, env, experimental=True, n=1000):
    return parse(run(exe, experimental, env, [(n, 256, 65536, 0, 0)])[0])[0]


def test_env_parsing_rules(driver):
    """Every rule of step_tuning_from_env, stated here in numbers."""
    default = dict(mfma_delta=0, d16=0, list_shards=1, split_arena=1, expand_merged=1, expand_parts=3, expand_dbl_npb=128, expand_dbl_pct=0,
                   root_in_boundary=0, overlap=0, root_f32_mfma=0, root_resident=1)
    assert _tuning(driver, {}) == default and _tuning(driver, {}, False) == default
    for n, want in ((24575, 0), (24576, 1), (1 << 20, 1)):                        # the size rule, and its override
        assert _tuning(driver, {}, True, n)["root_in_boundary"] == want == _tuning(driver, {}, False, n)["root_in_boundary"]
        assert _tuning(driver, {"BGAMD_ROOT_IN_BOUNDARY": "0"}, True, n)["root_in_boundary"] == 0
        assert _tuning(driver, {"BGAMD_ROOT_IN_BOUNDARY": "1"}, True, n)["root_in_boundary"] == 1
        assert _tuning(driver, {"BGAMD_ROOT_IN_BOUNDARY": ""}, True, n)["root_in_boundary"] == 0
        assert _tuning(driver, {"BGAMD_ROOT_IN_BOUNDARY": "0"}, False, n)["root_in_boundary"] == want
    for var, field in (("BGAMD_ROOT_F32", "root_f32_mfma"), ("BGAMD_MFMA_DELTA", "mfma_delta"), ("BGAMD_F16X2_RESIDENT", "d16")):     # =1 enables
        for v, want in (("0", 0), ("", 0), ("x", 0), ("1", 1), ("7", 1), ("-1", 1)):
            assert _tuning(driver, {var: v})[field] == want, (var, v)
            assert _tuning(driver, {var: v}, False)[field] == 0
    for var, field in (("BGAMD_ROOT_RESIDENT", "root_resident"), ("BGAMD_EXPAND_MERGED", "expand_merged"), ("BGAMD_LIST_SHARDS", "list_shards"),
                       ("BGAMD_SPLIT_ARENA", "split_arena")):                                                                           # =0 disables
        for v, want in (("0", 0), ("00", 0), ("", 0), ("x", 0), ("1", 1), ("2", 1), ("-1", 1)):
            assert _tuning(driver, {var: v})[field] == want, (var, v)
            assert _tuning(driver, {var: v}, False)[field] == 1
    for v, want in (("4", 0), ("5", 5), ("50", 50), ("95", 95), ("96", 0), ("0", 0), ("-20", 0), ("", 0), ("x", 0), ("30x", 30)):
        assert _tuning(driver, {"BGAMD_EXPAND_DBL_PCT": v})["expand_dbl_pct"] == want, v
    for v, want in (("0", 3), ("1", 1), ("2", 2), ("3", 3), ("4", 3), ("", 3), ("x", 3)):
        assert _tuning(driver, {"BGAMD_EXPAND_PARTS": v})["expand_parts"] == want, v
    for v, want in (("63", 128), ("64", 64), ("127", 64), ("200", 192), ("512", 512), ("513", 128), ("0", 128), ("", 128), ("x", 128)):
        assert _tuning(driver, {"BGAMD_EXPAND_DBL_NPB": v})["expand_dbl_npb"] == want, v
    for env, want in (({"BGAMD_OVERLAP": "1"}, 1), ({"BGAMD_OVERLAP": "0"}, 0), ({"BGAMD_OVERLAP": ""}, 0), ({"BGAMD_OVERLAP": "x"}, 0),
                      ({"BGAMD_OVERLAP": "1", "BGAMD_NO_OVERLAP": "0"}, 0), ({"BGAMD_OVERLAP": "1", "BGAMD_NO_OVERLAP": ""}, 0),
                      ({"BGAMD_OVERLAP": "1", "BGAMD_NO_OVERLAP": "1"}, 0), ({"BGAMD_NO_OVERLAP": "1"}, 0), ({"BGAMD_NO_OVERLAP": "0"}, 0)):
        assert _tuning(driver, env)["overlap"] == want, env
        assert _tuning(driver, env, False)["overlap"] == 0


def test_step_plan_under_asan_ubsan(tmp_path):
    """The plan and the environment parser compiled with the sanitizers and run as their own program over the same sweep: every tuning,
    both builds' parsers, three CU counts, every env size; what the plans SAY is the tests' above."""
    exe = build_driver(tmp_path / "step_plan_driver_san", ("-fsanitize=address,undefined", "-fno-omit-frame-pointer"))
    for n_cu in N_CUS:
        cs = cases(n_cu)
        for env in tunings():
            for experimental in (False, True):
                run(exe, experimental, env, cs, SAN_ENV)
