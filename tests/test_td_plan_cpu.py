"""The learner's step plan (csrc/bg_td_plan.h) without a GPU: the header, compiled into tests/sanitize/td_plan_driver.cpp, against the
independent restatement of the dispatch it replaced (tests/td_plan_ref.py), field by field over every step size at which a route can
change; every kernel route of tests/test_gpu_learner_steps.py against the kernels its comment names; the trace-scale recurrence against
float64 as float32 bit patterns; every rule of the environment parser."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import td_plan_ref as R
from learner_routes import EXPECTED, ROUTES

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N_CUS = (256, 64, 304)
STEPS = (0, 1, 7)


def build_driver(out, flags=()):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "backgammon-engine_amd", "csrc"),
                           os.path.join(ROOT, "tests", "sanitize", "td_plan_driver.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("td_plan") / "td_plan_driver")


def run(exe, args, tuning_env, stdin="", extra_env=None):
    """the driver with ONLY tuning_env of the library's variables set"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("BGAMD_")}
    env.update(tuning_env)
    env.update(extra_env or {})
    r = subprocess.run([exe, *map(str, args)], env=env, input=stdin, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    return r.stdout.splitlines()


# ---- the sweep -------------------------------------------------------------------------------------------------------------------

def step_sizes(n_cu):
    """every size 1 .. 600, and every threshold, default and derived boundary with its two neighbours"""
    edges = [512, 4096, 8192, 24576, 65536, n_cu * 16] + [n_cu * R.TD_CHUNK * k for k in range(1, 6)]
    per = n_cu * R.TD_CHUNK
    edges += [(m * per * 19 + 19) // 20 for m in range(1, 6)]      # wide_even: the least n with 20 n >= 19 m per (m = chunks-per-CU rounds)
    edges += [3000, 24, 4]                                          # the mid values the tunings below set
    return sorted(set(range(1, 601)) | {e + d for e in edges for d in (-1, 0, 1) if e + d > 0})


_MID = {"BGAMD_TD_FUSE_G": "4", "BGAMD_TD_NG": "24", "BGAMD_TD_PIPE": "2", "BGAMD_TD_FUSE_STEP": "2", "BGAMD_TD_NO_WIDE_EVEN": "2",
        "BGAMD_TD_LAZY": "2", "BGAMD_TD_DENSE": "2", "BGAMD_TD_FUSED": "2"}
_TD_VARS = ("BGAMD_TD_MFMA_MIN", "BGAMD_TD_FUSED", "BGAMD_TD_DIRECT_MIN", "BGAMD_TD_NT_MIN", "BGAMD_TD_WIDE_MIN", "BGAMD_TD_PIPE",
            "BGAMD_TD_FUSE_STEP", "BGAMD_TD_FUSE_MIN", "BGAMD_TD_FUSE_G", "BGAMD_TD_NG", "BGAMD_TD_NO_WIDE_EVEN", "BGAMD_TD_LAZY",
            "BGAMD_TD_DENSE")


def tunings():
    """the default, the nine routes, every variable alone at 0, 1 and a mid value, FUSE_G values the parser refuses"""
    ts = [{}] + [dict(v) for v in ROUTES.values()]
    ts += [{k: v} for k in _TD_VARS for v in ("0", "1", _MID.get(k, "3000"))]
    ts += [{"BGAMD_TD_FUSE_G": v, "BGAMD_TD_DIRECT_MIN": "1", "BGAMD_TD_FUSE_MIN": "1"} for v in ("3", "5", "17", "32", "-1", "x", "")]
    return ts


def plan_lines(exe, env, experimental, n_cu, pairs):
    """-> the plans as tuples shaped like td_plan_ref.plan's"""
    lines = run(exe, ["plan", int(experimental), n_cu], env, "".join("%d %d\n" % p for p in pairs))
    assert len(lines) == len(pairs)
    out = []
    for (t, n), line in zip(pairs, lines):
        head, fwd, trace, tail = (x.split() for x in line.split("|"))
        assert [int(x) for x in head] == [n_cu, t, n]
        out.append((fwd[0], int(fwd[1]), trace[0], int(trace[1]), int(trace[2]), int(tail[0]), int(tail[1]), int(tail[2])))
    return out


@pytest.mark.parametrize("n_cu", N_CUS)
def test_plan_is_the_dispatch_it_replaced(driver, n_cu):
    """Every field of every plan equals what the parent commit's bgamd_td_step / td_fuse_g_for / bgamd_td_replay decided inline."""
    sizes = step_sizes(n_cu)
    pairs = [(t, n) for t in STEPS for n in sizes]
    n_plans = 0
    for env in tunings():
        for experimental in (False, True):
            u = R.tuning(env, experimental)
            got = plan_lines(driver, env, experimental, n_cu, pairs)
            for (t, n), g in zip(pairs, got):
                want = R.plan(u, n_cu, t, n, experimental)
                assert g == want, (env, experimental, n_cu, t, n, g, want)
            n_plans += len(got)
            delay = run(driver, ["delay", int(experimental), n_cu], env, "".join("%d\n" % n for n in sizes))
            assert [tuple(map(int, x.split())) for x in delay] == [(n, R.delay_g(u, n_cu, n)) for n in sizes], (env, experimental)
    assert n_plans == 2 * len(tunings()) * len(pairs)


@pytest.mark.parametrize("route", tuple(ROUTES))
def test_route_reaches_the_kernels_it_names(driver, route):
    """What tests/test_gpu_learner_steps.py takes on trust: under a route's setting, on 256 CUs, every step of 157 ... 1 running games (and of
    7 slots) runs exactly the kernels and template instances learner_routes.EXPECTED names -- by the header AND by the parent's logic."""
    env = ROUTES[route]
    forward, trace_first, trace_later, fuse_g, lazy = EXPECTED[route]
    sizes = list(range(1, 158))
    pairs = [(t, n) for t in (0, 1, 7, 156) for n in sizes]
    u = R.tuning(env, False)
    assert bool(u["lazy"]) == lazy and u["dense"] == 0
    got = plan_lines(driver, env, False, 256, pairs)
    for (t, n), g in zip(pairs, got):
        want = (forward, trace_first if t == 0 else trace_later, fuse_g, 1 if t == 0 or not lazy else 0)
        assert (g[0], g[2], g[6], g[7]) == want, (route, t, n, g)
        r = R.plan(u, 256, t, n, False)
        assert (r[0], r[2], r[6], r[7]) == want, (route, t, n, r)
    assert run(driver, ["tuning", 0], env)[11] == "lazy %d" % lazy


@pytest.mark.parametrize("lazy", (True, False))
@pytest.mark.parametrize("lam", (0.0, 0.25, 0.7, 1.0, 1.5))
def test_trace_scale_step(driver, lam, lazy):
    """td_scale_step over 400 steps against the float64 recurrence, the three kernel arguments as float32 bit patterns; with lazily scaled
    traces λ = 0.7 folds c back in at step 78 (0.7^78 < 2^-40) and λ = 1.5 at step 69 (1.5^69 > 2^40)."""
    lam32 = np.float32(lam)
    lines = run(driver, ["scale", "%.9g" % lam32, 400], {} if lazy else {"BGAMD_TD_LAZY": "0"})
    assert len(lines) == 400
    scale, folds = 55.0, []
    for t, line in enumerate(lines):
        emul, ginv, cmul, full, scale = R.scale_step(t, lam32, lazy, scale)
        want = "%d %08x %08x %08x %d" % (t, emul.view(np.uint32), ginv.view(np.uint32), cmul.view(np.uint32), full)
        got = line.rsplit(" ", 1)
        assert got[0] == want and float.fromhex(got[1]) == scale, (t, line, want, scale)
        if full and t > 0:
            folds.append(t)
    if not lazy or lam == 0.0:
        assert folds == list(range(1, 400))                     # every step an ordinary pass
    elif lam == 0.7:
        assert folds[:2] == [78, 156]
    elif lam == 1.5:
        assert folds[:2] == [69, 138]
    else:
        assert folds == ([] if lam == 1.0 else [21 * k for k in range(1, 20)])      # 2^-2: c = 2^-40 at step 20 is still inside


def _tuning(exe, env, experimental=False):
    return {k: int(v) for k, v in (x.split() for x in run(exe, ["tuning", int(experimental)], env))}


def test_env_parsing_rules(driver):
    """Every rule of td_tuning_from_env, stated here in numbers (and once more through the reference for every tuning of the sweep)."""
    assert _tuning(driver, {}) == dict(mfma_min=24576, fused=1, direct_min=512, nt_min=8192, wide_min=8192, pipe=1, fuse_step=1, fuse_min=512,
                                       fuse_g=0, slice_ng=0, no_wide_even=0, lazy=1, dense=0, fit_chunk=65536, fit_groups=256)
    for v, want in (("1", 1), ("2", 2), ("4", 4), ("8", 8), ("16", 16), ("0", 0), ("3", 0), ("32", 0), ("-1", 0), ("x", 0), ("", 0)):
        assert _tuning(driver, {"BGAMD_TD_FUSE_G": v})["fuse_g"] == want, v
    for v, want in (("0", 32), ("-7", 32), ("1", 32), ("32", 32), ("33", 64), ("1000", 1024), ("4194304", 1 << 22), ("4194305", 1 << 22),
                    ("99999999999", 1 << 22), ("x", 32)):
        assert _tuning(driver, {"BGAMD_FIT_CHUNK": v})["fit_chunk"] == want, v
    for v, want in (("0", 1), ("-5", 1), ("1", 1), ("7", 7), ("256", 256), ("257", 256), ("1000", 256), ("x", 1)):
        assert _tuning(driver, {"BGAMD_FIT_GROUPS": v})["fit_groups"] == want, v
    for experimental in (False, True):                         # BGAMD_TD_FUSED: the experimental build's alone
        assert _tuning(driver, {"BGAMD_TD_FUSED": "0"}, experimental)["fused"] == (0 if experimental else 1)
        assert _tuning(driver, {"BGAMD_TD_FUSED": "1"}, experimental)["fused"] == 1
    for v in ("", "0", "1", "no"):                             # BGAMD_TD_DENSE counts when merely present
        assert _tuning(driver, {"BGAMD_TD_DENSE": v})["dense"] == 1
    for var, field in (("BGAMD_TD_PIPE", "pipe"), ("BGAMD_TD_FUSE_STEP", "fuse_step"), ("BGAMD_TD_LAZY", "lazy")):      # =0 disables
        for v, want in (("0", 0), ("00", 0), ("x", 0), ("", 0), ("1", 1), ("2", 1), ("-1", 1)):
            assert _tuning(driver, {var: v})[field] == want, (var, v)
    for v, want in (("0", 0), ("", 0), ("x", 0), ("1", 1), ("7", 1)):                                                  # =1 enables
        assert _tuning(driver, {"BGAMD_TD_NO_WIDE_EVEN": v})["no_wide_even"] == want, v
    for var, field in (("BGAMD_TD_MFMA_MIN", "mfma_min"), ("BGAMD_TD_DIRECT_MIN", "direct_min"), ("BGAMD_TD_NT_MIN", "nt_min"),
                       ("BGAMD_TD_WIDE_MIN", "wide_min"), ("BGAMD_TD_FUSE_MIN", "fuse_min"), ("BGAMD_TD_NG", "slice_ng")):
        for v, want in (("0", 0), ("1", 1), ("3000", 3000), ("-4", -4), ("5000000000", 5000000000), ("12x", 12), ("x", 0)):
            assert _tuning(driver, {var: v})[field] == want, (var, v)
    for env in tunings():
        for experimental in (False, True):
            assert _tuning(driver, env, experimental) == R.tuning(env, experimental), (env, experimental)
