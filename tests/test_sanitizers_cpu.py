"""CPU-side sanitizer runs: the C oracle and the library's host-only code under AddressSanitizer + UBSan.
Never on the GPU box's device code (GPU ASan / XNACK builds are not available on this pool); these run wherever gcc does."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1:abort_on_error=0", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def _need(tool):
    if shutil.which(tool) is None:
        pytest.skip(tool + " not installed")


def _clean(r):
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]


def test_oracle_golden_suite_under_asan_ubsan(tmp_path):
    """oracle/bg_oracle.c compiled with -fsanitize=address,undefined (oracle/Makefile: libbg_oracle_asan.so) replays the
    tests.cpp known answers, fixtures G1-G5 (1 380 edge calls, 200 random and 24 greedy reference games) and 800 env steps
    of the lane driver: no out-of-bounds access, no undefined shift / overflow in the restatement the parity tests trust."""
    _need("gcc"); _need("make")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "libbg_oracle_asan.so"], stdout=subprocess.DEVNULL)
    libasan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan.so not found")
    env = dict(os.environ, **SAN_ENV, LD_PRELOAD=libasan, BG_ORACLE_LIB=os.path.join(ROOT, "oracle", "libbg_oracle_asan.so"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sanitize", "oracle_driver.py")], env=env, capture_output=True,
                       text=True, timeout=900)
    _clean(r)
    assert r.stdout.strip().endswith("OK")


def test_library_host_code_under_asan_ubsan(tmp_path):
    """bgamd_td_stream_schedule is the library's one piece of host-only logic (csrc/bg_schedule.h, plain C++): compiled with the
    sanitizers and driven over 300 random rounds (ragged lengths, empty lanes, more slots than games, invalid arguments)."""
    _need("g++")
    exe = tmp_path / "schedule_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "backgammon-engine_amd", "csrc"),
                           os.path.join(ROOT, "tests", "sanitize", "schedule_driver.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=300)
    _clean(r)
    assert r.stdout.startswith("OK")


def test_learner_step_plan_under_asan_ubsan(tmp_path):
    """The learner's step plan, trace scale and environment parser (csrc/bg_td_plan.h, plain C++) compiled with the sanitizers into
    tests/sanitize/td_plan_driver.cpp and run over the sweep of tests/test_td_plan_cpu.py: every tuning, both builds' parsers, three CU
    counts, every step size at which a route can change; what the plans SAY is that module's business."""
    import test_td_plan_cpu as P
    exe = P.build_driver(tmp_path / "td_plan_driver", ("-fsanitize=address,undefined", "-fno-omit-frame-pointer"))
    for env in P.tunings():
        for experimental in (False, True):
            assert len(P.run(exe, ["tuning", int(experimental)], env, extra_env=SAN_ENV)) == 15
            for n_cu in P.N_CUS:
                sizes = P.step_sizes(n_cu)
                pairs = "".join("%d %d\n" % (t, n) for t in P.STEPS for n in sizes)
                assert len(P.run(exe, ["plan", int(experimental), n_cu], env, pairs, SAN_ENV)) == 3 * len(sizes)
                assert len(P.run(exe, ["delay", int(experimental), n_cu], env, "".join("%d\n" % n for n in sizes), SAN_ENV)) == len(sizes)
    for lam in ("0", "0.25", "0.699999988", "1", "1.5"):
        for lazy in ({}, {"BGAMD_TD_LAZY": "0"}):
            assert len(P.run(exe, ["scale", lam, 400], lazy, extra_env=SAN_ENV)) == 400


def test_device_memory_owner_under_asan_ubsan(tmp_path):
    """The owner of a handle's device memory (csrc/bg_devmem.h, plain C++) compiled with the sanitizers into
    tests/sanitize/devmem_driver.cpp and run over every failure point of tests/test_devmem_cpu.py's sequences.  A leak is a block the
    fake backend still counts as live after release_all, not LeakSanitizer's business."""
    import test_devmem_cpu as D
    exe = D.build_driver(tmp_path / "devmem_driver", ("-fsanitize=address,undefined", "-fno-omit-frame-pointer"))
    assert D.run(exe, SAN_ENV) == ["OK", str(D.CASES)]
