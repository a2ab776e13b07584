"""The owner of a handle's device memory (csrc/bg_devmem.h) without a GPU: the header, compiled into tests/sanitize/devmem_driver.cpp
over a fake backend that counts live blocks, aborts on a bad free and fails the k-th allocation, walked through sequences shaped like
the library's (the driver's head says what it holds each of them to)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# Allocations per sequence: 40 singles; a first-use group of 11; grows: one, two and one buffer(s) that grow 4 times and five that grow
# twice = 26; a pinned block and a device block = 2; all of them in one handle's life = 79.  Each sequence runs once clean and once per
# allocation with that allocation failing.
CASES = sum(n + 1 for n in (40, 11, 26, 2, 79))


def build_driver(out, flags=()):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "backgammon-engine_amd", "csrc"),
                           os.path.join(ROOT, "tests", "sanitize", "devmem_driver.cpp"), "-o", str(out)])
    return str(out)


def run(exe, extra_env=None):
    r = subprocess.run([exe], env=dict(os.environ, **(extra_env or {})), capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    return r.stdout.split()


def test_owner_over_a_fake_backend(tmp_path):
    """Every failure point of every sequence: failed groups all null, failed grows at cap 0 and repaired by the next call, the error
    naming the buffer, nothing live after release_all, nothing freed twice."""
    assert run(build_driver(tmp_path / "devmem_driver")) == ["OK", str(CASES)]
