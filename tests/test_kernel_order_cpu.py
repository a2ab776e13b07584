"""The order of the kernels in the default build's gfx950 code object is the one recorded in tests/kernel_order.txt (where a
kernel lies decides ~1 % of the greedy step).  Names only -- editing a kernel changes sizes and addresses, and may.  A pull request
that adds a kernel appends its line; one that shuffles kernels fails here, before anyone benchmarks it."""
import os
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
try:
    import codeobj_diff
finally:
    sys.path.pop(0)


def test_kernels_lie_in_the_recorded_order():
    if any(codeobj_diff.find_tool(t) is None for t in codeobj_diff.TOOLS):
        pytest.skip("llvm-objcopy / clang-offload-bundler not installed")
    lib = os.path.join(ROOT, "backgammon-engine_amd", "libbgamd.so")
    assert os.path.exists(lib), "libbgamd.so is not built"
    with tempfile.TemporaryDirectory() as tmp:
        _sections, symbols = codeobj_diff.parse(codeobj_diff.code_object(lib, tmp, "lib"))
    built = [name for _address, name in sorted((v[1], k) for k, v in symbols.items() if v[0] == 2)]      # STT_FUNC, by address
    with open(os.path.join(ROOT, "tests", "kernel_order.txt")) as f:
        recorded = f.read().split()
    assert built == recorded, "first difference at entry %d" % next((i for i, (a, b) in enumerate(zip(built, recorded)) if a != b), min(len(built), len(recorded)))
