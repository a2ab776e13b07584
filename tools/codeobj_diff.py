#!/usr/bin/env python3
"""Do two builds of the library carry the same gfx950 device code?   tools/codeobj_diff.py OLD.so NEW.so [INDEX]

Where a kernel lies in the code object costs about 1 % of the greedy step, so a change that is meant to leave the device
code alone is checked for exactly that: the .hip_fatbin section of each library is dumped (llvm-objcopy), its gfx950 code object
unbundled (clang-offload-bundler), and the two objects compared -- the bytes of .text, .rodata and .note, and the address and size of
every function symbol.  The one difference allowed is the object symbol __hip_cuid_<hash>: its name is a digest of the source.
INDEX (default 0) picks the translation unit: the library's .hip_fatbin holds one bundle per .hip file in link order (0 bgamd.hip,
1 bgamd_search3.hip, 2 bgamd_cube.hip).
Bytes and symbol tables only: nothing is disassembled.  Exit status 0 = identical, 1 = different, 2 = could not compare."""
import os
import shutil
import struct
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
SECTIONS = (".text", ".rodata", ".note")
TOOLS = ("llvm-objcopy", "clang-offload-bundler")


def find_tool(name):
    """the tool on PATH or in a ROCm tree's LLVM directory, else None"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    return shutil.which(name) or shutil.which(name, path=os.pathsep.join(os.path.join(rocm, d) for d in ("llvm/bin", "lib/llvm/bin")))


MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_object(lib, workdir, tag, index=0):
    """-> the bytes of the gfx950 code object of lib's index-th bundle"""
    fatbin, obj = os.path.join(workdir, tag + ".fatbin"), os.path.join(workdir, tag + ".o")
    subprocess.check_call([find_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fatbin, lib, os.devnull])
    if index:
        with open(fatbin, "rb") as f:
            blob = f.read()
        starts = [i for i in range(len(blob)) if blob.startswith(MAGIC, i)]
        if index >= len(starts):
            raise OSError("the library holds %d bundles" % len(starts))
        with open(fatbin, "wb") as f:
            f.write(blob[starts[index]:starts[index + 1] if index + 1 < len(starts) else len(blob)])
    subprocess.check_call([find_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fatbin,
                           "--output=" + obj])
    with open(obj, "rb") as f:
        return f.read()


def parse(elf):
    """ELF64 little-endian -> ({section name: (address, bytes)}, {symbol name: (type, address, size)})"""
    assert elf[:6] == b"\x7fELF\x02\x01", "not a 64-bit little-endian ELF"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    heads = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]     # name type flags addr off size link info align entsize

    def text(table, at):
        start = heads[table][4] + at
        return elf[start:elf.index(b"\0", start)].decode()

    body = lambda h: b"" if h[1] == 8 else elf[h[4]:h[4] + h[5]]          # (SHT_NOBITS has no bytes in the file)
    sections = {text(shstrndx, h[0]): (h[3], body(h)) for h in heads}
    symbols = {}
    for h in heads:
        if h[1] != 2:                                                     # SHT_SYMTAB
            continue
        for at in range(h[4], h[4] + h[5], 24):
            name, info, _other, _shndx, value, size = struct.unpack_from("<IBBHQQ", elf, at)
            if name:
                symbols[text(h[6], name)] = (info & 15, value, size)
    return sections, symbols


def compare(old, new, out=print):
    """report on two code objects -> the number of differences"""
    (osec, osym), (nsec, nsym) = parse(old), parse(new)
    bad = 0
    for name in SECTIONS:
        o, n = osec.get(name), nsec.get(name)
        same = o is not None and o == n
        bad += not same
        out("%-8s %s" % (name, "identical: 0x%x bytes at 0x%x" % (len(o[1]), o[0]) if same else
                         "DIFFERS: %s" % " vs ".join("absent" if x is None else "0x%x bytes at 0x%x" % (len(x[1]), x[0]) for x in (o, n))))
    differ = sorted(k for k in osym.keys() | nsym.keys() if osym.get(k) != nsym.get(k))
    cuid = [k for k in differ if k.startswith("__hip_cuid_")]
    is_function = lambda k: 2 in (s[k][0] for s in (osym, nsym) if k in s)                  # STT_FUNC
    show = lambda k: " vs ".join("absent" if k not in s else "0x%x + 0x%x" % s[k][1:] for s in (osym, nsym))
    for what, names in (("function", [k for k in differ if is_function(k)]),
                        ("other", [k for k in differ if not is_function(k) and k not in cuid])):
        count = ["%d" % sum(1 for v in s.values() if (v[0] == 2) == (what == "function")) for s in (osym, nsym)]
        out("%s symbols %s, %s" % (what, " vs ".join(count), "all at the same address and size" if not names else "%d DIFFER:" % len(names)))
        for k in names:
            out("  %s: %s" % (k, show(k)))
        bad += len(names)
    if cuid:
        out("allowed to differ: " + " / ".join(cuid))
    out("identical" if not bad else "DIFFERENT (%d)" % bad)
    return bad


def main(argv):
    if len(argv) not in (3, 4):
        print(__doc__, file=sys.stderr)
        return 2
    missing = [t for t in TOOLS if not find_tool(t)]
    if missing:
        print("not found: " + ", ".join(missing), file=sys.stderr)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        try:
            index = int(argv[3]) if len(argv) == 4 else 0
            old, new = code_object(argv[1], tmp, "old", index), code_object(argv[2], tmp, "new", index)
        except (OSError, subprocess.CalledProcessError) as e:
            print("could not extract a gfx950 code object: %s" % e, file=sys.stderr)
            return 2
    return 1 if compare(old, new) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
