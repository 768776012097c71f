#!/usr/bin/env python3
"""Print `unit, kernel, bytes, sha256` for every kernel of the scan units' device code.

Each of the nine scan sources is compiled device-only for gfx950, and the seven that hold a pattern kernel a second time
with -DCRYO_LIKE_UNIT (the Makefile's LIKE_SRCS).  For every kernel symbol of a code object the bytes of its function in
.text and its 64-byte kernel descriptor (<kernel>.kd) are cut out of their sections and hashed together.  Two trees whose
outputs do not differ run the same device code: that is how a change of host code alone (the launch layer) is shown to have
left the kernels as they were.

    python tools/scan_kernel_text.py [--tree DIR] [--keep DIR] [--objects] > profiles/NAME.txt

--objects adds a line per unit that hashes the whole code object.  That hash depends on where the tree lies: the compiler
names a symbol of every code object (__hip_cuid_...) after a hash of the source's real path and its command line.  Whole
objects therefore compare only between two builds at one and the same path (the first tree moved away, the second put in its
place); then they also tell whether the kernels are laid out in the same order.

No instruction is looked at and nothing runs on a GPU.
"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

SCAN_SRCS = ["filter", "agg", "agg_float", "group", "group_float", "group_bucket", "group_text", "project", "topn"]
LIKE_SRCS = ["filter", "agg_float", "group_float", "group_bucket", "group_text", "project", "topn"]
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.environ.get("HIPCC", os.path.join(ROCM, "bin", "hipcc"))
READELF = os.path.join(ROCM, "llvm", "bin", "llvm-readelf")


def sections(obj):
    """{index: (name, file offset, address)} of a code object"""
    out = {}
    for line in subprocess.check_output([READELF, "-S", "-W", obj], text=True).splitlines():
        line = line.strip()
        if not line.startswith("["):
            continue
        idx, rest = line[1:].split("]", 1)
        f = rest.split()
        if not idx.strip().isdigit() or len(f) < 5 or f[0] == "NULL":
            continue
        out[int(idx)] = (f[0], int(f[3], 16), int(f[2], 16))
    return out


def symbols(obj):
    """{name: (value, size, type, section index)} of a code object"""
    out = {}
    for line in subprocess.check_output([READELF, "-s", "-W", obj], text=True).splitlines():
        f = line.split()
        if len(f) != 8 or not f[0].endswith(":") or not f[0][:-1].isdigit() or not f[6].isdigit():
            continue
        out[f[7]] = (int(f[1], 16), int(f[2]), f[3], int(f[6]))
    return out


def cut(data, secs, sym):
    value, size, _, shndx = sym
    _, off, addr = secs[shndx]
    return data[off + value - addr: off + value - addr + size]


BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def unbundle(obj):
    """the compiler wraps the device-only output in an offload bundle: leave the gfx950 code object alone in the file"""
    data = open(obj, "rb").read()
    if not data.startswith(BUNDLE_MAGIC):
        return
    at = len(BUNDLE_MAGIC)
    n = int.from_bytes(data[at:at + 8], "little")
    at += 8
    for _ in range(n):
        off, size, tlen = (int.from_bytes(data[at + 8 * k:at + 8 * k + 8], "little") for k in range(3))
        triple = data[at + 24:at + 24 + tlen].decode()
        at += 24 + tlen
        if triple.startswith("hip") and triple.endswith("gfx950"):
            open(obj, "wb").write(data[off:off + size])
            return
    raise SystemExit(f"{obj}: no gfx950 code object in the bundle")


def unit_lines(unit, obj, whole):
    unbundle(obj)
    data = open(obj, "rb").read()
    secs, syms = sections(obj), symbols(obj)
    lines = []
    for name in sorted(n[:-3] for n in syms if n.endswith(".kd")):
        fn, kd = syms[name], syms[name + ".kd"]
        if fn[2] != "FUNC" or secs[fn[3]][0] != ".text" or kd[1] != 64:
            raise SystemExit(f"{unit}: {name}: not a kernel in .text with a 64-byte descriptor")
        text = cut(data, secs, fn)
        h = hashlib.sha256(text + cut(data, secs, kd)).hexdigest()
        lines.append(f"{unit}, {name}, {len(text)}, {h}")
    if whole:
        lines.append(f"{unit}, (code object), {len(data)}, {hashlib.sha256(data).hexdigest()}")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."),
                    help="root of the source tree (default: this one)")
    ap.add_argument("--keep", default=None, help="keep the code objects in this directory")
    ap.add_argument("--objects", action="store_true", help="a line per unit that hashes the whole code object as well")
    a = ap.parse_args()
    csrc = os.path.join(a.tree, "pg_cryogen_amd", "csrc")
    inc = os.path.join(a.tree, "include")
    with tempfile.TemporaryDirectory() as tmp:
        out = a.keep or tmp
        os.makedirs(out, exist_ok=True)
        units = [(s, []) for s in SCAN_SRCS] + [(s + "_like", ["-DCRYO_LIKE_UNIT"]) for s in LIKE_SRCS]
        procs = []
        for unit, defs in units:
            src = unit[:-5] if defs else unit
            obj = os.path.join(out, unit + ".co")
            cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + inc, "--cuda-device-only", *defs, "-c",
                   os.path.join(csrc, src + ".hip"), "-o", obj]
            procs.append((unit, obj, subprocess.Popen(cmd, stderr=subprocess.PIPE, text=True)))
        kernels = 0
        for unit, obj, p in procs:
            _, err = p.communicate()
            if p.returncode != 0:
                sys.stderr.write(err)
                raise SystemExit(f"{unit}: the compiler failed")
            lines = unit_lines(unit, obj, a.objects)
            kernels += len(lines) - (1 if a.objects else 0)
            print("\n".join(lines))
        print(f"# {len(units)} units, {kernels} kernels")


if __name__ == "__main__":
    main()
