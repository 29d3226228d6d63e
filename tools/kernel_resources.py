#!/usr/bin/env python3
"""Per-kernel register, LDS and scratch figures of a built libvfilter_hip.so, from the code
objects' metadata (no GPU): the table in profiles/lut_kernel_resources.txt.

    tools/kernel_resources.py LIB [--match REGEX] [--against OTHER_LIB]

With --against, the kernels of both libraries that match are printed side by side and the exit
status is 1 when a kernel present in both differs in any figure.  Needs llvm-readelf and
llvm-cxxfilt (ROCm's llvm/bin, or on PATH).
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def tool(name):
    for d in ("/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    p = shutil.which(name) or (shutil.which("c++filt") if name == "llvm-cxxfilt" else None)
    if not p:
        sys.exit(f"{name} not found")
    return p


def code_objects(lib):
    """The gfx950 ELF images of every offload bundle in the library (one bundle per source file)."""
    blob = open(lib, "rb").read()
    out, at = [], blob.find(MAGIC)
    while at >= 0:
        n = int.from_bytes(blob[at + 24:at + 32], "little")
        p = at + 32
        for _ in range(n):
            off, size, tl = (int.from_bytes(blob[p + 8 * i:p + 8 * i + 8], "little") for i in range(3))
            triple = blob[p + 24:p + 24 + tl]
            p += 24 + tl
            if b"gfx950" in triple and size:
                out.append(blob[at + off:at + off + size])
        at = blob.find(MAGIC, at + 1)
    return out


def kernels(lib):
    """{demangled kernel name: (vgpr, agpr, sgpr, lds bytes, scratch bytes, max workgroup)}"""
    res = {}
    for img in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(img)
            f.flush()
            notes = subprocess.run([tool("llvm-readelf"), "--notes", f.name], capture_output=True, text=True,
                                   check=True).stdout
        for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            blk = "    .agpr_count:" + blk

            def field(k, blk=blk):  # the kernel's own keys sit at four spaces (its arguments' deeper)
                m = re.search(r"^    \.%s:\s+(\S+)" % k, blk, flags=re.M)
                return m.group(1) if m else "?"
            sym = field("name")
            name = subprocess.run([tool("llvm-cxxfilt"), sym], capture_output=True, text=True).stdout.strip() or sym
            name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
            name = re.sub(r"\(.*$", "", name)
            res[name] = tuple(int(field(k)) for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
                                                      "private_segment_fixed_size", "max_flat_workgroup_size"))
    return res


def wg_per_cu(v):
    """Workgroups per CU by registers (512 VGPRs + AGPRs per SIMD lane, 8 waves per SIMD at most)
    and LDS (160 KiB), for the kernel's maximum workgroup size."""
    vgpr, agpr, _, lds, _, wg = v
    regs = max(8, (vgpr + agpr + 7) // 8 * 8)
    waves_simd = min(8, 512 // regs)
    waves_wg = (wg + 63) // 64
    by_regs = waves_simd * 4 // waves_wg
    by_lds = (160 * 1024) // lds if lds else 99
    return min(by_regs, by_lds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("--match", default=".")
    ap.add_argument("--against")
    ap.add_argument("--rename", nargs=2, metavar=("REGEX", "REPL"),
                    help="rewrite LIB's kernel names before comparing (a template that gained a defaulted parameter)")
    a = ap.parse_args()
    rx = re.compile(a.match)
    mine = kernels(a.lib)
    if a.rename:
        mine = {re.sub(a.rename[0], a.rename[1], k): v for k, v in mine.items()}
    mine = {k: v for k, v in mine.items() if rx.search(k)}
    other = {k: v for k, v in kernels(a.against).items() if rx.search(k)} if a.against else None
    hdr = "vgpr agpr sgpr   lds scratch wg/CU"
    fmt = lambda v: "%4d %4d %4d %5d %7d %5d" % (v[0], v[1], v[2], v[3], v[4], wg_per_cu(v))  # noqa: E731
    bad = 0
    if other is None:
        print(f"{hdr}  kernel")
        for k in sorted(mine):
            print(f"{fmt(mine[k])}  {k}")
        return 0
    print(f"{hdr} | {hdr}  same  kernel   (left: {a.against}, right: {a.lib})")
    for k in sorted(set(mine) | set(other)):
        l, r = other.get(k), mine.get(k)
        same = "new" if l is None else "gone" if r is None else "yes" if l == r else "NO"
        bad += same in ("NO", "gone")
        print(f"{fmt(l) if l else ' ' * len(hdr)} | {fmt(r) if r else ' ' * len(hdr)}  {same:4s}  {k}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
