#!/usr/bin/env python3
"""Refactoring guard: are the gfx950 kernels of two builds the same machine code?  For one object of two build directories
(default beam_search.o) the code objects are unbundled (check_kernel_regs.unbundle), disassembled, and compared kernel by
kernel: the instruction text with the addresses stripped, and the metadata note (registers, scratch, spills, LDS, kernarg size).
It only compares two listings; it knows nothing about particular instructions.
usage: tools/compare_kernels.py [--diff N] BUILD_DIR_A BUILD_DIR_B [object ...]; exit status 1 on any difference
--diff N also prints the first N lines of a unified diff of every kernel whose code differs"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

from check_kernel_regs import LLVM, unbundle

META = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
        "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size")


def listing(obj):
    """(symbols, {symbol: [instruction lines]}, {kernel: metadata dict}) of the gfx950 code object inside obj"""
    with tempfile.TemporaryDirectory() as td:
        co = unbundle(obj, td)
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
        syms = subprocess.run([f"{LLVM}/llvm-readelf", "--symbols", "--wide", co], capture_output=True, text=True, check=True).stdout
    code, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = code.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            # "  s_load_dword ... // 000000001234: " -> drop the address comment; branch targets are symbol-relative already
            cur.append(re.sub(r"\s*//\s*[0-9A-Fa-f]+:.*$", "", line).strip())
    meta = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            meta[name.group(1)] = {k: (re.search(rf"\.{k}:\s+(\S+)", blk) or [None, None])[1] for k in META}
    names = sorted(f[7] for f in (l.split() for l in syms.splitlines()) if len(f) == 8 and f[0].rstrip(":").isdigit())
    return names, code, meta


def compare(a, b, ndiff=0):
    sa, ca, ma = listing(a)
    sb, cb, mb = listing(b)
    print(f"{os.path.basename(a)}: {len(sa)} symbols / {len(ma)} kernels in A, {len(sb)} symbols / {len(mb)} kernels in B")
    only_a, only_b = sorted(set(ma) - set(mb)), sorted(set(mb) - set(ma))
    for k in only_a: print(f"ONLY IN A   {k}")
    for k in only_b: print(f"ONLY IN B   {k}")
    same = diff = 0
    for k in sorted(set(ma) & set(mb)):
        what = []
        if ca.get(k) != cb.get(k):
            what.append(f"code {len(ca.get(k, []))} -> {len(cb.get(k, []))} instructions")
        if ma[k] != mb[k]:
            what.append("metadata " + ", ".join(f"{f} {ma[k][f]} -> {mb[k][f]}" for f in META if ma[k][f] != mb[k][f]))
        if what:
            diff += 1
            print(f"DIFFERENT   {k}: " + "; ".join(what))
            if ndiff and ca.get(k) != cb.get(k):
                for line in list(difflib.unified_diff(ca.get(k, []), cb.get(k, []), "A", "B", n=2, lineterm=""))[:ndiff]:
                    print("    " + line)
        else:
            same += 1
    print(f"compare_kernels: {same} identical, {diff} different, {len(only_a)} only in A, {len(only_b)} only in B")
    return diff + len(only_a) + len(only_b)


def main():
    args = sys.argv[1:]
    ndiff = 0
    if args[:1] == ["--diff"] and len(args) >= 2:
        ndiff, args = int(args[1]), args[2:]
    if len(args) < 2:
        print(__doc__)
        return 2
    objs = args[2:] or ["beam_search.o"]
    bad = sum(compare(os.path.join(args[0], o), os.path.join(args[1], o), ndiff) for o in objs)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
