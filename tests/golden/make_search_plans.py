#!/usr/bin/env python3
"""Recorder of tests/golden/search_plans_v1.txt: what the beam search's host plan DECIDED at commit 07f3071, the last one whose
make_plan lived inside beam_search.hip.  Run by hand from a git checkout that has that commit; no test runs it.

The recorder never looks at the working tree's code.  It takes beam_search.hip, pann_internal.h and include/pann.h of 07f3071
with `git show`, cuts the host arithmetic out of beam_search.hip -- from `void choose_point_layout` up to the comment in front of
`launch_search` -- wraps it in a small main and builds it with the host compiler (under ASan + UBSan; the HIP runtime header is
only needed for its types: pass --rocm if it is not under /opt/rocm).  One row per plan, integers only.  Rows with a non-default
A/B switch come from a -DPANN_AB build of the same text, run with the variable set in that process's environment.

The combination filter + masked is not recorded: launch_beam_search refuses it before it plans.
usage: tests/golden/make_search_plans.py [--rocm DIR] [--out FILE]"""
import argparse
import os
import random
import subprocess
import sys
import tempfile

PARENT = "07f3071"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

IN_COLS = ["dtype", "metric", "dbytes", "max_deg", "n", "codes", "b64_seen", "sk_stride", "nq", "nstarts", "k", "beam",
           "degree_limit", "cut_sign", "dcap", "filter", "masked"]
SW_COLS = ["sw_b128_lds", "sw_b128_split", "sw_b128_no24", "sw_b64_seen", "sw_force_lpc"]      # defaults: 0 1 0 -1 0
OUT_COLS = ["choice", "bits", "bcap", "ccap", "deg_eff", "dcap_out", "lds_bytes", "hash_lds", "slots", "hsplit", "p24", "sk_lds_off",
            "rl_off", "seen_n", "ws_bytes", "lpc", "nch"]
SW_DEFAULT = (0, 1, 0, -1, 0)
CHOICES = ["sketch filter", "masked b64", "masked generic", "b64 with V", "b64 without V", "b128 codes", "b128 table in HBM",
           "b128 table in LDS", "generic table in LDS", "generic table in HBM"]

MAIN = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include "parlayann_amd/csrc/pann_internal.h"
#define PANN_WAVE 64
namespace pann {
enum { B64_SEEN = 3 };
#include "cut.inc"
}
using namespace pann;
int main() {
  static uint16_t codes[1];
  long long v[17];
  for (;;) {
    for (int i = 0; i < 17; i++) if (scanf("%lld", &v[i]) != 1) return i == 0 ? 0 : 1;
    DeviceIndex ix;
    ix.dtype = (int)v[0]; ix.metric = (int)v[1]; ix.dbytes = (uint32_t)v[2]; ix.max_deg = (uint32_t)v[3];
    ix.gstride = (ix.max_deg + 15) / 16 * 16; ix.n = (uint64_t)v[4];
    if (v[5]) { ix.codes_valid = 1; ix.gcode = codes; ix.rank16 = codes; }
    ix.b64_seen = (uint32_t)v[6]; ix.sk_stride = (uint32_t)v[7];
    choose_point_layout(ix.dbytes, &ix.lpc, &ix.nch);
    SearchArgs a{};
    a.nq = (uint64_t)v[8]; a.nstarts = (uint32_t)v[9]; a.k = v[10]; a.beam = v[11]; a.limit = a.beam; a.degree_limit = v[12];
    a.cut = 1.35 * (double)v[13]; a.dcap = (uint32_t)v[14]; a.filter = (int)v[15]; a.masked = (int)v[16];
    const Plan p = make_plan(ix, a);
    const int choice = p.filter ? 0 : p.masked ? (p.b64 ? 1 : 2) : p.b64 ? (p.seen_n ? 3 : 4) : p.b128_codes ? 5
                     : p.b128 ? (p.b128_hbm ? 6 : 7) : p.hash_lds ? 8 : 9;      // launch_variant's chain
    printf("%d %u %u %u %u %u %u %d %u %u %u %u %u %u %llu %u %u\n", choice, p.bits, p.bcap, p.ccap, p.deg_eff, p.dcap, p.lds_bytes,
           (int)p.hash_lds, p.slots, p.b128_hbm ? p.hsplit : 0u, p.b128_hbm ? p.p24 : 0u,      // what BSParams gets of the two
           p.sk_lds_off, p.rl_off, p.seen_n, (unsigned long long)search_workspace_bytes(ix, a), ix.lpc, ix.nch);
  }
}
"""


def git_show(path):
    return subprocess.run(["git", "-C", ROOT, "show", f"{PARENT}:{path}"], capture_output=True, text=True, check=True).stdout


def build(td, rocm):
    for path in ("parlayann_amd/csrc/pann_internal.h", "include/pann.h"):
        os.makedirs(os.path.join(td, os.path.dirname(path)), exist_ok=True)
        open(os.path.join(td, path), "w").write(git_show(path))
    src = git_show("parlayann_amd/csrc/beam_search.hip")
    a = src.index("void choose_point_layout")
    a = src.rindex("\n", 0, a) + 1
    b = src.index("using SearchKernel")
    b = src.rindex("\n\n", 0, b) + 1                       # the blank line in front of the comment before launch_search
    open(os.path.join(td, "cut.inc"), "w").write(src[a:b])
    open(os.path.join(td, "main.cpp"), "w").write(MAIN)
    exes = {}
    for name, extra in (("plain", []), ("ab", ["-DPANN_AB"])):
        exes[name] = os.path.join(td, name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{td}", "-w",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *extra, "-o", exes[name],
                               os.path.join(td, "main.cpp")])
    return exes


U8, I8, F32, F16, BF16, U4, I4 = range(7)
N24, NV = 0xFFFFFF, 0xFFFF * 512


def base(**kw):
    r = dict(dtype=U8, metric=0, dbytes=128, max_deg=64, n=1000000, codes=0, b64_seen=1, sk_stride=0, nq=10000, nstarts=1, k=10,
             beam=64, degree_limit=64, cut_sign=1, dcap=256, filter=0, masked=0)
    r.update(kw)
    return r


def grid():
    rng = random.Random(20261020)
    rows = []
    row_types = [(U8, 64), (U8, 100), (U8, 128), (I8, 256), (F16, 256), (F32, 384), (F32, 512), (F16, 768), (F32, 3072), (BF16, 64),
                 (BF16, 128), (BF16, 256), (BF16, 384), (BF16, 768), (U4, 64), (I4, 100), (F32, 128), (F16, 512)]
    beams = [1, 8, 32, 64, 65, 90, 91, 100, 128, 129, 200, 1000]
    # every row type x every beam x (plain, sketch, bitmap, labels), the other inputs drawn
    for dt, db in row_types:
        for beam in beams:
            for mode in range(4):
                rows.append(base(
                    dtype=dt, dbytes=db, metric=1 if dt == I4 else 0 if dt == U4 else rng.choice([0, 0, 1]), beam=beam,
                    filter=int(mode == 1), masked=max(mode - 1, 0), sk_stride=rng.choice([16, 32, 48]) if mode == 1 else rng.choice([0, 16]),
                    max_deg=rng.choice([16, 32, 64, 64, 80, 128]), degree_limit=rng.choice([-1, 16, 64, 64, 1000]),
                    n=rng.choice([1000, 1000000, N24 - 1, N24, N24 + 1, NV, NV + 1]), codes=rng.choice([0, 1, 1]), b64_seen=rng.choice([0, 1, 1, 1]),
                    nq=rng.choice([1, 2048, 2049, 100000]), nstarts=rng.choice([s for s in (1, 10, 64, 65, 70, 100, 128) if s <= beam]),
                    k=rng.choice([0, 10]), cut_sign=rng.choice([-1, 0, 1, 1]), dcap=rng.choice([0, 64, 256, 1000])))
    # the b128 family on both sides of each of its thresholds
    for beam in (65, 90, 91, 128, 129):
        for nq in (2048, 2049):
            for n in (N24 - 1, N24, NV + 1):
                for codes, max_deg in ((0, 64), (1, 64), (1, 80)):
                    for nstarts in (1, 64, 65):
                        rows.append(base(beam=beam, nq=nq, n=n, codes=codes, max_deg=max_deg, nstarts=nstarts, dbytes=rng.choice([100, 128, 256, 384]),
                                         dtype=rng.choice([U8, F16, BF16])))
    # the b64 family: V or not
    for beam in (10, 64):
        for n in (NV, NV + 1):
            for b64_seen in (0, 1):
                for k, metric, cut_sign in ((10, 0, 1), (10, 0, -1), (0, 0, -1), (10, 1, -1), (10, 0, 0)):
                    for masked in (0, 1, 2):
                        rows.append(base(beam=beam, n=n, b64_seen=b64_seen, k=k, metric=metric, cut_sign=cut_sign, masked=masked,
                                         dtype=rng.choice([U8, F16]), dbytes=rng.choice([64, 256, 512])))
    # generic with the table in LDS needs 65 <= nstarts <= beam <= 128; plans beyond 160 KB; tables too large for LDS
    for nstarts, beam in ((65, 65), (70, 100), (65, 128), (128, 128), (100, 129)):
        for masked in (0, 1, 2):
            rows.append(base(beam=beam, nstarts=nstarts, masked=masked, dbytes=256))
    for beam in (5000, 20000, 65536):
        for filt in (0, 1):
            rows.append(base(beam=beam, filter=filt, sk_stride=16 * filt, dbytes=3072, dtype=F32, nq=5000))
    seen, out = set(), []
    for r in rows:
        t = tuple(r[c] for c in IN_COLS)
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def switch_rows():
    """(switch tuple, rows): a few rows per non-default switch"""
    b128 = [base(beam=b, nq=2049, n=n, dbytes=db) for b in (91, 128) for n in (1000000, N24) for db in (128, 384)]
    b128 += [base(beam=65, nq=2049), base(beam=128, nq=2048)]
    b64 = [base(beam=b, b64_seen=s, masked=m) for b in (32, 64) for s in (0, 1) for m in (0, 1)]
    lpc = [base(beam=64, dbytes=db, dtype=F32) for db in (128, 384, 512, 768, 3072)]
    groups = [((0, s, 0, -1, 0), b128) for s in (0, 2, 3, 7)]
    groups += [((0, 1, 1, -1, 0), b128), ((0, 3, 1, -1, 0), b128), ((1, 1, 0, -1, 0), b128)]
    groups += [((0, 1, 0, 0, 0), b64), ((0, 1, 0, 1, 0), b64)]
    groups += [((0, 1, 0, -1, f), lpc) for f in (4, 8, 16)]
    return [(sw, [tuple(r[c] for c in IN_COLS) for r in rows]) for sw, rows in groups]


def run(exe, rows, sw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PANN_")}
    if sw[0]: env["PANN_B128_LDS"] = "1"
    if sw[1] != 1: env["PANN_B128_SPLIT"] = str(sw[1])
    if sw[2]: env["PANN_B128_NO24"] = "1"
    if sw[3] >= 0: env["PANN_B64_SEEN"] = str(sw[3])
    if sw[4]: env["PANN_FORCE_LPC"] = str(sw[4])
    text = "".join(" ".join(map(str, r)) + "\n" for r in rows)
    res = subprocess.run([exe], input=text, capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr
    outs = [tuple(int(x) for x in l.split()) for l in res.stdout.splitlines()]
    assert len(outs) == len(rows) and all(len(o) == len(OUT_COLS) for o in outs)
    return [r + tuple(sw) + o for r, o in zip(rows, outs)]


def check_coverage(table):
    """the conditions the table was asked to meet: every kernel choice, and both sides of every threshold of the plan"""
    col = {c: i for i, c in enumerate(IN_COLS + SW_COLS + OUT_COLS)}
    g = lambda r, c: r[col[c]]
    default = [r for r in table if tuple(g(r, c) for c in SW_COLS) == SW_DEFAULT]
    for ch in range(10):
        assert any(g(r, "choice") == ch for r in default), CHOICES[ch]
    nch1 = lambda r: g(r, "nch") == 1 and g(r, "lpc") != 4
    masked64 = [r for r in default if g(r, "masked") and g(r, "bcap") == 64 and g(r, "hash_lds")]
    assert any(g(r, "choice") == 2 and g(r, "lpc") == 8 and nch1(r) for r in masked64)                  # 128-byte rows
    assert any(g(r, "choice") == 2 and g(r, "dtype") == BF16 and not nch1(r) for r in masked64)         # bf16, several chunks
    assert any(g(r, "choice") == 1 for r in masked64)
    for name, values in (("beam", (64, 65, 90, 91, 128, 129)), ("nq", (2048, 2049)), ("n", (N24 - 1, N24, NV, NV + 1)), ("b64_seen", (0, 1)),
                         ("metric", (0, 1)), ("k", (0, 10)), ("cut_sign", (-1, 1)), ("dbytes", (64, 100, 128, 256, 384, 512, 768, 3072))):
        for v in values:
            assert any(g(r, name) == v for r in default), (name, v)
    b64 = [r for r in default if g(r, "choice") in (3, 4) and g(r, "b64_seen") and g(r, "n") <= NV]
    assert any(g(r, "choice") == 4 and g(r, "cut_sign") < 0 and g(r, "k") > 0 and g(r, "metric") == 0 for r in b64)
    assert any(g(r, "choice") == 3 and g(r, "cut_sign") < 0 and g(r, "k") == 0 for r in b64)
    assert any(g(r, "choice") == 3 and g(r, "cut_sign") < 0 and g(r, "metric") == 1 for r in b64)
    assert any(g(r, "codes") and g(r, "max_deg") > 64 and g(r, "bits") == 12 and g(r, "choice") in (6, 7) for r in default)
    assert any(g(r, "lds_bytes") > 160 * 1024 for r in default) and any(g(r, "p24") for r in default)
    for sw in {tuple(g(r, c) for c in SW_COLS) for r in table}:
        rows = [r for r in table if tuple(g(r, c) for c in SW_COLS) == sw]
        assert len(rows) >= 3, sw
    sw_rows = [r for r in table if tuple(g(r, c) for c in SW_COLS) != SW_DEFAULT]
    assert {g(r, "hsplit") for r in sw_rows} == {0, 1, 2, 3} and any(g(r, "sw_b128_lds") and g(r, "choice") == 7 and g(r, "nq") > 2048 for r in sw_rows)
    assert any(g(r, "sw_b64_seen") == 0 and g(r, "b64_seen") and g(r, "choice") == 4 for r in sw_rows)
    assert any(g(r, "sw_b128_no24") and g(r, "n") < N24 and g(r, "hsplit") and not g(r, "p24") for r in sw_rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rocm", default="/opt/rocm")
    ap.add_argument("--out", default=os.path.join(HERE, "search_plans_v1.txt"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        exes = build(td, args.rocm)
        table = run(exes["plain"], grid(), SW_DEFAULT)
        assert table == run(exes["ab"], grid(), SW_DEFAULT)          # a -DPANN_AB build with nothing set decides the same
        for sw, rows in switch_rows():
            table += run(exes["ab"], rows, sw)
    check_coverage(table)
    assert len(table) <= 3000, len(table)
    with open(args.out, "w") as f:
        f.write("# " + " ".join(IN_COLS + SW_COLS + OUT_COLS) + "\n")
        for r in table:
            f.write(" ".join(map(str, r)) + "\n")
    counts = [sum(1 for r in table if r[len(IN_COLS) + len(SW_COLS)] == ch) for ch in range(10)]
    print(f"{len(table)} rows, {os.path.getsize(args.out)} bytes; per choice: " + ", ".join(f"{n} {c}" for n, c in zip(counts, CHOICES)))


if __name__ == "__main__":
    sys.exit(main())
