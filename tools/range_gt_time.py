#!/usr/bin/env python3
"""wall time of the exact range ground truth (pann_bruteforce_range, host pointers in and out) next to the brute-force kNN
(k = 10) of the same data in the same process.  The radius is the median distance of the rank-th neighbour.
usage: range_gt_time.py [n=1000000] [nq=10000] [dtype=f16|bf16|u8|f32] [rank=100]
       range_gt_time.py --scan [n=1000000] [nq=10000] [rank=100] [rounds=5]
--scan: the quantised range scan (DeviceIndex.scan_range, pann_scan_range) on the one-byte and the four-bit copy of the f32 table
beside bruteforce_range on the f32 handle, same table, same radius, one process: after a warm-up of every call at the full shape the
routes are run in turn, `rounds` times over (median and min - max of the host-inclusive wall times; every call ends in a device
synchronise), at slack 0 and two wider values; with each, range recall against the exact answer ((query, id) pairs found / pairs)
and cand_total / matches."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parlayann_amd import DeviceIndex, bfloat16, datasets  # noqa: E402



def scan_leg(argv):
    n, nq, rank, rounds = (int(argv[i]) if len(argv) > i else v for i, v in enumerate((1_000_000, 10_000, 100, 5)))
    X = datasets.sift1m_like(n, 128, seed=1234, dtype=np.float32)
    Q = datasets.sift1m_like(nq, 128, seed=4321, dtype=np.float32)
    full = DeviceIndex(X, max_degree=8)
    radius = float(np.median(full.bruteforce_knn(Q, rank)[1][:, rank - 1]))
    copies = {kind: full.quantized(kind, copy_graph=False) for kind in ("euclid_u8", "euclid_u4")}
    routes = {"bruteforce_range f32": lambda: full.bruteforce_range(Q, radius)}
    for kind, (quant, p) in copies.items():
        for slack in (0.0, 0.1, 0.3):
            routes[f"scan_range {kind} slack {slack}"] = lambda quant=quant, p=p, slack=slack: full.scan_range(quant, p, Q, radius, slack=slack)
    times, out = {k: [] for k in routes}, {}
    for name, f in routes.items():                      # warm-up: every shape the timed window uses
        out[name] = f()
    for _ in range(rounds):                             # the routes in turn, so that what else the host does falls on all of them
        for name, f in routes.items():
            t0 = time.perf_counter(); f(); times[name].append(time.perf_counter() - t0)
    off, ids = out["bruteforce_range f32"]
    matches = int(off[-1])
    keys = lambda o, i: np.repeat(np.arange(nq, dtype=np.uint64), np.diff(o).astype(np.int64)) * np.uint64(n) + i   # (query, id) pairs
    exact = keys(off, ids)
    print(f"{nq} x {n} x 128 f32, radius {radius:.6g} (median rank-{rank} distance), {matches} matches; host-inclusive wall time of "
          f"count call + fill call, median [min - max] of {rounds} alternating rounds")
    for name, ts in times.items():
        line = f"{name:34s} {np.median(ts) * 1e3:8.1f} ms [{min(ts) * 1e3:.1f} - {max(ts) * 1e3:.1f}]"
        if name in out and isinstance(out[name], dict):
            r = out[name]
            found = np.intersect1d(keys(r["offsets"], r["ids"]), exact, assume_unique=True).size
            line += (f"  recall {found / max(matches, 1):.4f}  returned {len(r['ids'])}"
                     f"  cand_total / matches {r['cand_total'] / max(matches, 1):.2f}")
        print(line)


if sys.argv[1:2] == ["--scan"]:
    scan_leg(sys.argv[2:])
    sys.exit(0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
nq = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000
name = sys.argv[3] if len(sys.argv) > 3 else "f16"
dt = {"f16": np.float16, "bf16": bfloat16, "u8": np.uint8, "f32": np.float32}[name]
rank = int(sys.argv[4]) if len(sys.argv) > 4 else 100
X = datasets.sift1m_like(n, 128, seed=1234, dtype=dt)
Q = datasets.sift1m_like(nq, 128, seed=4321, dtype=dt)
ix = DeviceIndex(X, max_degree=8)
if os.environ.get("GT_PIECES"):
    ix.set_option("gt_pieces", int(os.environ["GT_PIECES"]))
gi, gd = ix.bruteforce_knn(Q, rank)
radius = float(np.median(gd[:, rank - 1]))
ix.bruteforce_range(Q[:256], radius)
ix.bruteforce_knn(Q[:256], 10)


def best_of_3(f):
    best, out = 1e9, None
    for _ in range(3):
        t0 = time.perf_counter(); out = f(); best = min(best, time.perf_counter() - t0)
    return best, out


t_range, (off, ids) = best_of_3(lambda: ix.bruteforce_range(Q, radius))
t_count, _ = best_of_3(lambda: ix._lib.pann_bruteforce_range(ix.handle, Q.ctypes.data, nq, Q.shape[1] * Q.itemsize, radius,
                                                             off.ctypes.data, None, 0))
t_knn, (ki, kd) = best_of_3(lambda: ix.bruteforce_knn(Q, 10))
print(f"bruteforce_range {nq} x {n} {name} radius {radius:.6g} (median rank-{rank} distance): {t_range * 1e3:.1f} ms "
      f"(host-inclusive, best of 3; count call + fill call), count call alone {t_count * 1e3:.1f} ms; {int(off[-1])} matches, "
      f"checksum {int(ids.astype(np.uint64).sum())}")
print(f"bruteforce_knn   {nq} x {n} {name} k=10: {t_knn * 1e3:.1f} ms (host-inclusive, best of 3); ratio {t_range / t_knn:.2f}")
