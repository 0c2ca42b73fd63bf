#!/usr/bin/env python3
"""wall time of the exact range ground truth (pann_bruteforce_range, host pointers in and out) next to the brute-force kNN
(k = 10) of the same data in the same process.  The radius is the median distance of the rank-th neighbour.
usage: range_gt_time.py [n=1000000] [nq=10000] [dtype=f16|bf16|u8|f32] [rank=100]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parlayann_amd import DeviceIndex, bfloat16, datasets  # noqa: E402

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
