#!/usr/bin/env python3
"""Host-inclusive time of the host-pointer calls that moved onto HostTrip (csrc/api.hip), and the pinned memory the handle
holds afterwards.  Two legs, both outside bench.py and never its `value`:

  hcnng   the C++ host mirror's HCNNG build (host/HCNNG/neighbors -host_tree): one pann_pivot_split per level and one
          pann_leaf_knn_batch per tree over ALL points -- the largest arrays any host-pointer call moves.
  calls   pann_bruteforce_knn (10 000 x n fp16, k = 100), pann_rerank and pann_range_query on the benchmark table, and one
          pann_leaf_knn_batch over all its points, after which "pinned_bytes" is read.

--libdir DIR takes libpann.so from DIR (another build of the library) for both legs: A/B runs alternate it."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--libdir", default=None)
ap.add_argument("--leg", default="both", choices=["both", "hcnng", "calls"])
ap.add_argument("--hcnng-n", type=int, default=2_000_000)
ap.add_argument("--hcnng-d", type=int, default=32)
ap.add_argument("--trees", type=int, default=8)
ap.add_argument("--seed", type=int, default=3)
ap.add_argument("--n", type=int, default=1_000_000)
args = ap.parse_args()
if args.libdir:
    os.environ["PANN_LIBRARY"] = os.path.join(os.path.abspath(args.libdir), "libpann.so")
    os.environ["LD_LIBRARY_PATH"] = os.path.abspath(args.libdir) + os.pathsep + os.environ.get("LD_LIBRARY_PATH", "")

import numpy as np  # noqa: E402
from parlayann_amd import DeviceIndex, datasets, io  # noqa: E402

tag = args.libdir or "in-tree"

if args.leg in ("both", "hcnng"):
    exe = os.path.join(ROOT, "parlayann_amd", "host", "HCNNG", "neighbors")
    with tempfile.TemporaryDirectory() as d:
        io.write_bin(os.path.join(d, "base.bin"), datasets.sift_like(args.hcnng_n, args.hcnng_d, seed=1234, dtype=np.uint8))
        t0 = time.perf_counter()
        r = subprocess.run([exe, "-base_path", os.path.join(d, "base.bin"), "-data_type", "uint8", "-dist_func", "Euclidian",
                            "-num_clusters", str(args.trees), "-cluster_size", "1000", "-mst_deg", "3", "-seed", str(args.seed),
                            "-host_tree"], capture_output=True, text=True)
        wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit(f"neighbors failed ({r.returncode}): " + r.stdout[-1000:] + r.stderr[-1000:])
    m = re.search(r"tree time: ([0-9.e+-]+) leaf knn time: ([0-9.e+-]+) mst time: ([0-9.e+-]+)", r.stdout)
    print(f"[{tag}] hcnng host mirror n={args.hcnng_n} d={args.hcnng_d} trees={args.trees}: process {wall:.2f} s, "
          f"tree {float(m.group(1)):.2f} s, leaf knn {float(m.group(2)):.2f} s, mst {float(m.group(3)):.2f} s", flush=True)

if args.leg in ("both", "calls"):
    X = datasets.sift1m_like(args.n, 128, seed=1234, dtype=np.float16)
    Q = datasets.sift1m_like(10_000, 128, seed=4321, dtype=np.float16)
    ix = DeviceIndex(X, max_degree=64)
    ix.vamana_build(64, 128, 1.15, num_passes=2, seed=1)

    def best(fn, reps=4):
        t = []
        for _ in range(reps):
            t0 = time.perf_counter(); out = fn(); t.append(time.perf_counter() - t0)
        return min(t) * 1e3, t[0] * 1e3, out

    ms, first, (gt, gd) = best(lambda: ix.bruteforce_knn(Q, 100))
    print(f"[{tag}] bruteforce_knn 10000 x {args.n} f16 k=100: best {ms:.2f} ms (first call {first:.2f} ms)")
    cand = np.ascontiguousarray(gt[:, ::-1])
    ms, first, _ = best(lambda: ix.rerank(Q, cand, None, 10))
    print(f"[{tag}] rerank 10000 x 100 candidates k=10: best {ms:.2f} ms (first call {first:.2f} ms)")
    radius = float(np.median(gd[:, 20]))
    ms, first, rq = best(lambda: ix.range_query(Q, radius=radius, beam=64, max_results=1024))
    print(f"[{tag}] range_query 10000 queries beam=64 max_results=1024 ({int(rq['counts'].sum())} ids): best {ms:.2f} ms "
          f"(first call {first:.2f} ms)")
    print(f"[{tag}] pinned_bytes after the three calls: {ix.get_option('pinned_bytes')}")
    ids = np.arange(args.n, dtype=np.uint32)
    off = np.arange(0, args.n + 1, 1000, dtype=np.uint64)
    ms, first, _ = best(lambda: ix.leaf_knn_batch(ids, off, 10), reps=3)
    print(f"[{tag}] leaf_knn_batch {args.n} points in leaves of 1000, m=10: best {ms:.2f} ms (first call {first:.2f} ms)")
    print(f"[{tag}] pinned_bytes after it: {ix.get_option('pinned_bytes')}   (-1: a library without the option)")
    ix.close()
