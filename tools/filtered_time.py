"""Rerank-only search against sketch-filtered search (two-level search), one process.  Every step has a time
limit, but it is a Python alarm: it ends a step that is slow, not one that hangs inside a native call (the interpreter
never gets to run the handler).  Run the tool under `timeout -k 10 <seconds>` so that a hang ends the process too.

Shape 1, the reference's own regime: f32 MIPS, d >= 256, normalised, quantised to i8, Vamana R = 64; second level
Mips_2Bit_Point.  Shape 2: f32 L2, d = 128, quantised to u8; second level Euclidean_Bit_Point.  For beams 16 .. 128 it
prints QPS (host-pointer calls, staging included, best of --reps), recall@10 against the exact float neighbours, full
distances per query and algorithmic bytes per query: adjacency rows + full rows + sketch rows.  The sketch term is an
estimate from the counters the search returns: one sketch row per neighbour that passed the hash filter (pruned_cmps), which
includes the starts and the neighbours seen before the frontier filled (no sketch row is read for those) and leaves out
the one frontier-back sketch row per visit.

    python tools/filtered_time.py [--n 200000] [--nq 10000] [--json out.json]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parlayann_amd import DeviceIndex, quantize  # noqa: E402
from parlayann_amd import sketch as sk  # noqa: E402
from parlayann_amd.recall import recall_at_k  # noqa: E402

BEAMS = (16, 32, 64, 128)


class step:
    """a time limit for one step of the run: a step that is slow ends the process (see the module docstring for hangs)"""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        def on_alarm(*_):
            print(f"step '{self.name}' exceeded {self.seconds}s: stopping", flush=True)
            os._exit(124)
        signal.signal(signal.SIGALRM, on_alarm)
        signal.alarm(self.seconds)
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        signal.alarm(0)
        print(f"  [{self.name}: {time.perf_counter() - self.t0:.1f}s]", flush=True)
        return False


def best_of(fn, reps):
    best, out = 1e30, None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t)
    return best, out


def run_shape(name, metric, d, n, nq, kind, reps):
    rng = np.random.default_rng(1)
    centres = rng.standard_normal((64, d)).astype(np.float32)
    X = (centres[rng.integers(0, 64, n)] * 0.7 + rng.standard_normal((n, d))).astype(np.float32)
    Q = (centres[rng.integers(0, 64, nq)] * 0.7 + rng.standard_normal((nq, d))).astype(np.float32)
    if metric == "mips":
        X, Q = quantize.normalize_rows(X), quantize.normalize_rows(Q)
    rows = []
    with step(f"{name}: upload + build R=64", 600):
        ix = DeviceIndex(X, max_degree=64, metric=metric)
        ix.vamana_build(64, 128, 1.0 if metric == "mips" else 1.2, num_passes=1, seed=3)
    with step(f"{name}: ground truth", 300):
        gt, gd = ix.bruteforce_knn(Q, 10)
    with step(f"{name}: quantise + sketch", 300):
        qix, qp = ix.quantized("mips_i8" if metric == "mips" else "euclid_u8")
        qq = quantize.device_quantize_rows(Q, qp)
        sp = sk.sketch_params(ix, kind)
        sk.attach_sketch(qix, ix, sp)
        sq = sk.sketch_rows(Q, sp)
    row_b, sk_b = d, (sk.row_bytes(kind, d) + 15) // 16 * 16
    for beam in BEAMS:
        with step(f"{name}: beam {beam}", 300):
            kw = dict(k=10, beam=beam, out_k=beam)

            def plain():
                r = qix.batch_search(qq, **kw)
                return r, ix.rerank(Q, r["ids"], np.minimum(r["frontier_size"], 1000).astype(np.uint32), 10)

            def filt():
                r = qix.batch_search_filtered(qq, sq, **kw)
                return r, ix.rerank(Q, r["ids"], np.minimum(r["frontier_size"], 1000).astype(np.uint32), 10)

            plain(); filt()                                      # warm-up: workspace growth
            for label, fn in (("rerank-only", plain), ("filtered", filt)):
                t, (r, (ids, _)) = best_of(fn, reps)
                full = float(r["dist_cmps"].mean())
                sketch_rows = float(r["pruned_cmps"].mean()) if "pruned_cmps" in r else 0.0
                by = float(r["degree_sum"].mean()) * 4 + full * row_b + sketch_rows * sk_b
                rows.append(dict(shape=name, beam=beam, mode=label, qps=nq / t, recall10=recall_at_k(ids, gt, gd, 10),
                                 full_dists=full, bytes_per_query=by))
                print(f"  {name} beam {beam:3d} {label:11s} QPS {nq / t:10.0f}  recall@10 {rows[-1]['recall10']:.4f}  "
                      f"full dists/q {full:8.1f}  bytes/q {by:10.0f}", flush=True)
    qix.close(); ix.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = run_shape("mips-d256-i8-2bit", "mips", 256, a.n, a.nq, "mips_2bit", a.reps)
    rows += run_shape("l2-d128-u8-bit", "l2", 128, a.n, a.nq, "euclid_bit", a.reps)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
