"""Deleting points on the device against what it replaces (DESIGN.md "Deleting points").  One process, one session:

  build     1M x 128 fp16 Vamana graph, R = 64, L = 128, alpha 1.15, two passes -- bench.py's flagship index
  delete    a seeded 1 %, 5 % and 20 % of the points (never vertex 0), each in ONE pann_vamana_delete_batch call on the
            full graph (restored from a host copy before every call): the two phase times, |A|, candidates per owner
  rebuild   pann_vamana_build over the survivors alone on a handle of their own (upload not counted)

Every figure is the median of --repeats calls after one call that is not counted (it grows the handle's scratch); the
smallest and largest are printed with it.  Wall clock around calls that return after the stream has drained.

Every step has a time limit, but it is a Python alarm: it ends a step that is slow, not one that hangs inside a native
call.  Run the tool under `timeout -k 10 <seconds>` so that a hang ends the process too.

    python tools/delete_time.py [--n 1000000] [--d 128] [--repeats 3] [--fractions 0.01,0.05,0.2] [--json out.json]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parlayann_amd import DeviceIndex, datasets  # noqa: E402

R, L, ALPHA, PASSES = 64, 128, 1.15, 2


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


def med(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fractions", default="0.01,0.05,0.2")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.n
    with step("data", 300):
        X = datasets.sift1m_like(n, a.d, seed=1234, dtype=np.float32).astype(np.float16)
    with step(f"upload + build R={R} L={L} x{PASSES}", 900):
        ix = DeviceIndex(X, max_degree=R)
        t0 = time.perf_counter()
        ix.vamana_build(R, L, ALPHA, num_passes=PASSES, seed=1, sort_neighbors=True)
        full_build_s = time.perf_counter() - t0
        G = ix.get_graph()
    print(f"  full build {full_build_s:.3f} s", flush=True)
    rows = []
    for frac in (float(f) for f in a.fractions.split(",")):
        m = int(round(frac * n))
        D = (1 + np.random.default_rng(int(frac * 1000)).choice(n - 1, m, replace=False)).astype(np.uint32)
        with step(f"delete {frac:.0%}", 900):
            runs = []
            for _ in range(a.repeats + 1):
                ix.set_graph(G)
                t0 = time.perf_counter()
                st = ix.vamana_delete_batch(D, R, ALPHA)
                st["wall_s"] = time.perf_counter() - t0
                runs.append(st)
            runs = runs[1:]
        live = np.setdiff1d(np.arange(n, dtype=np.uint32), D)
        with step(f"rebuild over the {len(live)} survivors", 900):
            sub = DeviceIndex(X[live], max_degree=R)
            ts = []
            for _ in range(a.repeats + 1):
                sub.clear_graph()
                t0 = time.perf_counter()
                sub.vamana_build(R, L, ALPHA, num_passes=PASSES, seed=1, sort_neighbors=True)
                ts.append(time.perf_counter() - t0)
            sub.close()
        st = runs[0]
        row = dict(fraction=frac, deleted=st["deleted"], affected=st["affected"], candidates=st["candidates"],
                   cand_per_owner=st["candidates"] / max(1, st["affected"]), prune_dist_cmps=st["prune_dist_cmps"],
                   expand_s=med([r["t_expand_s"] for r in runs]), prune_s=med([r["t_prune_s"] for r in runs]),
                   wall_s=med([r["wall_s"] for r in runs]), rebuild_s=med(ts[1:]))
        rows.append(row)
        print(f"  delete {frac:5.0%}: |D| {row['deleted']:7d}  |A| {row['affected']:7d}  candidates/owner {row['cand_per_owner']:7.1f}  "
              f"expand {row['expand_s'][0]:.3f} s  prune {row['prune_s'][0]:.3f} s  call {row['wall_s'][0]:.3f} s "
              f"(min {row['wall_s'][1]:.3f}, max {row['wall_s'][2]:.3f})  |  rebuild of the survivors {row['rebuild_s'][0]:.3f} s "
              f"(min {row['rebuild_s'][1]:.3f}, max {row['rebuild_s'][2]:.3f})", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(n=n, d=a.d, R=R, L=L, alpha=ALPHA, passes=PASSES, repeats=a.repeats, full_build_s=full_build_s, rows=rows), f, indent=1)
    ix.close()


if __name__ == "__main__":
    main()
