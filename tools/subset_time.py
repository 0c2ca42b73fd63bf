"""A subset index made on the device against the only route there was before it (DESIGN.md "Subset index").  One process, one
session:

  source    1M x 128 fp16 points, max_deg 64, one label per point, on the device.  The graph is random (full rows of 64 distinct
            ids): what the kernels move does not depend on what the edges are, and random ids are the worst case for the one
            access that does -- the 4-byte reads into the 4n-byte old_to_new table.
  subset    DeviceIndex.subset(allow, copy_graph=True) at keep fractions 1.0 / 0.5 / 0.1 / 0.01 (a seeded random bitmap; 1.0 is
            a bitmap of all ones, not the allow=None clone): the bitmap goes up, the two maps come down, the rest stays there.
  host      points() + get_graph() + labels(), select and renumber in numpy (one vectorised pass: a cumulative sum gives every
            kept neighbour its slot), DeviceIndex(points, graph) + set_labels: everything crosses the bus twice.

Both results are compared once per fraction (points, graph, labels) before anything is timed.  Every figure is the median of
--repeats calls after one call that is not counted; the smallest and largest are printed with it.  Wall clock around calls that
return after the stream has drained: host-inclusive times, not kernel times.

Every step has a time limit, but it is a Python alarm: it ends a step that is slow, not one that hangs inside a native call.
Run the tool under `timeout -k 10 <seconds>` so that a hang ends the process too.

    python tools/subset_time.py [--n 1000000] [--d 128] [--repeats 3] [--fractions 1.0,0.5,0.1,0.01] [--json out.json]
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
from parlayann_amd.index import pack_allow  # noqa: E402

MAX_DEG = 64
DROPPED = np.uint32(0xFFFFFFFF)


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


def random_graph(n, rng):
    """n x (MAX_DEG + 1), reference layout, every row full: row v holds v + 1 + (64 distinct offsets) mod n"""
    G = np.empty((n, MAX_DEG + 1), np.uint32)
    G[:, 0] = MAX_DEG
    base = rng.integers(0, n - 1, n, dtype=np.int64)
    stride = 1 + 2 * rng.integers(0, (n - 2) // (2 * MAX_DEG), n, dtype=np.int64)      # MAX_DEG steps stay below n - 1: distinct
    off = (base[:, None] + stride[:, None] * np.arange(MAX_DEG)[None, :]) % (n - 1)
    G[:, 1:] = (np.arange(n, dtype=np.int64)[:, None] + 1 + off) % n
    return G


def host_route(ix, keep):
    """what a caller did before: download, select and renumber on the host, create a new handle"""
    P, G, L = ix.points(), ix.get_graph(), ix.labels()
    K = np.flatnonzero(keep)
    o2n = np.full(ix.n, DROPPED, np.uint32)
    o2n[K] = np.arange(len(K), dtype=np.uint32)
    old = G[K]
    live = np.arange(MAX_DEG)[None, :] < old[:, :1]
    mapped = o2n[old[:, 1:]]
    kept = live & (mapped != DROPPED)
    slot = np.cumsum(kept, axis=1) - 1
    out = np.zeros_like(old)
    out[:, 0] = kept.sum(axis=1)
    r, _ = np.nonzero(kept)
    out[r, 1 + slot[kept]] = mapped[kept]
    sub = DeviceIndex(P[K], out)
    sub.set_labels(L[K])
    return sub


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fractions", default="1.0,0.5,0.1,0.01")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.n
    rng = np.random.default_rng(1)
    with step("data", 300):
        X = datasets.sift1m_like(n, a.d, seed=1234, dtype=np.float32).astype(np.float16)
        G = random_graph(n, rng)
        L = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    with step("upload", 300):
        ix = DeviceIndex(X, G)
        ix.set_labels(L)
    rows = []
    for frac in (float(f) for f in a.fractions.split(",")):
        keep = np.ones(n, bool) if frac >= 1.0 else rng.random(n) < frac
        allow = pack_allow(keep, n)
        with step(f"keep {frac:g}: both routes once, compared", 600):
            s, n2o, _ = ix.subset(allow)
            h = host_route(ix, keep)
            same = (np.array_equal(n2o, np.flatnonzero(keep)) and np.array_equal(s.points(), h.points())
                    and np.array_equal(s.get_graph(), h.get_graph()) and np.array_equal(s.labels(), h.labels()))
            m = s.n
            s.close()
            h.close()
            if not same:
                print(f"keep {frac:g}: the two routes DIFFER: stopping", flush=True)
                sys.exit(1)
        with step(f"keep {frac:g}: timing", 900):
            ts, th = [], []
            for _ in range(a.repeats):              # (the compared call above was the one that is not counted)
                t0 = time.perf_counter()
                s, _, _ = ix.subset(allow)
                ts.append(time.perf_counter() - t0)
                s.close()
                t0 = time.perf_counter()
                h = host_route(ix, keep)
                th.append(time.perf_counter() - t0)
                h.close()
        row = dict(fraction=frac, kept=m, subset_s=med(ts), host_s=med(th))
        rows.append(row)
        print(f"  keep {frac:5g}: m {m:8d}  subset() {row['subset_s'][0] * 1e3:9.2f} ms (min {row['subset_s'][1] * 1e3:.2f}, max "
              f"{row['subset_s'][2] * 1e3:.2f})  |  host route {row['host_s'][0] * 1e3:9.2f} ms (min {row['host_s'][1] * 1e3:.2f}, max "
              f"{row['host_s'][2] * 1e3:.2f})  |  x{row['host_s'][0] / row['subset_s'][0]:.1f}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(n=n, d=a.d, max_deg=MAX_DEG, repeats=a.repeats, rows=rows), f, indent=1)
    ix.close()


if __name__ == "__main__":
    main()
