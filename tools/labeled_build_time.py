"""Plain against label-aware Vamana under selective filters (DESIGN.md "Label-aware build").  1M x 128 fp16
(datasets.sift1m_like), 32 labels with skewed frequencies -- label b is drawn with weight 2^-(b / 3), so the most frequent is on
about a tenth of the points and the rarest on about a thousandth -- and 1 to 3 labels per point.  Two handles over the same points:

  plain     vamana_build(R = 64, L = 128, alpha 1.2, two passes)
  labeled   the same call with label_starts = label_start_table() (the per-label medoids)

Reported: the build time of each (wall clock, one build each: a build is minutes, not a kernel), then for single-label `any`
predicates at about 10 %, 1 % and 0.1 % allowed -- the labels whose frequency is nearest -- the masked beam-64 search on each
graph from vertex 0 and from the label's medoid: queries/s (median of --steps runs after a warm-up, min and max beside it) and
tie-aware recall@10 against bruteforce_knn_labeled.  Every step has a time limit, but it is a Python alarm: run the tool under
`timeout -k 10 <seconds>` so that a hang inside a native call ends the process too.

    python tools/labeled_build_time.py [--n 1000000] [--nq 10000] [--steps 5] [--json out.json]
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
from parlayann_amd.recall import recall_at_k  # noqa: E402

K, R, L, ALPHA, BEAM, NLABELS = 10, 64, 128, 1.2, 64, 32


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
        return self

    def __exit__(self, *exc):
        signal.alarm(0)
        self.s = time.perf_counter() - self.t0
        print(f"  [{self.name}: {self.s:.1f}s]", flush=True)
        return False


def skewed_labels(n, seed):
    """one uint32 per point: 1-3 of 32 labels, label b with weight 2^-(b / 3)"""
    rng = np.random.default_rng(seed)
    w = 2.0 ** (-np.arange(NLABELS) / 3.0)
    picks = rng.choice(NLABELS, (n, 3), p=w / w.sum())
    keep = np.arange(3)[None, :] < rng.integers(1, 4, n)[:, None]
    lab = np.zeros(n, np.uint32)
    for j in range(3):
        lab |= np.where(keep[:, j], np.uint32(1) << picks[:, j].astype(np.uint32), np.uint32(0))
    return lab


def wall(fn, steps, warmup):
    for _ in range(warmup):
        r = fn()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        r = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return r, ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n, nq = a.n, a.nq
    with step("data", 300):
        X = datasets.sift1m_like(n, a.d, seed=1234, dtype=np.float32).astype(np.float16)
        Q = datasets.sift1m_like(nq, a.d, seed=4321, dtype=np.float16)
        labels = skewed_labels(n, 99)
        freq = np.array([((labels >> b) & 1).mean() for b in range(NLABELS)])
    graphs, rows = {}, []
    for name in ("plain", "labeled"):
        ix = DeviceIndex(X, max_degree=R)
        ix.set_labels(labels)
        table = ix.label_start_table()
        with step(f"build {name} R={R} L={L}", 1500) as s:
            ix.vamana_build(R, L, ALPHA, num_passes=2, seed=1, sort_neighbors=True, label_starts=table if name == "labeled" else None)
        graphs[name] = (ix, table)
        rows.append(dict(graph=name, build_s=s.s))
        print(f"{name}: build {s.s:.2f} s", flush=True)
    for target in (0.10, 0.01, 0.001):
        b = int(np.argmin(np.abs(np.log(freq) - np.log(target))))
        where = ("any", (1 << b, 0))
        with step(f"label {b}: ground truth", 600):
            gt, gd, _ = graphs["plain"][0].bruteforce_knn_labeled(Q, 2 * K, where)      # 2 K: the ties of the k-th
        for name, (ix, table) in graphs.items():
            for entry, starts in (("start 0", (0,)), ("medoid", table[b])):
                with step(f"label {b} ({100 * freq[b]:.2f} %): {name}, {entry}", 600):
                    r, ms, lo, hi = wall(lambda: ix.batch_search_labeled(Q, where=where, starts=starts, k=K, beam=BEAM, out_k=K), a.steps, a.warmup)
                row = dict(graph=name, label=b, allowed=float(freq[b]), entry=entry, ms=ms, ms_min=lo, ms_max=hi, qps=nq / ms * 1e3,
                           recall10=recall_at_k(r["ids"], gt, gd, K))
                rows.append(row)
                print(f"  label {b:2d} {100 * freq[b]:6.2f} % allowed  {name:8s} {entry:8s} {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})  "
                      f"{row['qps']:10.0f} q/s  recall@10 {row['recall10']:.4f}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(n=n, d=a.d, nq=nq, k=K, beam=BEAM, R=R, L=L, alpha=ALPHA, steps=a.steps, rows=rows), f, indent=1)
    for ix, _ in graphs.values():
        ix.close()


if __name__ == "__main__":
    main()
