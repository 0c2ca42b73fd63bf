"""Graph reachability on the device against the host alternative (DESIGN.md "Graph reachability").  One process, one session:

  build     1M x 128 fp16 Vamana graph, R = 64, L = 128, alpha 1.15, two passes -- bench.py's flagship index
  reach     DeviceIndex.reachability((0,)) with levels and ids, and without either: wall clock around the call (it returns
            after the stream has drained) and the call's own device time (pann_reach_stats.t_s, two events)
  degrees   DeviceIndex.degrees() (wall clock, both arrays come down) and pann_graph_degrees_dev alone (two events)
  host      what a caller did before: get_graph() and the numpy walk of tests/reach_ref.py, timed separately
  deleted   all of it again after ONE pann_vamana_delete_batch of 20 % of the points, with the live bitmap as `consider`
  fixed     the same call on a 64-vertex handle with empty rows: the cost of a call that walks nothing (one group of rounds)

The device and the host answer are compared once per state before anything is timed.  Every figure is the median of --repeats
calls after one call that is not counted; the smallest and largest are printed with it.  The floor printed beside them is the
graph's bytes (n rows of gstride words) over 6.3 TB/s, the HBM rate a streaming kernel reaches on this part.

Every step has a time limit, but it is a Python alarm: it ends a step that is slow, not one that hangs inside a native call.
Run the tool under `timeout -k 10 <seconds>` so that a hang ends the process too.

    python tools/reach_time.py [--n 1000000] [--d 128] [--repeats 5] [--fraction 0.2] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reach_ref as rr  # noqa: E402
from parlayann_amd import DeviceIndex, _capi, allow_bitmap, datasets  # noqa: E402

R, L, ALPHA, PASSES = 64, 128, 1.15, 2
HBM_BYTES_PER_S = 6.3e12
GROUP = 8                  # REACH_GROUP of csrc/pann_internal.h


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


def ms(t):
    return f"{t[0] * 1e3:9.3f} ms (min {t[1] * 1e3:.3f}, max {t[2] * 1e3:.3f})"


def timed(fn, repeats):
    """-> (wall seconds, what fn returned) per counted call; one call before them is not counted"""
    fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0, r))
    return out


def degrees_dev_seconds(ix, repeats):
    import torch
    lib = _capi.load()
    d_out, d_in = torch.empty(ix.n, dtype=torch.int32, device="cuda:0"), torch.empty(ix.n, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.current_stream()
    ts = []
    for i in range(repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        _capi.check(lib.pann_graph_degrees_dev(ix.handle, C.c_void_p(d_out.data_ptr()), C.c_void_p(d_in.data_ptr()), C.c_void_p(s.cuda_stream or None)))
        e1.record(s)
        e1.synchronize()
        if i:
            ts.append(e0.elapsed_time(e1) * 1e-3)
    return med(ts)


def measure(ix, name, consider, repeats, with_host=True):
    n = ix.n
    row = dict(state=name)
    if with_host:
        with step(f"{name}: device and host answers compared", 900):
            G = ix.get_graph()
            ref = rr.reach_ref(G, (0,), consider)
            rr.same_fields(ix.reachability((0,), consider), ref)
            for a, b in zip(ix.degrees(), rr.degrees_ref(G)):
                assert np.array_equal(a, b)
            del G
        row.update({k: ref[k] for k in rr.STAT_KEYS})
    with step(f"{name}: device timing", 900):
        full = timed(lambda: ix.reachability((0,), consider), repeats)
        bare = timed(lambda: ix.reachability((0,), consider, levels=False, ids=False), repeats)
        deg = timed(ix.degrees, repeats)
        row.update(reach_wall_s=med([t for t, _ in full]), reach_dev_s=med([r["seconds"] for _, r in full]),
                   reach_bare_wall_s=med([t for t, _ in bare]), reach_bare_dev_s=med([r["seconds"] for _, r in bare]),
                   degrees_wall_s=med([t for t, _ in deg]), degrees_dev_s=degrees_dev_seconds(ix, repeats))
        if not with_host:
            row.update({k: full[0][1][k] for k in rr.STAT_KEYS})
    if with_host:
        with step(f"{name}: host timing", 1800):
            dl = timed(ix.get_graph, repeats)
            G = dl[-1][1]
            walk = timed(lambda: rr.reach_ref(G, (0,), consider), repeats)
            hdeg = timed(lambda: rr.degrees_ref(G), repeats)
            row.update(host_get_graph_s=med([t for t, _ in dl]), host_walk_s=med([t for t, _ in walk]), host_degrees_s=med([t for t, _ in hdeg]))
    graph_bytes = n * ((ix.max_degree + 15) // 16 * 16) * 4
    row.update(graph_bytes=graph_bytes, floor_s=graph_bytes / HBM_BYTES_PER_S, rounds=row["levels"],
               launches=GROUP * ((row["levels"] + GROUP - 1) // GROUP))
    print(f"  {name}: reached {row['reached_count']}, unreached {row['unreached_count']}, levels {row['levels']}, largest level "
          f"{row['max_frontier']}; {row['launches']} expand launches in {row['launches'] // GROUP} group(s)")
    print(f"    graph {graph_bytes / 1e6:.0f} MB, read once at 6.3 TB/s: {row['floor_s'] * 1e3:.3f} ms")
    print(f"    reachability, levels + ids : device {ms(row['reach_dev_s'])}   call {ms(row['reach_wall_s'])}")
    print(f"    reachability, counts only  : device {ms(row['reach_bare_dev_s'])}   call {ms(row['reach_bare_wall_s'])}")
    print(f"    degrees                    : device {ms(row['degrees_dev_s'])}   call {ms(row['degrees_wall_s'])}")
    if with_host:
        print(f"    host: get_graph {ms(row['host_get_graph_s'])}   numpy walk {ms(row['host_walk_s'])}   numpy degrees {ms(row['host_degrees_s'])}")
        host = row["host_get_graph_s"][0] + row["host_walk_s"][0]
        print(f"    host route / reachability call: x{host / row['reach_wall_s'][0]:.0f};  device time / floor: x{row['reach_dev_s'][0] / row['floor_s']:.1f}",
              flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fraction", type=float, default=0.2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.n
    rows = []

    def dump():
        if a.json:
            with open(a.json, "w") as f:
                json.dump(dict(n=n, d=a.d, R=R, L=L, alpha=ALPHA, passes=PASSES, repeats=a.repeats, rows=rows), f, indent=1)

    tiny = DeviceIndex(np.zeros((64, 8), np.uint8), max_degree=R)
    rows.append(measure(tiny, "fixed cost (64 vertices, empty rows)", None, a.repeats, with_host=False))
    tiny.close()
    with step("data", 300):
        X = datasets.sift1m_like(n, a.d, seed=1234, dtype=np.float32).astype(np.float16)
    with step(f"upload + build R={R} L={L} x{PASSES}", 900):
        ix = DeviceIndex(X, max_degree=R)
        ix.vamana_build(R, L, ALPHA, num_passes=PASSES, seed=1, sort_neighbors=True)
    rows.append(measure(ix, "built", None, a.repeats))
    dump()
    m = int(round(a.fraction * n))
    D = (1 + np.random.default_rng(200).choice(n - 1, m, replace=False)).astype(np.uint32)
    with step(f"delete {a.fraction:.0%}", 1800):
        ix.vamana_delete_batch(D, R, ALPHA)
    rows.append(measure(ix, f"after deleting {a.fraction:.0%}", allow_bitmap(n, deleted_ids=D), a.repeats))
    dump()
    ix.close()


if __name__ == "__main__":
    main()
