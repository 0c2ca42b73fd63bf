"""What a per-filter entry point buys (DESIGN.md "Entry points").  The bench.py workload -- 1M x 128 fp16 (datasets.sift1m_like),
Vamana R = 64 L = 128 alpha 1.15 two passes, 10 000 queries, k = 10 -- with CLUSTERED filters: T random pivot points, every point
belongs to the tenant of its nearest pivot (bruteforce_knn(k = 1) against a handle of the pivots), every query asks for the tenant
of ITS nearest pivot.  T = 100 and 1 000: filters of about 1 % and 0.1 % of the points that sit in one region of the graph.

Per T, in one process:

  medoids    filter_medoids for the whole table: the device call between two HIP events (pann_filter_medoids_labeled_dev; it
             synchronises once inside), the host-pointer call on the wall clock, and numpy doing the same job (per-tenant mean in
             float64, nearest allowed point); the allowed rows' bytes over the device time is a LOWER bound of the list-sum
             kernel's rate (the call also compacts the lists and runs the dense kernels).  --kernel-trace DIR gives the kernel
             alone: the tool starts itself with --only-medoids as a fresh child process under `rocprofv3 --kernel-trace`, reads the
             trace database and reports, per table, list_sum_kernel's time per call (the launches of a call summed, the first,
             cold call apart) and its bytes/s against the HBM peak, with centroid_rows_kernel and the dense launch beside it
  searches   beam 64: masked, steered fill 16, steered fill 64 -- from vertex 0 (batch_search_labeled, one predicate per query) and
             from the tenant's medoid (batch_search_grouped with filter_medoids(per_filter=1, fill_id=0)); host-pointer calls on the
             wall clock; queries/s, tie-aware recall@10 against bruteforce_knn_grouped, mean dist_cmps

Several runs per row after a warm-up; median, min and max are printed.  Every step has a time limit, but it is a Python alarm: run
the tool under `timeout -k 10 <seconds>` so that a hang inside a native call ends the process too.

    python tools/entry_time.py [--n 1000000] [--nq 10000] [--steps 5] [--tenants 100,1000] [--only-medoids] [--json out.json]
    python tools/entry_time.py --kernel-trace DIR [--n ...] [--steps ...] [--tenants ...]
"""
import argparse
import ctypes as C
import json
import os
import glob
import signal
import sqlite3
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parlayann_amd import DeviceIndex, _capi, datasets  # noqa: E402
from parlayann_amd.recall import recall_at_k  # noqa: E402

K, R, L, ALPHA, BEAM = 10, 64, 128, 1.15, 64
HBM_PEAK = 8.0e12          # bytes/s, the MI355X's specified peak


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


def wall(fn, steps, warmup):
    """(result of the last run, median ms, min, max) on the wall clock"""
    for _ in range(warmup):
        r = fn()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        r = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return r, ms[len(ms) // 2], ms[0], ms[-1]


def kernel_trace(a):
    """the medoid calls alone in a child process under the kernel trace; per table the kernels' time per call"""
    tenants = [int(t) for t in a.tenants.split(",")]
    cmd = ["rocprofv3", "--kernel-trace", "-d", a.kernel_trace, "-o", "entry", "--", sys.executable, os.path.abspath(__file__), "--only-medoids",
           "--n", str(a.n), "--d", str(a.d), "--steps", str(a.steps), "--warmup", str(a.warmup), "--tenants", a.tenants]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-2000:], flush=True)
        return r.returncode
    dbs = glob.glob(os.path.join(a.kernel_trace, "**", "*.db"), recursive=True)
    if not dbs:
        print(f"no trace database under {a.kernel_trace}", flush=True)
        return 1
    rows = sqlite3.connect(dbs[0]).execute("select name, start, end from kernels order by start").fetchall()
    calls, cur = [], {}                                 # one dict per medoid call: kernel -> microseconds; pad_fill_kernel ends a call
    for name, t0, t1 in rows:
        for key in ("list_sum_kernel", "centroid_rows_kernel", "piece_scan_kernel", "dense_topk", "pad_fill_kernel"):
            if key in name:
                cur[key] = cur.get(key, 0.0) + (t1 - t0) / 1e3
        if "pad_fill_kernel" in name:
            calls.append(cur)
            cur = {}
    per_table = 2 * (a.warmup + a.steps)                # the device-pointer calls, then the host-pointer calls
    if len(calls) != per_table * len(tenants):
        print(f"expected {per_table * len(tenants)} medoid calls in the trace, found {len(calls)}", flush=True)
        return 1
    out = []
    for i, T in enumerate(tenants):
        mine = calls[i * per_table:(i + 1) * per_table]
        row = dict(tenants=T, route="kernel trace", calls=len(mine), list_sum_first_us=mine[0].get("list_sum_kernel", 0.0))
        for key in ("list_sum_kernel", "centroid_rows_kernel", "piece_scan_kernel", "dense_topk"):
            us = sorted(c.get(key, 0.0) for c in mine[1:])
            row[key + "_us"], row[key + "_us_min"], row[key + "_us_max"] = us[len(us) // 2], us[0], us[-1]
        row["list_sum_bytes_per_s"] = float(a.n) * 2 * a.d / (row["list_sum_kernel_us"] * 1e-6)
        row["list_sum_fraction_of_hbm_peak"] = row["list_sum_bytes_per_s"] / HBM_PEAK
        out.append(row)
        print(f"  T={T} list_sum_kernel {row['list_sum_kernel_us']:.1f} us per call (min {row['list_sum_kernel_us_min']:.1f}, max "
              f"{row['list_sum_kernel_us_max']:.1f}; the first, cold call {row['list_sum_first_us']:.1f})  {row['list_sum_bytes_per_s'] / 1e12:.2f} TB/s = "
              f"{100 * row['list_sum_fraction_of_hbm_peak']:.1f} % of the HBM peak   centroid_rows_kernel {row['centroid_rows_kernel_us']:.1f} us  "
              f"piece_scan_kernel {row['piece_scan_kernel_us']:.1f} us  dense launch {row['dense_topk_us']:.1f} us", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(n=a.n, d=a.d, steps=a.steps, rows=out), f, indent=1)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tenants", default="100,1000")
    ap.add_argument("--only-medoids", action="store_true")
    ap.add_argument("--kernel-trace", metavar="DIR", default=None, help="trace the medoid calls in a child process; write the trace under DIR")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.kernel_trace:      # before this process touches the device
        sys.exit(kernel_trace(a))
    import torch
    n, d, nq = a.n, a.d, a.nq
    with step("data", 300):
        X = datasets.sift1m_like(n, d, seed=1234, dtype=np.float32).astype(np.float16)
        Q = datasets.sift1m_like(nq, d, seed=4321, dtype=np.float16)
    with step(f"upload + build R={R} L={L}", 900):
        ix = DeviceIndex(X, max_degree=R)
        if not a.only_medoids:
            ix.vamana_build(R, L, ALPHA, num_passes=2, seed=1, sort_neighbors=True)
    lib = _capi.load()
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())
    rows = []
    for T in [int(t) for t in a.tenants.split(",")]:
        with step(f"T={T}: tenants", 300):
            piv = np.sort(np.random.default_rng(50 + T).choice(n, T, replace=False))
            px = DeviceIndex(np.ascontiguousarray(X[piv]), max_degree=4)
            labels = np.concatenate([px.bruteforce_knn(X[i:i + 200000], 1)[0][:, 0] for i in range(0, n, 200000)]).astype(np.uint32)
            group = np.ascontiguousarray(px.bruteforce_knn(Q, 1)[0][:, 0].astype(np.uint32))
            px.close()
            ix.set_labels(labels)
            table = np.ascontiguousarray(np.stack([np.arange(T), np.arange(T)], 1).astype(np.uint32))      # RANGE [t, t]
            sizes = np.bincount(labels, minlength=T)
            print(f"T={T}: tenant sizes min {sizes.min()} median {int(np.median(sizes))} max {sizes.max()}", flush=True)
        name = f"T={T}"
        # ---- medoids: device, host-inclusive, numpy ----
        with step(f"{name}: filter_medoids", 600):
            t_p = torch.from_numpy(table.view(np.int32)).cuda()
            t_ids = torch.zeros((T, 1), dtype=torch.int32, device="cuda"); t_d = torch.zeros((T, 1), dtype=torch.float32, device="cuda")
            t_c = torch.zeros(T, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            call = lambda: _capi.check(lib.pann_filter_medoids_labeled_dev(ix.handle, _capi.PANN_PRED_RANGE, vp(t_p), T, 1, 0, 0, vp(t_ids), vp(t_d),
                                                                           vp(t_c), None, sp))
            for _ in range(a.warmup):
                call()
            stream.synchronize()
            dev_ms = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream); call(); e1.record(stream)
                stream.synchronize()
                dev_ms.append(e0.elapsed_time(e1))
            dev_ms.sort()
            med, h_ms, h_min, h_max = wall(lambda: ix.filter_medoids(where=("range", table), per_filter=1, fill_id=0), a.steps, a.warmup)
            assert np.array_equal(med["ids"].view(np.int32), t_ids.cpu().numpy())
        with step(f"{name}: numpy medoids", 900):
            def by_numpy():
                order = np.argsort(labels, kind="stable")
                off = np.concatenate([[0], np.cumsum(sizes)])
                out = np.zeros(T, np.uint32)
                for t in range(T):
                    sel = order[off[t]:off[t + 1]]
                    if len(sel):
                        rows_t = X[sel].astype(np.float64)
                        c = rows_t.mean(axis=0)
                        out[t] = sel[np.argmin(((rows_t - c) ** 2).sum(axis=1))]
                return out
            _, n_ms, n_min, n_max = wall(by_numpy, max(1, a.steps // 2), 0)
        row_bytes = float(n) * 2 * d
        mrow = dict(tenants=T, route="filter_medoids", dev_ms=dev_ms[len(dev_ms) // 2], dev_ms_min=dev_ms[0], dev_ms_max=dev_ms[-1], host_ms=h_ms,
                    host_ms_min=h_min, host_ms_max=h_max, numpy_ms=n_ms, numpy_ms_min=n_min, numpy_ms_max=n_max,
                    rows_bytes_per_s_lower_bound=row_bytes / (dev_ms[len(dev_ms) // 2] * 1e-3))
        mrow["fraction_of_hbm_peak_lower_bound"] = mrow["rows_bytes_per_s_lower_bound"] / HBM_PEAK
        rows.append(mrow)
        print(f"  {name} filter_medoids: device {mrow['dev_ms']:.3f} ms (min {dev_ms[0]:.3f}, max {dev_ms[-1]:.3f})  host-inclusive {h_ms:.3f} ms "
              f"(min {h_min:.3f}, max {h_max:.3f})  numpy {n_ms:.1f} ms (min {n_min:.1f}, max {n_max:.1f})  allowed rows / device time "
              f"{mrow['rows_bytes_per_s_lower_bound'] / 1e12:.3f} TB/s = {100 * mrow['fraction_of_hbm_peak_lower_bound']:.1f} % of the HBM peak "
              f"(a lower bound of the list-sum kernel's rate)", flush=True)
        if a.only_medoids:
            continue
        # ---- searches: start 0 against the tenant's medoid ----
        with step(f"{name}: ground truth", 600):
            gt, gd, _ = ix.bruteforce_knn_grouped(Q, 2 * K, where=("range", table), group_of_query=group)      # 2 K: the ties of the k-th
        starts = med["ids"]
        preds = np.ascontiguousarray(table[group])
        kw = dict(k=K, beam=BEAM, out_k=K)
        for route, steer in (("masked", None), ("steered fill 16", 16), ("steered fill 64", 64)):
            for entry in ("start 0", "medoid"):
                with step(f"{name}: {route}, {entry}", 600):
                    if entry == "start 0":
                        fn = lambda: ix.batch_search_labeled(Q, where=("range", preds), starts=(0,), steer=steer, **kw)
                    else:
                        fn = lambda: ix.batch_search_grouped(Q, where=("range", table), group_of_query=group, starts=starts, steer=steer, **kw)
                    r, ms, ms_min, ms_max = wall(fn, a.steps, a.warmup)
                    if int(r["status"][0]) != 0:
                        print("ERROR: status", int(r["status"][0]), flush=True)
                        sys.exit(1)
                    real = r["ids"] != 0xFFFFFFFF
                    if not (labels[r["ids"][real]] == group[np.nonzero(real)[0]]).all():
                        print("ERROR: a walk returned a point of another tenant", flush=True)
                        sys.exit(1)
                row = dict(tenants=T, route=route, entry=entry, ms=ms, ms_min=ms_min, ms_max=ms_max, qps=nq / ms * 1e3,
                           recall10=recall_at_k(r["ids"], gt, gd, K), dist_cmps=float(r["dist_cmps"].mean()), visited=float(r["visited_count"].mean()))
                rows.append(row)
                print(f"  {name} {route:16s} {entry:8s} {ms:9.3f} ms (min {ms_min:.3f}, max {ms_max:.3f})  {row['qps']:10.0f} q/s  recall@10 "
                      f"{row['recall10']:.4f}  dist_cmps {row['dist_cmps']:8.1f}  visited {row['visited']:6.1f}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(n=n, d=d, nq=nq, k=K, beam=BEAM, steps=a.steps, rows=rows), f, indent=1)
    ix.close()


if __name__ == "__main__":
    main()
