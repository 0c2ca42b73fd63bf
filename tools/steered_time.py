"""Steered masked search beside the masked search at larger beams and the exact per-query route (DESIGN.md "Steered masked
search").  The bench.py workload -- 1M x 128 fp16 (datasets.sift1m_like), Vamana R = 64 L = 128 alpha 1.15 two passes, 10 000
queries, k = 10 -- with masks that allow 50 %, 10 %, 1 % and 0.1 % of the points, once as ONE mask for the batch and once as a
different mask for every query.  The masks are label windows: every point has a uniform label in 0..9999 and a query may return
the points whose label lies in a window of the mask's width (RANGE predicates; query q's window starts at (q * 37) mod the free
room, the shared mask is query 0's for everybody), so per-query masks cost 8 bytes per query and no bitmap rows are made.

Per mask and form, in one process, HIP events on a stream of its own:

  steered    pann_batch_search_steered_labeled_dev at beam 64 with fill 8, 16, 32, 64
  masked     pann_batch_search_labeled_dev at beams 64, 128, 256, 512
  exact      pann_bruteforce_knn_labeled_dev with one predicate per query (shared masks: the same predicate nq times) -- also the
             ground truth: recall@10 of every walk is counted against its ids

and per row queries/s, recall@10, and per query the mean dist_cmps, bridge_rows and row bytes: point rows of dist_cmps full
distances plus graph rows of the visited vertices and the bridges.

Every step has a time limit, but it is a Python alarm: it ends a step that is slow, not one that hangs inside a native call.
Run the tool under `timeout -k 10 <seconds>` so that a hang ends the process too.

    python tools/steered_time.py [--n 1000000] [--nq 10000] [--steps 5] [--fractions 0.5,0.1,0.01,0.001] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parlayann_amd import DeviceIndex, _capi, datasets  # noqa: E402
from parlayann_amd.recall import recall_at_k  # noqa: E402

K, R, L, ALPHA, LABELS = 10, 64, 128, 1.15, 10000
FILLS, BEAMS = (8, 16, 32, 64), (64, 128, 256, 512)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--fractions", default="0.5,0.1,0.01,0.001")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    n, d, nq = a.n, a.d, a.nq
    with step("data", 300):
        X = datasets.sift1m_like(n, d, seed=1234, dtype=np.float32).astype(np.float16)
        Q = datasets.sift1m_like(nq, d, seed=4321, dtype=np.float16)
        labels = np.random.default_rng(77).integers(0, LABELS, n).astype(np.uint32)
    with step(f"upload + build R={R} L={L}", 900):
        ix = DeviceIndex(X, max_degree=R)
        ix.vamana_build(R, L, ALPHA, num_passes=2, seed=1, sort_neighbors=True)
        ix.set_labels(labels)
    lib = _capi.load()
    gstride = (R + 15) // 16 * 16
    t_q = torch.from_numpy(Q.view(np.uint8).reshape(nq, -1)).cuda()
    t_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    t_ids = torch.zeros((nq, K), dtype=torch.int32, device="cuda")
    t_d = torch.zeros((nq, K), dtype=torch.float32, device="cuda")
    t_rc, t_ac, t_dc, t_vc, t_cnt = (torch.zeros(nq, dtype=torch.int32, device="cuda") for _ in range(5))
    t_steer = torch.zeros((nq, 2), dtype=torch.int32, device="cuda")
    t_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())

    def search_out():
        return _capi.SearchOut(ids=t_ids.data_ptr(), dists=t_d.data_ptr(), out_k=K, visited_count=t_vc.data_ptr(), dist_cmps=t_dc.data_ptr(),
                               status=t_status.data_ptr())

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        stream.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
        with torch.cuda.stream(stream):
            for e0, e1 in ev:
                e0.record(stream); fn(); e1.record(stream)
        stream.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        return ms[len(ms) // 2], ms[0], ms[-1]

    def u32(t):
        return t.cpu().numpy().view(np.uint32).copy()

    rows = []
    qn = np.arange(nq, dtype=np.int64)
    for frac in [float(f) for f in a.fractions.split(",")]:
        width = max(1, int(round(frac * LABELS)))
        for form in ("shared", "per-query"):
            lo = (qn * 37) % (LABELS - width + 1) if form == "per-query" else np.zeros(nq, np.int64)
            preds = np.ascontiguousarray(np.stack([lo, lo + width - 1], 1).astype(np.uint32))
            t_p = torch.from_numpy(preds.view(np.int32)).cuda()
            torch.cuda.synchronize()
            name = f"{frac:.1%} {form}"

            def check_allowed(ids):
                real = ids != 0xFFFFFFFF
                lab = labels[ids[real]]
                qi = np.nonzero(real)[0]
                if not ((lab >= preds[qi, 0]) & (lab <= preds[qi, 1])).all():
                    print("ERROR: a walk returned a point its predicate does not allow", flush=True)
                    sys.exit(1)

            with step(f"{name}: exact per-query route", 600):
                e_ms = timed(lambda: _capi.check(lib.pann_bruteforce_knn_labeled_dev(ix.handle, vp(t_q), nq, 2 * d, K, _capi.PANN_PRED_RANGE, vp(t_p),
                                                                                   nq, vp(t_ids), vp(t_d), vp(t_cnt), sp)))
                gt, gd = u32(t_ids), t_d.cpu().numpy().copy()
            rows.append(dict(mask=name, route="exact", ms=e_ms[0], ms_min=e_ms[1], ms_max=e_ms[2], qps=nq / e_ms[0] * 1e3, recall10=1.0))
            print(f"  {name:18s} exact per-query            {e_ms[0]:9.3f} ms (min {e_ms[1]:.3f}, max {e_ms[2]:.3f})  {rows[-1]['qps']:10.0f} q/s", flush=True)

            def walk(beam, fill):
                qp = _capi.QueryParams(k=K, beam=beam, cut=1.35, limit=n, degree_limit=R, rerank_factor=100, pad=1.0)
                out = search_out()
                if fill is None:
                    _capi.check(lib.pann_batch_search_labeled_dev(ix.handle, vp(t_q), None, nq, 2 * d, vp(t_st), 1, C.byref(qp), _capi.PANN_PRED_RANGE,
                                                                  vp(t_p), nq, C.byref(out), vp(t_rc), vp(t_ac), sp))
                else:
                    _capi.check(lib.pann_batch_search_steered_labeled_dev(ix.handle, vp(t_q), None, nq, 2 * d, vp(t_st), 1, C.byref(qp),
                                                                          _capi.PANN_PRED_RANGE, vp(t_p), nq, C.byref(out), vp(t_rc), vp(t_ac), fill,
                                                                          vp(t_steer), sp))

            for route, beam, fill in [("steered", 64, f) for f in FILLS] + [("masked", b, None) for b in BEAMS]:
                with step(f"{name}: {route} beam {beam}" + (f" fill {fill}" if fill else ""), 300):
                    t_steer.zero_()
                    ms = timed(lambda: walk(beam, fill))
                    if int(t_status.cpu()[0]) != 0:
                        print("ERROR: status", int(t_status.cpu()[0]), flush=True)
                        sys.exit(1)
                    ids = u32(t_ids)
                    check_allowed(ids)
                    dc, vc, st = u32(t_dc), u32(t_vc), u32(t_steer)
                br = st[:, 0] if fill is not None else np.zeros(nq, np.uint32)
                row = dict(mask=name, route=route, beam=beam, fill=fill, ms=ms[0], ms_min=ms[1], ms_max=ms[2], qps=nq / ms[0] * 1e3,
                           recall10=recall_at_k(ids, gt, gd, K), dist_cmps=float(dc.mean()), visited=float(vc.mean()), bridge_rows=float(br.mean()),
                           row_bytes=float((dc.astype(np.float64) * 2 * d + (vc.astype(np.float64) + br) * gstride * 4).mean()))
                rows.append(row)
                print(f"  {name:18s} {route:7s} beam {beam:3d} fill {str(fill):4s} {ms[0]:9.3f} ms (min {ms[1]:.3f}, max {ms[2]:.3f})  {row['qps']:10.0f} q/s  "
                      f"recall@10 {row['recall10']:.4f}  dist_cmps {row['dist_cmps']:8.1f}  visited {row['visited']:6.1f}  bridge_rows "
                      f"{row['bridge_rows']:8.1f}  row bytes {row['row_bytes'] / 1024:8.1f} KB", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(n=n, d=d, nq=nq, k=K, steps=a.steps, rows=rows), f, indent=1)
    ix.close()


if __name__ == "__main__":
    main()
