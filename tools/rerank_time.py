"""Quantised search with exact rerank: what the one-byte copy buys for a float32 table, and what keeping the pipeline on
the device buys (DESIGN.md "Quantised search with exact rerank").  One process, three paths over the same resident
queries, beam 64, k = 10:

  (a) float      pann_batch_search_dev on the f32 handle                       HIP events on a stream of its own
  (b) composed   pann_quantize_rows, pann_batch_search (out_k = beam) on the one-byte handle, min(frontier, k * 100) on
                 the host, pann_rerank on the f32 handle -- GraphIndex._search before the fused call       wall clock
  (c) fused      pann_batch_search_rerank_dev                                  HIP events on a stream of its own

For each: time per batch, QPS, recall@10 against pann_bruteforce_knn on the float table, and the algorithmic bytes per
query computed from the counters: dist_cmps rows of the searched table plus, for (b) and (c), num_check float rows of the
rerank (adjacency rows are the same for all three and left out).  (c)'s ids must equal (b)'s; the tool stops otherwise.

Every step has a time limit, but it is a Python alarm: it ends a step that is slow, not one that hangs inside a native
call.  Run the tool under `timeout -k 10 <seconds>` so that a hang ends the process too.

    python tools/rerank_time.py [--n 1000000] [--d 128] [--nq 10000] [--steps 20] [--json out.json]
    python tools/rerank_time.py --bits 4 [--beam 128] # the quantised copy holds four-bit rows (DESIGN.md "Four-bit rows")
    python tools/rerank_time.py --profile-steps 5     # only fused steps, for a kernel trace taken in a run of its own
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
from parlayann_amd import DeviceIndex, _capi, datasets, quantize  # noqa: E402
from parlayann_amd.recall import recall_at_k  # noqa: E402

K, BEAM, RF = 10, 64, 100


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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--bits", type=int, choices=(8, 4), default=8, help="bits per coordinate of the quantised copy")
    ap.add_argument("--beam", type=int, default=BEAM)
    a = ap.parse_args()
    import torch
    n, d, nq, beam = a.n, a.d, a.nq, a.beam
    qrow = d if a.bits == 8 else (d + 1) // 2          # bytes of one row of the quantised copy
    with step("data", 300):                       # real-valued, so that the quantiser is not the identity
        X = (datasets.deep_like(n, d, seed=1) * 2.0).astype(np.float32)
        Q = (datasets.deep_like(nq, d, seed=2) * 2.0).astype(np.float32)
    with step("upload + build R=64 L=128", 900):
        full = DeviceIndex(X, max_degree=64, metric="Euclidian")
        full.vamana_build(64, 128, 1.2, num_passes=1, seed=3)
    with step("quantise", 120):
        quant, qparams = full.quantized("euclid_u8" if a.bits == 8 else "euclid_u4")
        assert not qparams.identity
    lib = _capi.load()
    qp = _capi.QueryParams(k=K, beam=beam, cut=1.35, limit=n, degree_limit=64, rerank_factor=RF, pad=1.0)
    t_q = torch.from_numpy(Q).cuda()
    t_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    t_ids = torch.zeros((nq, K), dtype=torch.int32, device="cuda")
    t_d = torch.zeros((nq, K), dtype=torch.float32, device="cuda")
    t_fs, t_vc, t_dc = (torch.zeros(nq, dtype=torch.int32, device="cuda") for _ in range(3))
    t_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)

    def float_step():
        out = _capi.SearchOut(ids=t_ids.data_ptr(), dists=t_d.data_ptr(), out_k=K, frontier_size=t_fs.data_ptr(),
                              visited_count=t_vc.data_ptr(), dist_cmps=t_dc.data_ptr(), status=t_status.data_ptr())
        _capi.check(lib.pann_batch_search_dev(full.handle, C.c_void_p(t_q.data_ptr()), None, nq, 4 * d, C.c_void_p(t_st.data_ptr()), 1,
                                              C.byref(qp), C.byref(out), sp))

    def fused_step():
        full.search_rerank_dev(quant, qparams, t_q.data_ptr(), nq, 4 * d, t_st.data_ptr(), 1, t_ids.data_ptr(), t_d.data_ptr(),
                               k=K, beam=beam, limit=n, degree_limit=64, rerank_factor=RF, d_frontier_size_ptr=t_fs.data_ptr(),
                               d_visited_count_ptr=t_vc.data_ptr(), d_dist_cmps_ptr=t_dc.data_ptr(),
                               d_status_ptr=t_status.data_ptr(), stream_ptr=stream.cuda_stream)

    def composed_step():
        qq = quantize.device_quantize_rows(Q, qparams)
        r = quant.batch_search(qq, k=K, beam=beam, out_k=beam, limit=n, degree_limit=64)
        counts = np.minimum(r["frontier_size"], K * RF).astype(np.uint32)
        return r, counts, full.rerank(Q, r["ids"], counts, K, resort=True)

    def timed_dev(fn, steps):
        for _ in range(a.warmup):
            fn()
        stream.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        with torch.cuda.stream(stream):
            for e0, e1 in ev:
                e0.record(stream); fn(); e1.record(stream)
        stream.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        assert int(t_status.cpu()[0]) == 0
        return ms[len(ms) // 2], ms[0], ms[-1]

    if a.profile_steps:
        with step("fused steps for the trace", 300):
            for _ in range(a.warmup + a.profile_steps):
                fused_step()
            stream.synchronize()
        return
    with step("ground truth", 600):
        gt, gd = full.bruteforce_knn(Q, K)
    rows = []

    def report(name, ms, lo, hi, ids, cmps, row_bytes, num_check):
        by = float(cmps.mean()) * row_bytes + float(num_check) * 4 * d
        rows.append(dict(path=name, ms=ms, ms_min=lo, ms_max=hi, qps=nq / ms * 1e3, recall10=recall_at_k(ids, gt, gd, K),
                         dist_cmps=float(cmps.mean()), num_check=float(num_check), bytes_per_query=by))
        print(f"  {name:9s} {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})  QPS {rows[-1]['qps']:10.0f}  recall@10 {rows[-1]['recall10']:.4f}  "
              f"full dists/q {cmps.mean():8.1f}  rerank rows/q {num_check:5.1f}  bytes/q {by:10.0f}", flush=True)

    with step("(a) float search", 300):
        ms = timed_dev(float_step, a.steps)
        report("float", *ms, t_ids.cpu().numpy().view(np.uint32), t_dc.cpu().numpy().view(np.uint32), 4 * d, 0.0)
    with step("(b) composed", 300):
        composed_step()
        ts = []
        for _ in range(max(3, a.steps // 4)):
            t = time.perf_counter(); r, counts, (ids_b, _) = composed_step(); ts.append((time.perf_counter() - t) * 1e3)
        ts.sort()
        report("composed", ts[len(ts) // 2], ts[0], ts[-1], ids_b, r["dist_cmps"], qrow, counts.mean())
    with step("(c) fused", 300):
        ms = timed_dev(fused_step, a.steps)
        ids_c = t_ids.cpu().numpy().view(np.uint32)
        nc = np.minimum(t_fs.cpu().numpy().view(np.uint32), K * RF)
        report("fused", *ms, ids_c, t_dc.cpu().numpy().view(np.uint32), qrow, nc.mean())
    if not np.array_equal(ids_b, ids_c):
        print("ERROR: the fused ids differ from the composed ids", flush=True)
        sys.exit(1)
    print(f"  fused ids == composed ids; table {n * d * 4 / 2**20:.0f} MiB float / {n * qrow / 2**20:.0f} MiB "
          f"{'one-byte' if a.bits == 8 else 'four-bit'} (Infinity Cache: 256 MiB)", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(n=n, d=d, nq=nq, k=K, beam=beam, bits=a.bits, rerank_factor=RF, steps=a.steps, rows=rows), f, indent=1)
    quant.close(); full.close()


if __name__ == "__main__":
    main()
