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
    python tools/rerank_time.py --bits f8 [--metric mips]   # ... FP8 (E4M3) rows (DESIGN.md "FP8 rows"); --metric goes with every --bits
    python tools/rerank_time.py --profile-steps 5     # only fused steps, for a kernel trace taken in a run of its own
    python tools/rerank_time.py --scan [--bits 4] [--no-graph]   # (d) the exhaustive scan, pann_scan_rerank_dev (DESIGN.md "Exhaustive
                                                      # quantised scan"), beside (c); then three alternating wall-clock runs of the host
                                                      # entries pann_scan_rerank / pann_bruteforce_knn on the float handle / (--bits 8)
                                                      # pann_bruteforce_knn(k = 64) on the copy.  --no-graph: no build, (d) and those only
    python tools/rerank_time.py --scan --no-graph --allow-frac 0.05 [--tenants 16]   # the filtered scan (DESIGN.md "Filtered exhaustive
                                                      # scan"), pann_bruteforce_knn_masked / _grouped on the float handle and the unfiltered
                                                      # scan, host entries, three alternating runs; recall@10 against the float route
    python tools/rerank_time.py --scan --no-graph --allow-frac 0.1 --per-query [--labels]   # one filter per query (DESIGN.md "Per-query
                                                      # filtered scan"): the per-query scan, the exact per-query route on the float handle
                                                      # and the unfiltered scan, device entries, --steps alternating rounds under HIP events;
                                                      # the table form with one entry per query on --table-nq queries; recall@10
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
    ap.add_argument("--bits", type=lambda v: v if v == "f8" else int(v), choices=(8, 4, "f8"), default=8,
                    help="bits per coordinate of the quantised copy; f8: one byte of FP8 E4M3")
    ap.add_argument("--beam", type=int, default=BEAM)
    ap.add_argument("--metric", choices=("Euclidian", "mips"), default="Euclidian", help="mips: normalised rows and queries, the MIPS quantisers")
    ap.add_argument("--scan", action="store_true", help="also time the exhaustive scan + rerank (pann_scan_rerank*)")
    ap.add_argument("--no-graph", action="store_true", help="with --scan: build no graph, time the scan and the exact routes only")
    ap.add_argument("--allow-frac", type=float, default=None, help="with --scan: also time the filtered scan under a filter that allows this fraction")
    ap.add_argument("--tenants", type=int, default=1, help="with --allow-frac: a table of this many filters, one index per query (1: one bitmap)")
    ap.add_argument("--per-query", action="store_true", help="with --allow-frac: one filter per query, tested inside the scan (device entries, HIP events)")
    ap.add_argument("--labels", action="store_true", help="with --per-query: range predicates over random labels in place of bitmap rows")
    ap.add_argument("--table-nq", type=int, default=200, help="with --per-query: queries of the table-form comparison (one list per query: slow)")
    a = ap.parse_args()
    import torch
    n, d, nq, beam, mips = a.n, a.d, a.nq, a.beam, a.metric == "mips"
    qrow = (d + 1) // 2 if a.bits == 4 else d          # bytes of one row of the quantised copy
    with step("data", 300):                       # real-valued, so that the quantiser is not the identity
        if mips:                                   # queries normalised here, the rows on the device: every step sees the same floats
            X, Q = datasets.t2i_like(n, d, seed=1), quantize.normalize_rows(datasets.t2i_like(nq, d, seed=2))
        else:
            X = (datasets.deep_like(n, d, seed=1) * 2.0).astype(np.float32)
            Q = (datasets.deep_like(nq, d, seed=2) * 2.0).astype(np.float32)
    with step("upload + build R=64 L=128", 900):
        full = DeviceIndex(X, max_degree=64, metric=a.metric)
        if mips:
            full.normalize()
        if not (a.scan and a.no_graph):
            full.vamana_build(64, 128, 1.2, num_passes=1, seed=3)
    with step("quantise", 120):
        quant, qparams = full.quantized({8: "mips_i8" if mips else "euclid_u8", 4: "mips_i4" if mips else "euclid_u4", "f8": "f8"}[a.bits])
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

    def scan_step():
        full.scan_rerank_dev(quant, qparams, t_q.data_ptr(), nq, 4 * d, t_ids.data_ptr(), t_d.data_ptr(), k=K, rerank_factor=RF,
                             stream_ptr=stream.cuda_stream)

    def scan_report():
        with step("(d) scan", 300):
            ms, lo, hi = timed_dev(scan_step, a.steps)
            rec = recall_at_k(t_ids.cpu().numpy().view(np.uint32), gt, gd, K)
            rows.append(dict(path="scan", ms=ms, ms_min=lo, ms_max=hi, qps=nq / ms * 1e3, recall10=rec, num_check=float(min(K * RF, 64, n))))
            print(f"  {'scan':9s} {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})  QPS {nq / ms * 1e3:10.0f}  recall@10 {rec:.4f}  "
                  f"rows scanned/q {n}  rerank rows/q {min(K * RF, 64, n)}", flush=True)
        with step("host entries, three alternating runs", 600):
            legs = [("scan_rerank", lambda: full.scan_rerank(quant, qparams, Q, K, RF)), ("bruteforce_knn f32", lambda: full.bruteforce_knn(Q, K))]
            if a.bits == 8:
                qq = quantize.device_quantize_rows(Q, qparams)
                legs.append(("bruteforce_knn copy k=64", lambda: quant.bruteforce_knn(qq, 64)))
            for _, fn in legs:
                fn()                                   # warm-up: scratch growth
            wall = {name: [] for name, _ in legs}
            for _ in range(3):
                for name, fn in legs:
                    t = time.perf_counter(); fn(); wall[name].append((time.perf_counter() - t) * 1e3)
            for name, ts in wall.items():
                rows.append(dict(path="host " + name, ms_runs=ts))
                print(f"  host {name:26s} " + "  ".join(f"{t:8.2f}" for t in ts) + " ms", flush=True)

    def filtered_report():
        """--allow-frac F [--tenants G]: the filtered scan, the exact filtered route on the float handle and the unfiltered scan, host
        entries, three alternating wall-clock runs; recall@10 of the filtered scan against the exact filtered route"""
        rng = np.random.default_rng(5)
        G = max(a.tenants, 1)
        if G == 1:         # one bitmap: a random F of the points
            kw, exact = dict(allow=rng.random(n) < a.allow_frac), lambda: full.bruteforce_knn_masked(Q, K, kw["allow"])
        else:              # G tenants of F * n random points each, every query one tenant's
            kw = dict(allow=rng.random((G, n)) < a.allow_frac, group_of_query=rng.integers(0, G, nq).astype(np.uint32))
            exact = lambda: full.bruteforce_knn_grouped(Q, K, **kw)
        with step("filtered scan, three alternating runs", 900):
            legs = [("scan_rerank filtered", lambda: full.scan_rerank(quant, qparams, Q, K, RF, **kw)), ("bruteforce_knn filtered f32", exact),
                    ("scan_rerank unfiltered", lambda: full.scan_rerank(quant, qparams, Q, K, RF))]
            got = {name: fn() for name, fn in legs}        # warm-up: scratch growth; and the results for the recall
            wall = {name: [] for name, _ in legs}
            for _ in range(3):
                for name, fn in legs:
                    t = time.perf_counter(); fn(); wall[name].append((time.perf_counter() - t) * 1e3)
            ei, ed, _ = got["bruteforce_knn filtered f32"]
            rec = recall_at_k(got["scan_rerank filtered"]["ids"], ei, ed, K)
            for name, ts in wall.items():
                rows.append(dict(path="host " + name, ms_runs=ts, allow_frac=a.allow_frac, tenants=G))
                print(f"  host {name:28s} " + "  ".join(f"{t:8.2f}" for t in ts) + " ms", flush=True)
            rows.append(dict(path="scan_rerank filtered", recall10=rec))
            print(f"  filtered scan recall@10 against the exact filtered route: {rec:.4f}  (allow-frac {a.allow_frac}, tenants {G})", flush=True)

    def per_query_report():
        """--allow-frac F --per-query [--labels]: one filter per query.  HIP events on the tool's stream, a.steps alternating rounds
        of: the per-query scan (pann_scan_rerank_*_per_query_dev), the exact per-query route on the float handle
        (pann_bruteforce_knn_masked_dev / _labeled_dev with one row / predicate per query) and the unfiltered scan; then the
        table form of the filtered scan with one entry per query on the first --table-nq queries (wall clock: it synchronises),
        beside the per-query scan on the same queries; recall@10 of the per-query scan against the exact route."""
        rng = np.random.default_rng(5)
        t_cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
        t_ids2, t_d2 = torch.zeros((nq, K), dtype=torch.int32, device="cuda"), torch.zeros((nq, K), dtype=torch.float32, device="cuda")
        if a.labels:      # labels uniform in [0, 1000): the range predicate of query q allows a window of F * 1000 values
            full.set_labels(rng.integers(0, 1000, n).astype(np.uint32))
            lo = rng.integers(0, 1000 - max(int(a.allow_frac * 1000), 1) + 1, nq)
            preds = np.stack([lo, lo + max(int(a.allow_frac * 1000), 1) - 1], 1).astype(np.uint32)
            t_f = torch.from_numpy(preds.view(np.int32)).cuda()
            flt = dict(d_preds_ptr=t_f.data_ptr(), pred_kind="range")
            exact_step = lambda: _capi.check(lib.pann_bruteforce_knn_labeled_dev(full.handle, C.c_void_p(t_q.data_ptr()), nq, 4 * d, K, _capi.PANN_PRED_RANGE,
                                                                                 C.c_void_p(t_f.data_ptr()), nq, C.c_void_p(t_ids2.data_ptr()),
                                                                                 C.c_void_p(t_d2.data_ptr()), C.c_void_p(t_cnt.data_ptr()), sp))
            table_kw = lambda m: dict(where=("range", preds[:m]), group_of_query=np.arange(m))
        else:             # a random F of the points per query, drawn on the device (int64 words: 2 x ceil(n / 64) uint32 per row)
            W = (n + 63) // 64 * 2
            t_f = torch.zeros((nq, W // 2), dtype=torch.int64, device="cuda")
            weights = (1 << torch.arange(64, dtype=torch.int64, device="cuda"))
            for q0 in range(0, nq, 64):
                bits = torch.rand((min(64, nq - q0), W // 2, 64), device="cuda") < a.allow_frac
                t_f[q0:q0 + 64] = (bits.to(torch.int64) * weights).sum(-1)
            flt = dict(d_allow_ptr=t_f.data_ptr(), allow_stride_words=W)
            exact_step = lambda: full.bruteforce_knn_masked_dev(t_q.data_ptr(), nq, 4 * d, K, t_f.data_ptr(), W, t_ids2.data_ptr(), t_d2.data_ptr(),
                                                                t_cnt.data_ptr(), stream.cuda_stream)
            table_kw = lambda m: dict(allow=t_f[:m].cpu().numpy().view(np.uint32), group_of_query=np.arange(m))
        pq_step = lambda: full.scan_rerank_dev(quant, qparams, t_q.data_ptr(), nq, 4 * d, t_ids.data_ptr(), t_d.data_ptr(), k=K, rerank_factor=RF,
                                               per_query=True, stream_ptr=stream.cuda_stream, **flt)
        legs = [("per-query scan", pq_step), ("exact per-query f32", exact_step), ("unfiltered scan", scan_step)]
        with step("per-query filters, alternating runs", 900):
            for _, fn in legs:
                for _ in range(a.warmup):
                    fn()
            stream.synchronize()
            ms = {name: [] for name, _ in legs}
            for _ in range(a.steps):
                for name, fn in legs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream); fn(); e1.record(stream); stream.synchronize()
                    ms[name].append(e0.elapsed_time(e1))
            for name, ts in ms.items():
                rows.append(dict(path=name, ms_runs=ts, ms=float(np.median(ts)), allow_frac=a.allow_frac, labels=bool(a.labels)))
                print(f"  {name:22s} median {np.median(ts):8.3f} ms  (min {min(ts):.3f}, max {max(ts):.3f}, {len(ts)} runs)", flush=True)
            pq_step(); exact_step(); stream.synchronize()
            rec = recall_at_k(t_ids.cpu().numpy().view(np.uint32), t_ids2.cpu().numpy().view(np.uint32), t_d2.cpu().numpy(), K)
            rows.append(dict(path="per-query scan", recall10=rec))
            print(f"  per-query scan recall@10 against the exact per-query route: {rec:.4f}  (allow-frac {a.allow_frac})", flush=True)
        m = min(a.table_nq, nq)
        with step(f"table form with one entry per query, {m} queries", 600):
            kw = table_kw(m)
            pq_kw = {k: v for k, v in kw.items() if k != "group_of_query"}
            hosts = [("table form", lambda: full.scan_rerank(quant, qparams, Q[:m], K, RF, **kw)),
                     ("per-query scan (host entry)", lambda: full.scan_rerank(quant, qparams, Q[:m], K, RF, per_query=True, **pq_kw))]
            got = [fn() for _, fn in hosts]
            assert np.array_equal(got[0]["ids"], got[1]["ids"]), "the table form and the per-query scan disagree"
            for _ in range(3):
                for name, fn in hosts:
                    t = time.perf_counter(); fn(); rows.append(dict(path=name, nq=m, ms=(time.perf_counter() - t) * 1e3))
                    print(f"  host {name:28s} {m} queries {rows[-1]['ms']:9.2f} ms", flush=True)

    if a.scan and a.allow_frac is not None and a.per_query:
        per_query_report()
    elif a.scan and a.allow_frac is not None:
        filtered_report()
    if a.scan and a.no_graph:
        scan_report()
        if a.json:
            with open(a.json, "w") as f:
                json.dump(dict(n=n, d=d, nq=nq, k=K, bits=a.bits, rerank_factor=RF, steps=a.steps, rows=rows), f, indent=1)
        quant.close(); full.close()
        return
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
    if a.scan:
        scan_report()
    if not np.array_equal(ids_b, ids_c):
        print("ERROR: the fused ids differ from the composed ids", flush=True)
        sys.exit(1)
    print(f"  fused ids == composed ids; table {n * d * 4 / 2**20:.0f} MiB float / {n * qrow / 2**20:.0f} MiB "
          f"{'four-bit' if a.bits == 4 else 'one-byte'} (Infinity Cache: 256 MiB)", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(n=n, d=d, nq=nq, k=K, beam=beam, bits=a.bits, rerank_factor=RF, steps=a.steps, rows=rows), f, indent=1)
    quant.close(); full.close()


if __name__ == "__main__":
    main()
