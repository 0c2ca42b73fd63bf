"""Masked beam search against the plain search, and against filtering the plain search's answer on the host (DESIGN.md
"Masked search").  The bench.py workload -- 1M x 128 fp16 (datasets.sift1m_like), Vamana R = 64 L = 128 alpha 1.15 two passes,
10 000 queries, beam 64, k = 10 -- with seeded random SHARED masks that allow 100 %, 90 %, 50 % and 10 % of the points.
Per mask, in one process:

  speed            QPS of pann_batch_search_masked_dev beside pann_batch_search_dev (HIP events on a stream of its own; the plain
                   search is timed again next to every mask, so the two columns of a row come from the same minutes)
  recall           recall@10 of the masked result against the exact neighbours AMONG THE ALLOWED POINTS (pann_bruteforce_knn on
                   a compacted index of the allowed rows, ids mapped back)
  baseline recall  recall@10 of the post-filter baseline: the plain search at out_k = beam, disallowed ids thrown away on the
                   host, the first 10 kept

Every step has a time limit, but it is a Python alarm: it ends a step that is slow, not one that hangs inside a native call.
Run the tool under `timeout -k 10 <seconds>` so that a hang ends the process too.

    python tools/masked_time.py [--n 1000000] [--nq 10000] [--steps 20] [--fractions 1.0,0.9,0.5,0.1] [--json out.json]

--rerank: the same question for the fused quantised search with exact rerank (DESIGN.md "Masked search on the fused path").  The
tools/rerank_time.py setup -- 1M x 128 f32 (datasets.deep_like x 2), Vamana R = 64 L = 128, 10 000 resident queries, beam 64,
k = 10, rerank_factor 100 -- with pann_batch_search_rerank_dev and pann_batch_search_masked_rerank_dev timed beside each other
at 100 %, 50 % and 10 % allowed; recall@10 of the masked call against the exact allowed neighbours, and of the post-filter
baseline (the plain fused call at k = 64, disallowed ids thrown away on the host, the first 10 kept).  The fused masked ids must
equal those of the composition (pann_quantize_rows, pann_batch_search_masked with out_k = 64, pann_rerank); the tool stops
otherwise.

    python tools/masked_time.py --rerank [--bits 8|4|8,4] [--fractions 1.0,0.5,0.1] [--json out.json]

--exact: the exact masked kNN beside the masked search on selective masks (DESIGN.md "Exact masked kNN").  The first setup above
with masks that allow 0.1 %, 1 % and 10 % of the points.  Per mask: pann_bruteforce_knn_masked_dev with the shared bitmap, the
same call with the same content as one row per query (nq x ceil(n / 32) words on the device: 1.25 GB at the defaults), and
pann_batch_search_masked_dev at beam 64 -- time (HIP events) and recall@10 of each against the sub-index ground truth above,
whose wall time (upload of the allowed rows + pann_bruteforce_knn) is printed as the yardstick it is.  The shared exact ids
must equal that ground truth; the tool stops otherwise.  Last line: the allowed count at which the shared exact route and the
masked search cost the same, interpolated between the measured masks in log(count).

    python tools/masked_time.py --exact [--fractions 0.001,0.01,0.1] [--json out.json]

--labels: label predicates beside per-query bitmaps (DESIGN.md "Label predicates").  The first setup above; every point gets a
label whose low byte is a tenant in 0..9 and whose second byte is a sub-tenant in 0..9 (the upper half is random), and every
query its own MATCH predicate: one tenant (about 10 % of the points) or one (tenant, sub-tenant) pair (about 1 %).  Per
selectivity, in one process and from one binary: QPS of pann_batch_search_labeled_dev with 10 000 predicates, of
pann_batch_search_masked_dev on the same content as 10 000 bitmap rows (expanded on the device by pann_labels_to_allow_dev: 1.25 GB
at the defaults), and of the plain search; the bytes each form stages per batch; the two id arrays must be equal, the tool stops
otherwise.  With --exact also pann_bruteforce_knn_labeled_dev (one predicate per query: the label scan) beside
pann_bruteforce_knn_masked_dev on the rows, and the time of pann_label_count_dev for the 10 000 predicates.

    python tools/masked_time.py --labels [--exact] [--json out.json]

--labels --exact --grouped: the exact kNN by predicate group (DESIGN.md "Exact kNN by predicate group") on the same data and
predicates -- 10 000 queries that name 10 tenants, or 100 (tenant, sub-tenant) pairs.  No graph is built and nothing is walked.
Per selectivity, in one process: pann_bruteforce_knn_labeled_grouped_dev with the deduplicated table (10 or 100 predicates) and
one table index per query; the per-query label scan and the per-query bitmap scan of --exact; and G sequential calls of the shared
route (pann_bruteforce_knn_labeled_dev with one predicate) over the queries of one table entry each.  HIP events on the stream,
and for the two forms that synchronise also the host's wall time per batch.  The grouped ids must equal the scan's ids; the tool
stops otherwise.

    python tools/masked_time.py --labels --exact --grouped [--json out.json]
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
from parlayann_amd.index import pack_allow  # noqa: E402
from parlayann_amd.recall import recall_at_k  # noqa: E402

K, BEAM, R, L, ALPHA = 10, 64, 64, 128, 1.15
RF = 100          # --rerank: rerank_factor


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
    ap.add_argument("--fractions", default=None, help="default 1.0,0.9,0.5,0.1 (--rerank: 1.0,0.5,0.1)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--rerank", action="store_true", help="the fused quantised search + rerank instead of the plain search")
    ap.add_argument("--bits", default="8", help="--rerank: bits per coordinate of the quantised copy: 8, 4 or 8,4 (one build for both)")
    ap.add_argument("--exact", action="store_true", help="the exact masked kNN beside the masked search on selective masks")
    ap.add_argument("--labels", action="store_true", help="per-query label predicates beside per-query bitmaps (with --exact: on the exact route too)")
    ap.add_argument("--grouped", action="store_true", help="with --labels --exact: the grouped exact route beside the scans; no graph, no walk")
    a = ap.parse_args()
    if a.grouped and not (a.labels and a.exact):
        ap.error("--grouped goes with --labels --exact")
    if a.labels:
        return main_labels(a)
    if a.fractions is None:
        a.fractions = "0.001,0.01,0.1" if a.exact else "1.0,0.5,0.1" if a.rerank else "1.0,0.9,0.5,0.1"
    if a.rerank:
        return main_rerank(a)
    if a.exact:
        return main_exact(a)
    import torch
    n, d, nq = a.n, a.d, a.nq
    with step("data", 300):
        X = datasets.sift1m_like(n, d, seed=1234, dtype=np.float32).astype(np.float16)
        Q = datasets.sift1m_like(nq, d, seed=4321, dtype=np.float16)
    with step(f"upload + build R={R} L={L}", 900):
        ix = DeviceIndex(X, max_degree=R)
        ix.vamana_build(R, L, ALPHA, num_passes=2, seed=1, sort_neighbors=True)
    lib = _capi.load()
    qp = _capi.QueryParams(k=K, beam=BEAM, cut=1.35, limit=n, degree_limit=R, rerank_factor=100, pad=1.0)
    t_q = torch.from_numpy(Q.view(np.uint8).reshape(nq, -1)).cuda()
    t_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    # rows are packed at stride out_k: one pair of buffers per out_k used (k for the timed calls, beam for the baseline)
    t_ids = {ok: torch.zeros((nq, ok), dtype=torch.int32, device="cuda") for ok in (K, BEAM)}
    t_d = {ok: torch.zeros((nq, ok), dtype=torch.float32, device="cuda") for ok in (K, BEAM)}
    t_rc, t_ac, t_dc = (torch.zeros(nq, dtype=torch.int32, device="cuda") for _ in range(3))
    t_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)

    def search_out(out_k):
        return _capi.SearchOut(ids=t_ids[out_k].data_ptr(), dists=t_d[out_k].data_ptr(), out_k=out_k, dist_cmps=t_dc.data_ptr(), status=t_status.data_ptr())

    def plain_step(out_k=K):
        out = search_out(out_k)
        _capi.check(lib.pann_batch_search_dev(ix.handle, C.c_void_p(t_q.data_ptr()), None, nq, 2 * d, C.c_void_p(t_st.data_ptr()), 1,
                                              C.byref(qp), C.byref(out), sp))

    def masked_step(t_allow):
        out = search_out(K)
        _capi.check(lib.pann_batch_search_masked_dev(ix.handle, C.c_void_p(t_q.data_ptr()), None, nq, 2 * d, C.c_void_p(t_st.data_ptr()), 1,
                                                     C.byref(qp), C.c_void_p(t_allow.data_ptr()), 0, C.byref(out),
                                                     C.c_void_p(t_rc.data_ptr()), C.c_void_p(t_ac.data_ptr()), sp))

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
        assert int(t_status.cpu()[0]) == 0
        return ms[len(ms) // 2], ms[0], ms[-1]

    rows = []
    for frac in [float(f) for f in a.fractions.split(",")]:
        allow = np.ones(n, bool) if frac >= 1.0 else np.random.default_rng(int(frac * 1000)).random(n) < frac
        live = np.flatnonzero(allow).astype(np.uint32)
        t_allow = torch.from_numpy(pack_allow(allow, n).view(np.int32)).cuda()
        torch.cuda.synchronize()
        with step(f"allow {frac:.0%}: ground truth over {len(live)} allowed points", 600):
            sub = DeviceIndex(X[live], max_degree=4)
            gt_local, gd = sub.bruteforce_knn(Q, K)
            sub.close()
            gt = live[gt_local]
        with step(f"allow {frac:.0%}: timing", 300):
            p_ms = timed(plain_step)
            m_ms = timed(lambda: masked_step(t_allow))
            ids_m = t_ids[K].cpu().numpy().view(np.uint32).copy()
            rc, ac, dc = (t.cpu().numpy().view(np.uint32).copy() for t in (t_rc, t_ac, t_dc))
            if not allow[ids_m[ids_m != 0xFFFFFFFF]].all():
                print("ERROR: the masked search returned a disallowed id", flush=True)
                sys.exit(1)
        with step(f"allow {frac:.0%}: post-filter baseline", 300):
            plain_step(BEAM); stream.synchronize()
            front = t_ids[BEAM].cpu().numpy().view(np.uint32)
            ids_p = np.full((nq, K), 0xFFFFFFFF, np.uint32)
            for q in range(nq):
                row = front[q][front[q] != 0xFFFFFFFF]
                kept = row[allow[row]][:K]
                ids_p[q, :len(kept)] = kept
        # a padded slot (0xFFFFFFFF) matches no ground-truth id: a short row counts as misses
        row = dict(allow=frac, plain_ms=p_ms[0], plain_ms_min=p_ms[1], plain_ms_max=p_ms[2], masked_ms=m_ms[0], masked_ms_min=m_ms[1],
                   masked_ms_max=m_ms[2], plain_qps=nq / p_ms[0] * 1e3, masked_qps=nq / m_ms[0] * 1e3,
                   recall10_masked=recall_at_k(ids_m, gt, gd, K), recall10_post_filter=recall_at_k(ids_p, gt, gd, K),
                   short_rows=int((rc < K).sum()), allowed_cmps=float(ac.mean()), dist_cmps=float(dc.mean()))
        rows.append(row)
        print(f"  allow {frac:5.0%}  plain {p_ms[0]:8.3f} ms (min {p_ms[1]:.3f}, max {p_ms[2]:.3f}) QPS {row['plain_qps']:9.0f}   "
              f"masked {m_ms[0]:8.3f} ms (min {m_ms[1]:.3f}, max {m_ms[2]:.3f}) QPS {row['masked_qps']:9.0f}  ratio "
              f"{row['masked_qps'] / row['plain_qps']:.3f}   recall@10 masked {row['recall10_masked']:.4f} post-filter "
              f"{row['recall10_post_filter']:.4f}   short rows {row['short_rows']}  allowed cmps/q {row['allowed_cmps']:.1f} of "
              f"{row['dist_cmps']:.1f}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(n=n, d=d, nq=nq, k=K, beam=BEAM, steps=a.steps, rows=rows), f, indent=1)
    ix.close()


def main_exact(a):
    import torch
    n, d, nq = a.n, a.d, a.nq
    with step("data", 300):
        X = datasets.sift1m_like(n, d, seed=1234, dtype=np.float32).astype(np.float16)
        Q = datasets.sift1m_like(nq, d, seed=4321, dtype=np.float16)
    with step(f"upload + build R={R} L={L}", 900):
        ix = DeviceIndex(X, max_degree=R)
        ix.vamana_build(R, L, ALPHA, num_passes=2, seed=1, sort_neighbors=True)
    lib = _capi.load()
    qp = _capi.QueryParams(k=K, beam=BEAM, cut=1.35, limit=n, degree_limit=R, rerank_factor=100, pad=1.0)
    t_q = torch.from_numpy(Q.view(np.uint8).reshape(nq, -1)).cuda()
    t_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    t_ids = torch.zeros((nq, K), dtype=torch.int32, device="cuda")
    t_d = torch.zeros((nq, K), dtype=torch.float32, device="cuda")
    t_cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    t_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    words = (n + 31) // 32

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

    def ids_now():
        return t_ids.cpu().numpy().view(np.uint32).copy()

    rows = []
    for frac in [float(f) for f in a.fractions.split(",")]:
        allow = np.random.default_rng(int(frac * 100000)).random(n) < frac
        live = np.flatnonzero(allow).astype(np.uint32)
        t_allow = torch.from_numpy(pack_allow(allow, n).view(np.int32)).cuda()
        torch.cuda.synchronize()
        with step(f"allow {frac:.1%}: ground truth over {len(live)} allowed points", 600):
            t0 = time.perf_counter()
            sub = DeviceIndex(X[live], max_degree=4)
            gt_local, gd = sub.bruteforce_knn(Q, K)
            sub.close()
            sub_ms = (time.perf_counter() - t0) * 1e3
            gt = np.where(gt_local != 0xFFFFFFFF, live[np.minimum(gt_local, len(live) - 1)], 0xFFFFFFFF).astype(np.uint32)

        def exact_step(t_bits, stride):
            ix.bruteforce_knn_masked_dev(t_q.data_ptr(), nq, 2 * d, K, t_bits.data_ptr(), stride, t_ids.data_ptr(), t_d.data_ptr(),
                                         t_cnt.data_ptr(), stream.cuda_stream)

        def masked_step():
            out = _capi.SearchOut(ids=t_ids.data_ptr(), dists=t_d.data_ptr(), out_k=K, status=t_status.data_ptr())
            _capi.check(lib.pann_batch_search_masked_dev(ix.handle, C.c_void_p(t_q.data_ptr()), None, nq, 2 * d, C.c_void_p(t_st.data_ptr()), 1,
                                                         C.byref(qp), C.c_void_p(t_allow.data_ptr()), 0, C.byref(out), None, None,
                                                         C.c_void_p(stream.cuda_stream)))

        with step(f"allow {frac:.1%}: shared exact route", 300):
            s_ms = timed(lambda: exact_step(t_allow, 0))
            ids_s = ids_now()
            if not np.array_equal(ids_s, gt):
                print("ERROR: the shared exact ids differ from the sub-index ground truth", flush=True)
                sys.exit(1)
        with step(f"allow {frac:.1%}: per-query exact route", 300):
            t_rows = t_allow.repeat(nq, 1)
            torch.cuda.synchronize()
            r_ms = timed(lambda: exact_step(t_rows, words))
            ids_r = ids_now()
            del t_rows
        with step(f"allow {frac:.1%}: masked search, beam {BEAM}", 300):
            m_ms = timed(masked_step)
            assert int(t_status.cpu()[0]) == 0
            ids_m = ids_now()
        row = dict(allow=frac, allowed=int(len(live)), sub_index_wall_ms=sub_ms, shared_ms=s_ms[0], shared_ms_min=s_ms[1],
                   shared_ms_max=s_ms[2], rows_ms=r_ms[0], rows_ms_min=r_ms[1], rows_ms_max=r_ms[2], masked_ms=m_ms[0],
                   masked_ms_min=m_ms[1], masked_ms_max=m_ms[2], recall10_shared=recall_at_k(ids_s, gt, gd, K),
                   recall10_rows=recall_at_k(ids_r, gt, gd, K), recall10_masked=recall_at_k(ids_m, gt, gd, K))
        rows.append(row)
        print(f"  allow {frac:6.1%} ({len(live):7d} points)  sub-index ground truth {sub_ms:9.1f} ms wall   exact shared {s_ms[0]:9.3f} ms "
              f"(min {s_ms[1]:.3f}, max {s_ms[2]:.3f}) recall@10 {row['recall10_shared']:.4f}   exact per-query {r_ms[0]:9.3f} ms "
              f"(min {r_ms[1]:.3f}, max {r_ms[2]:.3f}) recall@10 {row['recall10_rows']:.4f}   masked beam {BEAM} {m_ms[0]:9.3f} ms "
              f"(min {m_ms[1]:.3f}, max {m_ms[2]:.3f}) recall@10 {row['recall10_masked']:.4f}   shared exact ids == ground truth", flush=True)
    # where the shared exact route and the masked search cost the same: log-linear between the two masks around the sign change
    rows_sorted = sorted(rows, key=lambda r: r["allowed"])
    diff = [r["shared_ms"] - r["masked_ms"] for r in rows_sorted]
    cross = None
    for lo, hi, d0, d1 in zip(rows_sorted, rows_sorted[1:], diff, diff[1:]):
        if d0 <= 0 < d1:
            t = d0 / (d0 - d1)
            cross = float(np.exp(np.log(lo["allowed"]) + t * (np.log(hi["allowed"]) - np.log(lo["allowed"]))))
    if cross is not None:
        print(f"  equal cost at about {cross:.0f} allowed points ({cross / n:.2%} of {n}): below it the shared exact route is faster", flush=True)
    elif all(x <= 0 for x in diff):
        print(f"  the shared exact route was faster at every mask measured (up to {rows_sorted[-1]['allowed']} allowed points)", flush=True)
    else:
        print(f"  the masked search was faster at every mask measured (down to {rows_sorted[0]['allowed']} allowed points)", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(n=n, d=d, nq=nq, k=K, beam=BEAM, steps=a.steps, equal_cost_allowed=cross, rows=rows), f, indent=1)
    ix.close()


def main_labels(a):
    import torch
    n, d, nq = a.n, a.d, a.nq
    with step("data", 300):
        X = datasets.sift1m_like(n, d, seed=1234, dtype=np.float32).astype(np.float16)
        Q = datasets.sift1m_like(nq, d, seed=4321, dtype=np.float16)
        rng = np.random.default_rng(77)
        labels = (rng.integers(0, 10, n).astype(np.uint32) | (rng.integers(0, 10, n).astype(np.uint32) << np.uint32(8))
                  | (rng.integers(0, 1 << 16, n).astype(np.uint32) << np.uint32(16)))
    with step(f"upload + build R={R} L={L}", 900):
        ix = DeviceIndex(X, max_degree=4 if a.grouped else R)
        if not a.grouped:
            ix.vamana_build(R, L, ALPHA, num_passes=2, seed=1, sort_neighbors=True)
        ix.set_labels(labels)
    lib = _capi.load()
    qp = _capi.QueryParams(k=K, beam=BEAM, cut=1.35, limit=n, degree_limit=R, rerank_factor=100, pad=1.0)
    words = (n + 31) // 32
    t_q = torch.from_numpy(Q.view(np.uint8).reshape(nq, -1)).cuda()
    t_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    t_ids = torch.zeros((nq, K), dtype=torch.int32, device="cuda")
    t_d = torch.zeros((nq, K), dtype=torch.float32, device="cuda")
    t_rc, t_ac, t_dc, t_cnt = (torch.zeros(nq, dtype=torch.int32, device="cuda") for _ in range(4))
    t_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    t_rows = torch.zeros((nq, words), dtype=torch.int32, device="cuda")          # the per-query bitmaps: nq * ceil(n / 32) words
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())

    def search_out():
        return _capi.SearchOut(ids=t_ids.data_ptr(), dists=t_d.data_ptr(), out_k=K, dist_cmps=t_dc.data_ptr(), status=t_status.data_ptr())

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
        assert int(t_status.cpu()[0]) == 0
        return ms[len(ms) // 2], ms[0], ms[-1]

    def wall(fn):
        """median host time of a call that synchronises: from a drained stream to a drained stream"""
        out = []
        for _ in range(a.steps):
            stream.synchronize()
            t0 = time.perf_counter()
            fn()
            stream.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return sorted(out)[len(out) // 2]

    def ids_now():
        return t_ids.cpu().numpy().view(np.uint32).copy()

    qn = np.arange(nq, dtype=np.uint32)
    sets = [("tenant (about 10 %)", np.stack([np.full(nq, 0xFF, np.uint32), qn % 10], axis=1)),
            ("tenant and sub-tenant (about 1 %)", np.stack([np.full(nq, 0xFFFF, np.uint32), (qn % 10) | ((qn // 10 % 10) << 8)], axis=1))]
    rows = []
    for name, preds in sets:
        preds = np.ascontiguousarray(preds.astype(np.uint32))
        t_p = torch.from_numpy(preds.view(np.int32)).cuda()
        torch.cuda.synchronize()

        def plain_step():
            out = search_out()
            _capi.check(lib.pann_batch_search_dev(ix.handle, vp(t_q), None, nq, 2 * d, vp(t_st), 1, C.byref(qp), C.byref(out), sp))

        def labeled_step():
            out = search_out()
            _capi.check(lib.pann_batch_search_labeled_dev(ix.handle, vp(t_q), None, nq, 2 * d, vp(t_st), 1, C.byref(qp), _capi.PANN_PRED_MATCH,
                                                          vp(t_p), nq, C.byref(out), vp(t_rc), vp(t_ac), sp))

        def bitmap_step():
            out = search_out()
            _capi.check(lib.pann_batch_search_masked_dev(ix.handle, vp(t_q), None, nq, 2 * d, vp(t_st), 1, C.byref(qp), vp(t_rows), words,
                                                         C.byref(out), vp(t_rc), vp(t_ac), sp))

        def expand_step():
            _capi.check(lib.pann_labels_to_allow_dev(ix.handle, _capi.PANN_PRED_MATCH, vp(t_p), nq, vp(t_rows), words, sp))

        def count_step():
            _capi.check(lib.pann_label_count_dev(ix.handle, _capi.PANN_PRED_MATCH, vp(t_p), nq, vp(t_cnt), sp))

        if a.grouped:
            rows.append(grouped_rows(a, name, preds, lib, ix, labels, t_q, t_p, t_rows, t_ids, t_d, t_cnt, stream, timed, wall, ids_now))
            continue
        with step(f"{name}: expand to {nq} bitmap rows on the device, count", 300):
            x_ms = timed(expand_step)
            c_ms = timed(count_step)
            cnt = t_cnt.cpu().numpy().view(np.uint32)
            want = np.bincount((labels & np.uint32(preds[0, 0])).astype(np.int64), minlength=1 << 16)[preds[:, 1]]
            if not np.array_equal(cnt, want):
                print("ERROR: pann_label_count_dev differs from the host count", flush=True)
                sys.exit(1)
        with step(f"{name}: timing", 300):
            p_ms = timed(plain_step)
            l_ms = timed(labeled_step)
            ids_l = ids_now()
            rc, ac, dc = (t.cpu().numpy().view(np.uint32).copy() for t in (t_rc, t_ac, t_dc))
            b_ms = timed(bitmap_step)
            if not np.array_equal(ids_now(), ids_l):
                print("ERROR: the labeled ids differ from the bitmap entry's", flush=True)
                sys.exit(1)
            real = ids_l != 0xFFFFFFFF
            if not ((labels[ids_l[real]] & preds[np.nonzero(real)[0], 0]) == preds[np.nonzero(real)[0], 1]).all():
                print("ERROR: the labeled search returned a point its predicate does not allow", flush=True)
                sys.exit(1)
        row = dict(predicates=name, allowed_mean=float(cnt.mean()), plain_ms=p_ms[0], labeled_ms=l_ms[0], labeled_ms_min=l_ms[1],
                   labeled_ms_max=l_ms[2], bitmap_ms=b_ms[0], bitmap_ms_min=b_ms[1], bitmap_ms_max=b_ms[2], plain_qps=nq / p_ms[0] * 1e3,
                   labeled_qps=nq / l_ms[0] * 1e3, bitmap_qps=nq / b_ms[0] * 1e3, labeled_bytes_per_batch=8 * nq,
                   bitmap_bytes_per_batch=4 * words * nq, expand_ms=x_ms[0], count_ms=c_ms[0], short_rows=int((rc < K).sum()),
                   allowed_cmps=float(ac.mean()), dist_cmps=float(dc.mean()))
        print(f"  {name}: {row['allowed_mean']:.0f} allowed points per query   plain {p_ms[0]:.3f} ms QPS {row['plain_qps']:.0f}   labeled "
              f"{l_ms[0]:.3f} ms (min {l_ms[1]:.3f}, max {l_ms[2]:.3f}) QPS {row['labeled_qps']:.0f}   per-query bitmaps {b_ms[0]:.3f} ms (min "
              f"{b_ms[1]:.3f}, max {b_ms[2]:.3f}) QPS {row['bitmap_qps']:.0f}   labeled / bitmap {row['labeled_qps'] / row['bitmap_qps']:.3f}   "
              f"staged per batch: {row['labeled_bytes_per_batch']} B of predicates against {row['bitmap_bytes_per_batch']} B of bitmap rows   "
              f"expanding the rows {x_ms[0]:.3f} ms, counting {c_ms[0]:.3f} ms   rows shorter than k {row['short_rows']}  allowed cmps/q "
              f"{row['allowed_cmps']:.1f} of {row['dist_cmps']:.1f}   labeled ids == bitmap ids", flush=True)
        if a.exact:
            with step(f"{name}: exact routes", 600):
                e_l = timed(lambda: _capi.check(lib.pann_bruteforce_knn_labeled_dev(ix.handle, vp(t_q), nq, 2 * d, K, _capi.PANN_PRED_MATCH,
                                                                                  vp(t_p), nq, vp(t_ids), vp(t_d), vp(t_cnt), sp)))
                ids_el = ids_now()
                e_b = timed(lambda: ix.bruteforce_knn_masked_dev(t_q.data_ptr(), nq, 2 * d, K, t_rows.data_ptr(), words, t_ids.data_ptr(),
                                                                 t_d.data_ptr(), t_cnt.data_ptr(), stream.cuda_stream))
                if not np.array_equal(ids_now(), ids_el):
                    print("ERROR: the labeled exact ids differ from the per-query bitmap route's", flush=True)
                    sys.exit(1)
            row.update(exact_labeled_ms=e_l[0], exact_labeled_ms_min=e_l[1], exact_labeled_ms_max=e_l[2], exact_bitmap_ms=e_b[0],
                       exact_bitmap_ms_min=e_b[1], exact_bitmap_ms_max=e_b[2])
            print(f"  {name}: exact, one predicate per query {e_l[0]:.3f} ms (min {e_l[1]:.3f}, max {e_l[2]:.3f})   exact, per-query bitmaps "
                  f"{e_b[0]:.3f} ms (min {e_b[1]:.3f}, max {e_b[2]:.3f})   ids equal", flush=True)
        rows.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(n=n, d=d, nq=nq, k=K, beam=BEAM, steps=a.steps, rows=rows), f, indent=1)
    ix.close()


def grouped_rows(a, name, preds, lib, ix, labels, t_q, t_p, t_rows, t_ids, t_d, t_cnt, stream, timed, wall, ids_now):
    """--labels --exact --grouped, one selectivity: the grouped call, the two scans, G sequential shared-route calls"""
    import torch
    n, d, nq = a.n, a.d, a.nq
    words = (n + 31) // 32
    sp = C.c_void_p(stream.cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())
    table, group = np.unique(preds, axis=0, return_inverse=True)
    table = np.ascontiguousarray(table.astype(np.uint32))
    group = np.ascontiguousarray(group.reshape(-1).astype(np.uint32))
    G = len(table)
    t_tab, t_grp = torch.from_numpy(table.view(np.int32)).cuda(), torch.from_numpy(group.view(np.int32)).cuda()
    # the sequential form: the queries of a table entry side by side, one shared-route call per entry
    order = np.argsort(group, kind="stable")
    first = np.concatenate([[0], np.cumsum(np.bincount(group, minlength=G))])
    t_qs = t_q[torch.from_numpy(order).cuda()].contiguous()
    t_ids_s, t_d_s, t_cnt_s = torch.zeros_like(t_ids), torch.zeros_like(t_d), torch.zeros_like(t_cnt)
    torch.cuda.synchronize()
    qb = 2 * d

    def grouped_step():
        _capi.check(lib.pann_bruteforce_knn_labeled_grouped_dev(ix.handle, vp(t_q), nq, qb, K, _capi.PANN_PRED_MATCH, vp(t_tab), G, vp(t_grp), 0,
                                                                vp(t_ids), vp(t_d), vp(t_cnt), sp))

    def sequential_step():
        for g in range(G):
            lo, m = int(first[g]), int(first[g + 1] - first[g])
            if m:
                _capi.check(lib.pann_bruteforce_knn_labeled_dev(ix.handle, C.c_void_p(t_qs.data_ptr() + lo * qb), m, qb, K, _capi.PANN_PRED_MATCH,
                                                                C.c_void_p(t_tab.data_ptr() + 8 * g), 1, C.c_void_p(t_ids_s.data_ptr() + lo * K * 4),
                                                                C.c_void_p(t_d_s.data_ptr() + lo * K * 4), C.c_void_p(t_cnt_s.data_ptr() + lo * 4), sp))

    with step(f"{name}: grouped, scans, {G} sequential shared calls", 900):
        _capi.check(lib.pann_labels_to_allow_dev(ix.handle, _capi.PANN_PRED_MATCH, vp(t_p), nq, vp(t_rows), words, sp))
        g_ms = timed(grouped_step)
        g_wall = wall(grouped_step)
        ids_g = ids_now()
        cnt_g = t_cnt.cpu().numpy().view(np.uint32).copy()
        s_ms = timed(sequential_step)
        s_wall = wall(sequential_step)
        ids_s = t_ids_s.cpu().numpy().view(np.uint32)
        e_l = timed(lambda: _capi.check(lib.pann_bruteforce_knn_labeled_dev(ix.handle, vp(t_q), nq, qb, K, _capi.PANN_PRED_MATCH, vp(t_p), nq,
                                                                          vp(t_ids), vp(t_d), vp(t_cnt), sp)))
        ids_el = ids_now()
        e_b = timed(lambda: ix.bruteforce_knn_masked_dev(t_q.data_ptr(), nq, qb, K, t_rows.data_ptr(), words, t_ids.data_ptr(), t_d.data_ptr(),
                                                         t_cnt.data_ptr(), stream.cuda_stream))
        if not np.array_equal(ids_g, ids_el) or not np.array_equal(ids_now(), ids_el):
            print("ERROR: the grouped ids differ from the per-query scan's", flush=True)
            sys.exit(1)
        if not np.array_equal(ids_s, ids_g[order]):
            print("ERROR: the sequential shared-route ids differ from the grouped ids", flush=True)
            sys.exit(1)
    allowed = np.array([int(((labels & t[0]) == t[1]).sum()) for t in table])
    if not np.array_equal(cnt_g, np.minimum(allowed[group], K)):
        print("ERROR: the grouped counts differ from the host count", flush=True)
        sys.exit(1)
    row = dict(predicates=name, distinct=G, allowed_mean=float(allowed[group].mean()),
               grouped_ms=g_ms[0], grouped_ms_min=g_ms[1], grouped_ms_max=g_ms[2], grouped_wall_ms=g_wall, sequential_ms=s_ms[0],
               sequential_ms_min=s_ms[1], sequential_ms_max=s_ms[2], sequential_wall_ms=s_wall, exact_labeled_ms=e_l[0],
               exact_labeled_ms_min=e_l[1], exact_labeled_ms_max=e_l[2], exact_bitmap_ms=e_b[0], exact_bitmap_ms_min=e_b[1],
               exact_bitmap_ms_max=e_b[2])
    print(f"  {name}: {G} distinct predicates, {row['allowed_mean']:.0f} allowed points per query   grouped {g_ms[0]:.3f} ms (min {g_ms[1]:.3f}, "
          f"max {g_ms[2]:.3f}; host wall {g_wall:.3f})   {G} sequential shared calls {s_ms[0]:.3f} ms (min {s_ms[1]:.3f}, max {s_ms[2]:.3f}; host "
          f"wall {s_wall:.3f})   label scan {e_l[0]:.3f} ms (min {e_l[1]:.3f}, max {e_l[2]:.3f})   bitmap scan {e_b[0]:.3f} ms (min "
          f"{e_b[1]:.3f}, max {e_b[2]:.3f})   grouped ids == scan ids == sequential ids", flush=True)
    return row


def main_rerank(a):
    import torch
    n, d, nq = a.n, a.d, a.nq
    bits_list = [int(b) for b in a.bits.split(",")]
    assert all(b in (8, 4) for b in bits_list)
    with step("data", 300):                       # real-valued, so that the quantiser is not the identity
        X = (datasets.deep_like(n, d, seed=1) * 2.0).astype(np.float32)
        Q = (datasets.deep_like(nq, d, seed=2) * 2.0).astype(np.float32)
    with step(f"upload + build R={R} L={L}", 900):
        full = DeviceIndex(X, max_degree=R, metric="Euclidian")
        full.vamana_build(R, L, 1.2, num_passes=1, seed=3)
    t_q = torch.from_numpy(Q).cuda()
    t_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    t_ids = {k: torch.zeros((nq, k), dtype=torch.int32, device="cuda") for k in (K, BEAM)}
    t_d = {k: torch.zeros((nq, k), dtype=torch.float32, device="cuda") for k in (K, BEAM)}
    t_rc, t_ac, t_dc = (torch.zeros(nq, dtype=torch.int32, device="cuda") for _ in range(3))
    t_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()

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
        assert int(t_status.cpu()[0]) == 0
        return ms[len(ms) // 2], ms[0], ms[-1]

    truth = {}          # fraction -> (allow, gt ids, gt dists): shared by the bit widths
    out = []
    for bits in bits_list:
        with step(f"quantise to {bits} bits", 120):
            quant, qparams = full.quantized("euclid_u8" if bits == 8 else "euclid_u4")
            assert not qparams.identity

        def fused_step(k=K, t_allow=None):
            kw = {} if t_allow is None else dict(d_allow_ptr=t_allow.data_ptr(), allow_stride_words=0, d_result_count_ptr=t_rc.data_ptr(),
                                                 d_allowed_cmps_ptr=t_ac.data_ptr())
            full.search_rerank_dev(quant, qparams, t_q.data_ptr(), nq, 4 * d, t_st.data_ptr(), 1, t_ids[k].data_ptr(), t_d[k].data_ptr(),
                                   k=k, beam=BEAM, limit=n, degree_limit=R, rerank_factor=RF, d_dist_cmps_ptr=t_dc.data_ptr(),
                                   d_status_ptr=t_status.data_ptr(), stream_ptr=stream.cuda_stream, **kw)

        rows = []
        for frac in [float(f) for f in a.fractions.split(",")]:
            if frac not in truth:
                allow = np.ones(n, bool) if frac >= 1.0 else np.random.default_rng(int(frac * 1000)).random(n) < frac
                live = np.flatnonzero(allow).astype(np.uint32)
                with step(f"allow {frac:.0%}: ground truth over {len(live)} allowed points", 600):
                    sub = DeviceIndex(X[live], max_degree=4)
                    gt_local, gd = sub.bruteforce_knn(Q, K)
                    sub.close()
                truth[frac] = (allow, live[gt_local], gd)
            allow, gt, gd = truth[frac]
            packed = pack_allow(allow, n)
            t_allow = torch.from_numpy(packed.view(np.int32)).cuda()
            torch.cuda.synchronize()
            with step(f"{bits} bits, allow {frac:.0%}: timing", 300):
                p_ms = timed(fused_step)
                m_ms = timed(lambda: fused_step(K, t_allow))
                ids_m = t_ids[K].cpu().numpy().view(np.uint32).copy()
                rc, ac, dc = (t.cpu().numpy().view(np.uint32).copy() for t in (t_rc, t_ac, t_dc))
                if not allow[ids_m[ids_m != 0xFFFFFFFF]].all():
                    print("ERROR: the fused masked search returned a disallowed id", flush=True)
                    sys.exit(1)
            with step(f"{bits} bits, allow {frac:.0%}: composition", 300):
                qq = quantize.device_quantize_rows(Q, qparams)
                r = quant.batch_search_masked(qq, allow=packed, k=K, beam=BEAM, out_k=BEAM, limit=n, degree_limit=R)
                ids_c, _ = full.rerank(Q, r["ids"], r["result_count"], K, resort=True)
                ids_c[np.arange(K)[None, :] >= r["result_count"][:, None]] = 0xFFFFFFFF
                if not np.array_equal(ids_c, ids_m):
                    print("ERROR: the fused masked ids differ from the composition's", flush=True)
                    sys.exit(1)
            with step(f"{bits} bits, allow {frac:.0%}: post-filter baseline", 300):
                fused_step(BEAM); stream.synchronize()
                front = t_ids[BEAM].cpu().numpy().view(np.uint32)
                ids_p = np.full((nq, K), 0xFFFFFFFF, np.uint32)
                for q in range(nq):
                    row = front[q][front[q] != 0xFFFFFFFF]
                    kept = row[allow[row]][:K]
                    ids_p[q, :len(kept)] = kept
            row = dict(bits=bits, allow=frac, plain_ms=p_ms[0], plain_ms_min=p_ms[1], plain_ms_max=p_ms[2], masked_ms=m_ms[0],
                       masked_ms_min=m_ms[1], masked_ms_max=m_ms[2], plain_qps=nq / p_ms[0] * 1e3, masked_qps=nq / m_ms[0] * 1e3,
                       recall10_masked=recall_at_k(ids_m, gt, gd, K), recall10_post_filter=recall_at_k(ids_p, gt, gd, K),
                       short_rows=int((rc < K).sum()), result_count=float(rc.mean()), allowed_cmps=float(ac.mean()),
                       dist_cmps=float(dc.mean()))
            rows.append(row)
            print(f"  {bits} bits  allow {frac:5.0%}  fused plain {p_ms[0]:8.3f} ms (min {p_ms[1]:.3f}, max {p_ms[2]:.3f}) QPS "
                  f"{row['plain_qps']:9.0f}   fused masked {m_ms[0]:8.3f} ms (min {m_ms[1]:.3f}, max {m_ms[2]:.3f}) QPS "
                  f"{row['masked_qps']:9.0f}  ratio {row['masked_qps'] / row['plain_qps']:.3f}   recall@10 masked "
                  f"{row['recall10_masked']:.4f} post-filter {row['recall10_post_filter']:.4f}   rows shorter than k "
                  f"{row['short_rows']}  list {row['result_count']:.1f}  allowed cmps/q {row['allowed_cmps']:.1f} of "
                  f"{row['dist_cmps']:.1f}   fused masked ids == composition", flush=True)
        out.extend(rows)
        quant.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(n=n, d=d, nq=nq, k=K, beam=BEAM, rerank_factor=RF, steps=a.steps, rows=out), f, indent=1)
    full.close()


if __name__ == "__main__":
    main()
