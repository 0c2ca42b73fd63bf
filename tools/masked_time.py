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
from parlayann_amd.index import pack_allow  # noqa: E402
from parlayann_amd.recall import recall_at_k  # noqa: E402

K, BEAM, R, L, ALPHA = 10, 64, 64, 128, 1.15


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
    ap.add_argument("--fractions", default="1.0,0.9,0.5,0.1")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
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


if __name__ == "__main__":
    main()
