"""Stream order of the steered device entries (pann_batch_search_steered_dev, pann_batch_search_steered_labeled_dev; DESIGN.md
"Stream order", "Steered masked search") with the busy-stream harness of tests/stream_order.py: both calls are enqueued behind a
delay kernel on the caller's stream while their buffers still hold decoys -- other queries, a bitmap that allows everything,
other predicates -- and their outputs poison.  Whatever the library put on another stream, or did before the stream reached it,
shows as different bytes; a call that synchronised shows as a late return."""
import ctypes as C

import numpy as np
import pytest

import steered_cases as sc
import stream_order as so
from parlayann_amd import DeviceIndex, _capi

pytestmark = pytest.mark.gpu

FIELDS = ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum", "result_count", "allowed_cmps")


def test_steered_dev_entries_behind_a_busy_stream():
    import torch
    lib = _capi.load()
    dev = torch.device("cuda", 0)
    X, Q, metric = sc.layout_data("f16")
    T, beam, fill, nq, ok = 20, 64, 8, sc.NQ, 10
    m = sc.mask(T, True)
    lab, preds = sc.labels_of(T, "match", True)
    ix = DeviceIndex(X, sc.graph("f16", 32), metric=metric)
    try:
        ix.set_labels(lab)
        kw = dict(k=10, beam=beam, out_k=ok, cut=1.35)
        want = ix.batch_search_masked(Q, allow=sc.pack(m), steer=fill, **kw)           # the host entry: also warms the workspace
        assert want["bridge_rows"].sum() > 0
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        real_q, decoy_q = up(Q.view(np.uint8).reshape(nq, -1)), up(Q[::-1].copy().view(np.uint8).reshape(nq, -1))
        real_a, decoy_a = up(sc.pack(m).view(np.int32)), up(np.full((nq, sc.WORDS), -1, np.int32))
        real_p, decoy_p = up(preds.view(np.int32)), up(np.zeros((nq, 2), np.int32))      # MATCH a = 0, b = 0 allows every point
        t_st = torch.zeros(1, dtype=torch.int32, device=dev)
        q_buf, a_buf, p_buf = decoy_q.clone(), decoy_a.clone(), decoy_p.clone()
        stream = torch.cuda.Stream(device=dev)
        assert stream.cuda_stream != 0

        def outputs():
            return {"ids": torch.zeros((nq, ok), dtype=torch.int32, device=dev), "dists": torch.zeros((nq, ok), dtype=torch.float32, device=dev),
                    **{f: torch.zeros(nq, dtype=torch.int32, device=dev) for f in FIELDS[2:]},
                    "steer": torch.zeros((nq, 2), dtype=torch.int32, device=dev), "status": torch.zeros(1, dtype=torch.int32, device=dev)}

        o1, o2 = outputs(), outputs()
        qp = _capi.QueryParams(k=10, beam=beam, cut=1.35, limit=sc.N, degree_limit=32, rerank_factor=100, pad=1.0)
        vp = lambda t: C.c_void_p(t.data_ptr())
        mk_out = lambda o: _capi.SearchOut(ids=o["ids"].data_ptr(), dists=o["dists"].data_ptr(), out_k=ok, frontier_size=o["frontier_size"].data_ptr(),
                                           visited_count=o["visited_count"].data_ptr(), dist_cmps=o["dist_cmps"].data_ptr(),
                                           degree_sum=o["degree_sum"].data_ptr(), status=o["status"].data_ptr())
        so1, so2 = mk_out(o1), mk_out(o2)
        sp = C.c_void_p(stream.cuda_stream)
        calls = [
            lambda: _capi.check(lib.pann_batch_search_steered_dev(ix.handle, vp(q_buf), None, nq, q_buf.shape[1], vp(t_st), 1, C.byref(qp), vp(a_buf),
                                                                  sc.WORDS, C.byref(so1), vp(o1["result_count"]), vp(o1["allowed_cmps"]), fill,
                                                                  vp(o1["steer"]), sp)),
            lambda: _capi.check(lib.pann_batch_search_steered_labeled_dev(ix.handle, vp(q_buf), None, nq, q_buf.shape[1], vp(t_st), 1, C.byref(qp),
                                                                          _capi.PANN_PRED_MATCH, vp(p_buf), nq, C.byref(so2),
                                                                          vp(o2["result_count"]), vp(o2["allowed_cmps"]), fill, vp(o2["steer"]), sp)),
        ]
        early = so.run_behind_delay(stream, [(q_buf, real_q), (a_buf, real_a), (p_buf, real_p)],
                                    [t for o in (o1, o2) for t in o.values()], calls)
        assert early, "a steered _dev entry synchronised with the caller's stream"
        for name, o in (("bitmap", o1), ("labeled", o2)):
            assert int(o["status"].cpu()[0]) == 0
            for f in FIELDS:
                np.testing.assert_array_equal(o[f].cpu().numpy().view(want[f].dtype), want[f], err_msg=f"{name} {f}")
            st = o["steer"].cpu().numpy().view(np.uint32)
            np.testing.assert_array_equal(st[:, 0], want["bridge_rows"], err_msg=name)
            np.testing.assert_array_equal(st[:, 1], want["hop2_cmps"], err_msg=name)
    finally:
        ix.close()
