"""pann_batch_search_labeled_rerank / _dev (DESIGN.md "Label predicates"): the fused quantised search + exact rerank with label
predicates in place of the allow bitmap.  On an f32 handle with a u8 copy and with a u4 copy the fused labeled call must equal,
bit for bit and field for field,
    pann_batch_search_masked_rerank with the expanded rows { i : pred_q(label[i]) }, and
    the three-step host sequence that entry is defined by: pann_quantize_rows -> pann_batch_search_masked on the quantised copy
    with out_k = pool -> pann_rerank on the float handle with counts = result_count, resort = 1;
in exact-float-order mode it must equal the CPU restatement (tests/masked_ref.py on label_allow(...) over the oracle's
quantised rows, oracle distances for the rerank).  The labels are the FLOAT handle's: the copy has none, and labels put on the
copy afterwards change nothing."""
import ctypes as C

import numpy as np
import pytest

import label_cases as lc
import masked_ref
import masked_rerank_cases as rc
from parlayann_amd import DeviceIndex, PannError, _capi, quantize
from parlayann_amd.index import label_allow

pytestmark = pytest.mark.gpu

N, NQ, R = rc.N, rc.NQ, rc.R
SENT = rc.SENT
FIELDS = ("ids", "dists", "result_count", "allowed_cmps", "frontier_size", "visited_count", "dist_cmps")
assert (N, NQ) == (lc.N, lc.NQ)
# (beam, k, rerank_factor): pool 16 / 64 / 6; beam 100: the generic kernel
SWEEP = [(16, 10, 100), (64, 10, 100), (64, 2, 3), (100, 10, 100)]
PREDICATES = ["tenant", "tenant-shared", "range-rows", "range-straddle", "match-none", "match-all"]


class Case:
    """an f32 index with the graph of tests/masked_rerank_cases.py (the oracle's, or built on the device) and its quantised copy"""

    def __init__(self, name):
        d, metric, bits = rc.DATASETS[name]
        assert metric == "l2"
        self.name = name
        self.X, self.Q = rc.data(name)
        if name in rc.RESTATED:
            self.full = DeviceIndex(self.X, rc.graph(name))
        else:
            self.full = DeviceIndex(self.X, max_degree=R)
            self.full.vamana_build(R, rc.L, 1.2, num_passes=1, seed=5)
        self.quant, self.qparams = self.full.quantized("euclid_u" + str(bits))
        assert bits == 4 or not self.qparams.identity

    def fused(self, k, beam, rf, **kw):
        return self.full.search_rerank(self.quant, self.qparams, self.Q, k=k, beam=beam, rerank_factor=rf, **kw)

    def compose(self, k, beam, rf, allow):
        pool = rc.pool(beam, k, rf)
        qq = quantize.device_quantize_rows(self.Q, self.qparams)
        r = self.quant.batch_search_masked(qq, allow=allow, k=k, beam=beam, out_k=pool)
        ids, dists = self.full.rerank(self.Q, r["ids"], r["result_count"], k, resort=True)
        pad = np.arange(k)[None, :] >= r["result_count"][:, None]
        ids[pad] = SENT; dists[pad] = np.inf
        exp = {"ids": ids, "dists": dists}
        for f in FIELDS[2:]:
            exp[f] = r[f]
        return exp

    def close(self):
        self.full.close(); self.quant.close()


@pytest.fixture(scope="module")
def cases():
    built = {}

    def get(name):
        if name not in built:
            built[name] = Case(name)
        return built[name]
    yield get
    for c in built.values():
        c.close()


def _same(got, exp, msg=""):
    for f in FIELDS:
        assert got[f].dtype == exp[f].dtype and np.array_equal(got[f].view(np.uint32), exp[f].view(np.uint32)), (msg, f)


@pytest.mark.parametrize("name", ["l2_64", "l2_128_u4"])         # a u8 copy and a u4 copy, both on the beam-64 route at beam <= 64
def test_fused_labeled_equals_the_bitmap_entry_and_the_three_steps(cases, name):
    c = cases(name)
    assert not c.quant.has_labels
    for pname in PREDICATES:
        labels, kind, preds, claim = lc.CASES[pname]
        c.full.set_labels(labels)
        rows = np.broadcast_to(label_allow(labels, kind, preds), (NQ, N))
        packed = rc.pack(rows)                                    # the 7 dead bits of the last word set
        for beam, k, rf in SWEEP:
            got = c.fused(k, beam, rf, where=(kind, preds))
            _same(got, c.fused(k, beam, rf, allow=packed), msg=(pname, beam, "bitmap entry"))
            _same(got, c.compose(k, beam, rf, packed), msg=(pname, beam, "three steps"))
            assert int(got["status"][0]) == 0                     # a short row raises no SHORT_FRONTIER
            real = got["ids"] != SENT
            assert rows[np.nonzero(real)[0], got["ids"][real]].all()
            if claim == "none":
                assert (got["result_count"] == 0).all() and not real.any()
            if claim == "all":
                assert (got["result_count"] == rc.pool(beam, k, rf)).all()
        if np.asarray(preds).ndim == 1:                           # the same predicate once per query
            _same(c.fused(10, 64, 100, where=(kind, lc.preds_rows(preds))), c.fused(10, 64, 100, where=(kind, preds)), msg=pname)
    # quant's own labels are not consulted
    labels, kind, preds, _ = lc.CASES["tenant"]
    c.full.set_labels(labels)
    before = c.fused(10, 64, 100, where=(kind, preds))
    c.quant.set_labels(~labels)
    try:
        _same(c.fused(10, 64, 100, where=(kind, preds)), before, msg="labels on the copy")
    finally:
        c.quant.drop_labels()


def test_exact_order_equals_the_restatement(cases, oracle):
    """the independent reference: masked_ref on the oracle's quantised rows with the expanded mask, oracle distances, (dist, id)"""
    c = cases("l2_64")
    _capi.check(c.full._lib.pann_index_set_exact_float_order(c.full.handle, 1))
    try:
        slope, offset, Xq, Qq = rc.quantised("l2_64")
        assert (np.float32(c.qparams.slope), int(c.qparams.offset)) == (slope, offset)
        for pname, beam, k, rf in (("tenant", 64, 10, 100), ("range-rows", 16, 10, 100), ("range-straddle", 100, 10, 100)):
            labels, kind, preds, _ = lc.CASES[pname]
            c.full.set_labels(labels)
            allow = label_allow(labels, kind, preds)
            ref = masked_ref.masked_batch_search(Xq, rc.graph("l2_64"), allow, queries=Qq, k=k, beam=beam, cut=1.35,
                                                 out_k=rc.pool(beam, k, rf))
            rr_ids, rr_dists = rc.rerank_rows("l2_64", ref["ids"], ref["result_count"], k)
            got = c.fused(k, beam, rf, where=(kind, preds))
            np.testing.assert_array_equal(got["ids"], rr_ids, err_msg=pname)
            assert np.array_equal(got["dists"].view(np.uint32), rr_dists.view(np.uint32)), pname
            for f in FIELDS[2:]:
                np.testing.assert_array_equal(got[f], ref[f], err_msg=f"{pname} {f}")
            assert (ref["result_count"] > 0).all() and (ref["allowed_cmps"] < ref["dist_cmps"]).all()
    finally:
        _capi.check(c.full._lib.pann_index_set_exact_float_order(c.full.handle, 0))


def test_dev_entry_on_a_callers_stream(cases):
    import torch
    c = cases("l2_64")
    k, beam, d = 10, 64, c.X.shape[1]
    for pname in ("tenant", "range-straddle"):
        labels, kind, preds, _ = lc.CASES[pname]
        c.full.set_labels(labels)
        host = c.fused(k, beam, 100, where=(kind, preds))
        p = np.ascontiguousarray(np.asarray(preds, np.uint32).reshape(-1, 2))
        t_q = torch.from_numpy(c.Q.copy()).cuda()
        t_p = torch.from_numpy(p.view(np.int32)).cuda()
        t_st = torch.zeros(1, dtype=torch.int32, device="cuda")
        t_ids = torch.zeros((NQ, k), dtype=torch.int32, device="cuda")
        t_d = torch.zeros((NQ, k), dtype=torch.float32, device="cuda")
        t_cnt = [torch.zeros(NQ, dtype=torch.int32, device="cuda") for _ in range(5)]
        t_status = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        for _ in range(2):                                            # the second launch finds the scratch at its size
            c.full.search_rerank_dev(c.quant, c.qparams, t_q.data_ptr(), NQ, 4 * d, t_st.data_ptr(), 1, t_ids.data_ptr(), t_d.data_ptr(),
                                     k=k, beam=beam, d_frontier_size_ptr=t_cnt[0].data_ptr(), d_visited_count_ptr=t_cnt[1].data_ptr(),
                                     d_dist_cmps_ptr=t_cnt[2].data_ptr(), d_status_ptr=t_status.data_ptr(), stream_ptr=stream.cuda_stream,
                                     d_preds_ptr=t_p.data_ptr(), pred_kind=kind, npreds=len(p), d_result_count_ptr=t_cnt[3].data_ptr(),
                                     d_allowed_cmps_ptr=t_cnt[4].data_ptr())
        stream.synchronize()
        got = {"ids": t_ids, "dists": t_d, "frontier_size": t_cnt[0], "visited_count": t_cnt[1], "dist_cmps": t_cnt[2],
               "result_count": t_cnt[3], "allowed_cmps": t_cnt[4]}
        for f, t in got.items():
            assert np.array_equal(t.cpu().numpy().view(np.uint32), host[f].view(np.uint32)), (pname, f)
        assert int(t_status.cpu()[0]) == 0


def test_refusals(cases):
    c = cases("l2_64")
    labels, kind, preds, _ = lc.CASES["tenant"]
    c.full.set_labels(labels)
    BAD, UNS = _capi.PANN_ERR_BAD_ARG, _capi.PANN_ERR_UNSUPPORTED

    def code(**kw):
        with pytest.raises(PannError) as e:
            c.fused(**{**dict(k=10, beam=64, rf=100, where=(kind, preds)), **kw})
        assert str(e.value)
        return e.value.code

    assert code(use_filter=True) == UNS                               # no sketch-filter x predicate kernel, as the bitmap twin
    assert code(k=65, beam=128) == UNS                                # the list holds at most 64 keys
    assert code(k=65, beam=64) == BAD
    assert code(where=(7, preds)) == BAD                              # unknown kind
    lib = _capi.load()
    q = _capi.QueryParams(k=10, beam=64, cut=1.35, limit=N, degree_limit=R, rerank_factor=100, pad=1.0)
    ids = np.full((NQ, 10), 0x25A5A5A5, np.uint32); dists = np.full((NQ, 10), -7.0, np.float32)
    st = np.zeros(1, np.uint32)
    o = _capi.RerankOut(ids=ids.ctypes.data_as(C.c_void_p), dists=dists.ctypes.data_as(C.c_void_p))

    def raw(full, p, npreds):
        return lib.pann_batch_search_labeled_rerank(full, c.quant.handle, C.byref(c.qparams), c.Q.ctypes.data_as(C.c_void_p), NQ,
                                                    4 * c.X.shape[1], 0, 0, st.ctypes.data_as(C.c_void_p), 1, C.byref(q), 1,
                                                    None if p is None else p.ctypes.data_as(C.c_void_p), npreds, C.byref(o), None, None)
    assert raw(c.full.handle, preds, 2) == BAD                        # npreds = 2 with nq = 8
    assert raw(c.full.handle, None, NQ) == BAD
    c.full.drop_labels()
    assert raw(c.full.handle, preds, NQ) == BAD                       # `full` without labels (labels on quant do not count)
    c.quant.set_labels(labels)
    try:
        assert raw(c.full.handle, preds, NQ) == BAD
    finally:
        c.quant.drop_labels()
    assert (ids == 0x25A5A5A5).all() and (dists == -7.0).all()
    c.full.set_labels(labels)
    assert raw(c.full.handle, preds, NQ) == _capi.PANN_OK and (ids != 0x25A5A5A5).all()      # the handles still work
    with pytest.raises(ValueError):
        c.fused(10, 64, 100, where=(kind, preds), allow=np.ones(N, bool))
