"""The sketch-filtered beam search on the device (FILTER variants of the generic kernel, csrc/beam_search.hip) against the
Python checker of filtered_beam_search with use_filtering (tests/filtered_ref.py): every output bit for bit.  The cases are
those of tests/filtered_cases.py; tests/test_filtered_ref_cpu.py shows on the CPU that each of them really filters."""
import ctypes as C

import numpy as np
import pytest

import filtered_cases as fc
import filtered_ref
from parlayann_amd import DeviceIndex, PannError, _capi, io, quantize
from parlayann_amd import sketch as sk
from parlayann_amd.graph_index import FloatEuclidianIndex, FloatMipsIndex

pytestmark = pytest.mark.gpu

FIELDS = ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum", "pruned_cmps")
VCAP = 2000


def _compare(g, r):
    for f in FIELDS:
        assert np.array_equal(g[f], r[f]), (f, g[f], r[f])
    for i in range(len(r["visited_count"])):
        v = int(r["visited_count"][i])
        assert np.array_equal(g["visited_ids"][i, :v], r["visited_ids"][i, :v]), i
        assert np.array_equal(g["visited_dists"][i, :v], r["visited_dists"][i, :v]), i


def _attach(c):
    """-> (searched handle, float source handle or None when it is the searched handle itself)"""
    ix = DeviceIndex(c["X"], c["graph"], metric=c["metric"], exact_float_order=c["exact"])
    src = ix if c["X"].dtype == np.float32 else DeviceIndex(c["Xf"], max_degree=4, metric=c["metric"])
    p = sk.sketch_params(src, c["kind"])
    e = c["params"]
    assert (p.kind, p.dims, p.median) == (e.kind, e.dims, e.median) and np.float32(p.cut) == np.float32(e.cut)
    p.hamming_as_written = e.hamming_as_written
    sk.attach_sketch(ix, src, p)
    return ix, (None if src is ix else src), p


@pytest.mark.parametrize("case", fc.CASES, ids=fc.CASE_IDS)
def test_filtered_search_equals_the_checker(case):
    c = fc.build_case(case)
    ref = filtered_ref.filtered_batch_search(**fc.checker_args(c, True))
    ix, src, p = _attach(c)
    try:
        sq = None if c["queries"] is None else sk.sketch_rows(c["Qf"], p)
        if sq is not None:
            np.testing.assert_array_equal(sq, sk.sketch_rows_numpy(c["Qf"], c["params"]))
        g = ix.batch_search_filtered(c["queries"], sq, query_ids=c["query_ids"], out_k=c["qp"]["beam"], visited_cap=VCAP, **c["qp"])
        _compare(g, ref)
    finally:
        ix.close()
        if src is not None:
            src.close()


@pytest.mark.parametrize("beam", [16, 64, 100, 200])
def test_degenerate_sketch_drops_everything_once_full(beam):
    """all-positive data under MIPS_BIT: every sketch distance is 0, the threshold is 0, and 0 >= 0 drops every neighbour"""
    rng = np.random.default_rng(beam)
    n, d, nq = 3000, 96, 8
    Xf = quantize.normalize_rows(np.abs(rng.standard_normal((n, d))).astype(np.float32) + 0.01)
    Qf = quantize.normalize_rows(np.abs(rng.standard_normal((nq, d))).astype(np.float32) + 0.01)
    mv = quantize.mips_i8_max_val(Xf)
    X, Q = quantize.mips_i8_translate(Xf, mv), quantize.mips_i8_translate(Qf, mv)
    G = fc.random_graph(n, 32, 9)
    p = sk.make_params("mips_bit", d)
    S, SQ = sk.sketch_rows_numpy(Xf, p), sk.sketch_rows_numpy(Qf, p)
    assert (S[:, :d // 8] == 0xFF).all() and (SQ[:, :d // 8] == 0xFF).all() and not S[:, d // 8:].any()      # d = 96: 12 bytes set
    qp = dict(k=0, beam=beam)
    ref = filtered_ref.filtered_batch_search(X, G, queries=Q, metric="mips", out_k=beam, visited_cap=VCAP, use_filtering=True,
                                             sketches=S, sketch_queries=SQ, sketch_params=p, **qp)
    assert (ref["sketch_dropped"] > 0).all()
    ix, src = DeviceIndex(X, G, metric="mips"), DeviceIndex(Xf, max_degree=4, metric="mips")
    try:
        sk.attach_sketch(ix, src, p)
        g = ix.batch_search_filtered(Q, sk.sketch_rows(Qf, p), out_k=beam, visited_cap=VCAP, **qp)
        _compare(g, ref)
    finally:
        ix.close(); src.close()


@pytest.mark.parametrize("beam", [16, 64, 100, 128, 200])
def test_plain_search_ignores_an_attached_sketch(beam):
    c = fc.build_case(fc.CASES[0])
    ix = DeviceIndex(c["X"], c["graph"], metric=c["metric"])
    src = DeviceIndex(c["Xf"], max_degree=4, metric=c["metric"])
    try:
        kw = dict(k=10, beam=beam, out_k=beam, visited_cap=VCAP)
        before = ix.batch_search(c["Q"], **kw)
        before_ids = ix.batch_search(query_ids=np.arange(5, 50, 5, dtype=np.uint32), **kw)
        sk.attach_sketch(ix, src, sk.sketch_params(src, "euclid_bit"))
        after = ix.batch_search(c["Q"], **kw)
        after_ids = ix.batch_search(query_ids=np.arange(5, 50, 5, dtype=np.uint32), **kw)
        for a, b in ((before, after), (before_ids, after_ids)):
            for f in ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum"):
                assert np.array_equal(a[f], b[f]), f
            for i, v in enumerate(a["visited_count"]):          # slots past a row's count are not written
                assert np.array_equal(a["visited_ids"][i, :v], b["visited_ids"][i, :v])
                assert np.array_equal(a["visited_dists"][i, :v], b["visited_dists"][i, :v])
    finally:
        ix.close(); src.close()


def test_device_pointer_form_and_large_batches():
    """pann_batch_search_filtered_dev with device sketch-query rows at a caller's stride and d_out_pruned_cmps, on the LDS-filter
    (beam 64) and HBM-filter (beam 200) variants, with more queries than the HBM variant has persistent blocks (nq > 2048: a
    block re-stages the query sketch for every query it takes).  The batch is the case's 12 queries repeated, so every
    repetition must equal the host-pointer result of its query."""
    import torch
    c = fc.build_case(fc.CASES[1])               # u8 / L2 / Euclidean_Bit_Point, as written, d = 200: 32-byte sketch rows
    ix, src, p = _attach(c)
    lib = _capi.load()
    try:
        n, d = c["X"].shape
        rb, reps = sk.row_bytes(p.kind, d), 260
        nq = fc.NQ * reps                                                   # 3120 > 2048
        sq = sk.sketch_rows(c["Qf"], p)
        sq_pad = np.full((fc.NQ, rb + 24), 0xA5, np.uint8)                  # stride larger than a row, still a multiple of 8
        sq_pad[:, :rb] = sq
        t_q = torch.from_numpy(np.tile(c["Q"], (reps, 1))).cuda()
        t_sq = torch.from_numpy(np.tile(sq_pad, (reps, 1))).cuda()
        t_st = torch.zeros(1, dtype=torch.int32, device="cuda")
        for beam in (64, 200):
            host = ix.batch_search_filtered(c["Q"], sq, k=10, beam=beam, out_k=beam)
            t_ids = torch.zeros((nq, beam), dtype=torch.int32, device="cuda")
            t_dist = torch.zeros((nq, beam), dtype=torch.float32, device="cuda")
            t_cnt = [torch.zeros(nq, dtype=torch.int32, device="cuda") for _ in range(5)]
            t_status = torch.zeros(1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            qp = _capi.QueryParams(k=10, beam=beam, cut=1.35, limit=n, degree_limit=32, rerank_factor=100, pad=1.0)
            out = _capi.SearchOut(ids=t_ids.data_ptr(), dists=t_dist.data_ptr(), out_k=beam, frontier_size=t_cnt[0].data_ptr(),
                                  visited_count=t_cnt[1].data_ptr(), dist_cmps=t_cnt[2].data_ptr(), degree_sum=t_cnt[3].data_ptr(),
                                  status=t_status.data_ptr())

            def launch(sq_ptr, stride):
                return lib.pann_batch_search_filtered_dev(ix.handle, C.c_void_p(t_q.data_ptr()), None, nq, d, C.c_void_p(sq_ptr), stride,
                                                          C.c_void_p(t_st.data_ptr()), 1, C.byref(qp), C.byref(out),
                                                          C.c_void_p(t_cnt[4].data_ptr()), None)
            assert launch(t_sq.data_ptr(), rb + 20) == 1                    # stride not a multiple of 8
            assert launch(t_sq.data_ptr() + 4, rb + 24) == 1                # rows not 8-byte aligned
            assert launch(t_sq.data_ptr(), rb - 8) == 1                     # stride shorter than a row
            assert launch(None, 0) == 1                                     # queries without sketch queries
            _capi.check(launch(t_sq.data_ptr(), rb + 24))
            torch.cuda.synchronize()
            assert int(t_status.cpu()[0]) == 0
            got = {"ids": t_ids, "dists": t_dist, "frontier_size": t_cnt[0], "visited_count": t_cnt[1], "dist_cmps": t_cnt[2],
                   "degree_sum": t_cnt[3], "pruned_cmps": t_cnt[4]}
            for f, t in got.items():
                a = t.cpu().numpy().view(host[f].dtype).reshape((reps,) + host[f].shape)
                assert (a == host[f][None]).all(), (beam, f)
    finally:
        ix.close()
        if src is not None:
            src.close()


def test_graph_index_refuses_a_second_level_it_cannot_apply(tmp_path):
    from parlayann_amd.graph_index import UInt8EuclidianIndex
    rng = np.random.default_rng(2)
    G = fc.random_graph(400, 16, 3)
    io.write_graph(tmp_path / "g.graph", G)
    io.write_bin(tmp_path / "u8.bin", rng.integers(0, 256, (400, 32), dtype=np.uint8))
    io.write_bin(tmp_path / "int.bin", rng.integers(0, 200, (400, 32)).astype(np.float32))      # quantises to itself (slope 1)
    with pytest.raises(ValueError):
        UInt8EuclidianIndex(str(tmp_path / "u8.bin"), str(tmp_path / "g.graph"), second_level="bit")
    with pytest.raises(ValueError):
        FloatEuclidianIndex(str(tmp_path / "int.bin"), str(tmp_path / "g.graph"), second_level="bit")
    with pytest.raises(ValueError):
        FloatEuclidianIndex(str(tmp_path / "int.bin"), str(tmp_path / "g.graph"), second_level="2bit")


def test_error_statuses():
    rng = np.random.default_rng(1)
    n, d = 300, 70
    Xf = rng.standard_normal((n, d)).astype(np.float32)
    G = fc.random_graph(n, 16, 2)
    ix, other = DeviceIndex(Xf, G, metric="mips"), DeviceIndex(Xf[:, :64].copy(), max_degree=4, metric="mips")
    short = DeviceIndex(Xf[:100].copy(), max_degree=4, metric="mips")
    lib = _capi.load()
    p = sk.make_params("mips_bit", d)
    Q = Xf[:4].copy()

    def code(fn):
        with pytest.raises(PannError) as e:
            fn()
        return e.value.code

    try:
        assert code(lambda: ix.batch_search_filtered(Q, np.zeros((4, 16), np.uint8), k=0, beam=8)) == 1        # no sketch attached
        assert code(lambda: _capi.check(lib.pann_index_download_sketch(ix.handle, 0, 1, np.zeros(64, np.uint8).ctypes.data_as(C.c_void_p),
                                                                       16))) == 1                                 # nothing to download
        assert code(lambda: sk.attach_sketch(ix, other, sk.make_params("mips_bit", 64))) == 1                   # d mismatch
        assert code(lambda: sk.attach_sketch(ix, short, p)) == 1                                                # n mismatch
        assert code(lambda: sk.attach_sketch(ix, ix, sk.make_params("mips_bit", 64))) == 1                      # parameters of another dimension
        assert code(lambda: sk.attach_sketch(ix, ix, _capi.SketchParams(kind=7, dims=d))) == 1                  # unknown kind
        assert code(lambda: _capi.check(lib.pann_index_attach_sketch(ix.handle, ix.handle, None))) == 1         # NULL parameters
        assert code(lambda: _capi.check(lib.pann_sketch_params_generate(ix.handle, 9, C.byref(_capi.SketchParams())))) == 1
        assert code(lambda: _capi.check(lib.pann_sketch_params_generate(ix.handle, 1, None))) == 1
        sk.attach_sketch(ix, ix, p)
        rb = sk.row_bytes("mips_bit", d)
        assert rb == 16
        sq = sk.sketch_rows(Q, p)
        qp = _capi.QueryParams(k=0, beam=8, cut=1.35, limit=n, degree_limit=16, rerank_factor=100, pad=1.0)
        ids = np.zeros((4, 8), np.uint32)
        out = _capi.SearchOut(ids=ids.ctypes.data_as(C.c_void_p), out_k=8)
        st = np.zeros(1, np.uint32)
        qids = np.arange(4, dtype=np.uint32)

        def search(q, qid, s, stride):
            return lambda: _capi.check(lib.pann_batch_search_filtered(
                ix.handle, None if q is None else q.ctypes.data_as(C.c_void_p), None if qid is None else qid.ctypes.data_as(C.c_void_p),
                4, d * 4, None if s is None else s.ctypes.data_as(C.c_void_p), stride, st.ctypes.data_as(C.c_void_p), 1,
                C.byref(qp), C.byref(out), None))

        search(Q, None, sq, rb)()                                                                                # the valid call
        assert code(search(Q, None, None, 0)) == 1                    # queries without sketch queries
        assert code(search(None, qids, sq, rb)) == 1                  # query_ids with sketch queries
        assert code(search(Q, qids, sq, rb)) == 1                     # both query forms
        assert code(search(None, None, None, 0)) == 1                 # neither
        assert code(search(Q, None, sq, rb - 8)) == 1                 # stride shorter than a sketch row
        out_small = np.zeros((4, 8), np.uint8)
        assert code(lambda: _capi.check(lib.pann_index_download_sketch(ix.handle, 0, 4, out_small.ctypes.data_as(C.c_void_p), 8))) == 1
        assert code(lambda: _capi.check(lib.pann_sketch_rows(C.byref(p), Q.ctypes.data_as(C.c_void_p), 4, d * 4,
                                                             out_small.ctypes.data_as(C.c_void_p), 8, 0))) == 1
        assert code(lambda: _capi.check(lib.pann_sketch_rows(C.byref(p), Q.ctypes.data_as(C.c_void_p), 4, d * 4 - 4,
                                                             np.zeros((4, 16), np.uint8).ctypes.data_as(C.c_void_p), 16, 0))) == 1
        sk.drop_sketch(ix)
        assert code(search(None, qids, None, 0)) == 1                 # dropped: no sketch attached
    finally:
        ix.close(); other.close(); short.close()


@pytest.mark.parametrize("metric,level", [("mips", "2bit"), ("mips", "bit"), ("Euclidian", "bit")])
def test_graph_index_second_level(tmp_path, metric, level):
    rng = np.random.default_rng(7)
    n, d, nq, knn, beam = 3000, 256, 10, 10, 32
    X = (rng.standard_normal((n, d)) * 3 + (1.5 if metric == "Euclidian" else 0)).astype(np.float32)
    Q = (rng.standard_normal((nq, d)) * 3 + (1.5 if metric == "Euclidian" else 0)).astype(np.float32)
    G = fc.random_graph(n, 32, 3)
    io.write_bin(tmp_path / "b.bin", X)
    io.write_graph(tmp_path / "g.graph", G)
    cls = FloatMipsIndex if metric == "mips" else FloatEuclidianIndex
    plain = cls(str(tmp_path / "b.bin"), str(tmp_path / "g.graph"))
    two = cls(str(tmp_path / "b.bin"), str(tmp_path / "g.graph"), second_level=level)
    try:
        # second_level=None: today's output, with and without quantisation
        base_q = plain.batch_search(Q, knn, beam, quant=True, visit_limit=1000)
        ids0, d0 = two.batch_search(Q, knn, beam, quant=False, visit_limit=1000)
        idsp, dp = plain.batch_search(Q, knn, beam, quant=False, visit_limit=1000)
        assert np.array_equal(ids0, idsp) and np.array_equal(d0, dp)
        # composed by hand: filtered search of the one-byte handle, then pann_rerank on the float handle
        ids, dists = two.batch_search(Q, knn, beam, quant=True, visit_limit=1000)
        qp = two._qp(knn, beam, 1000)
        if metric == "mips":
            full_q = quantize.normalize_rows(Q)
            qq = quantize.device_quantize_rows(Q, two.qparams, normalize_first=True)
        else:
            full_q = Q
            qq = quantize.device_quantize_rows(Q, two.qparams)
        sq = sk.sketch_rows(full_q, two.sparams)
        np.testing.assert_array_equal(sq, sk.sketch_rows_numpy(full_q, two.sparams))
        r = two.q_index.batch_search_filtered(qq, sq, out_k=beam, **qp)
        counts = np.minimum(r["frontier_size"], knn * 100).astype(np.uint32)
        eids, edists = two.index.rerank(full_q, r["ids"], counts, knn, resort=True)
        assert np.array_equal(ids, eids) and np.array_equal(dists, edists)
        assert (r["dist_cmps"] < r["pruned_cmps"]).any()              # the second level really filtered
        # the unfiltered quantised path of the same object's class is untouched
        again = plain.batch_search(Q, knn, beam, quant=True, visit_limit=1000)
        assert np.array_equal(base_q[0], again[0]) and np.array_equal(base_q[1], again[1])
    finally:
        for o in (plain, two):
            o.index.close()
            if o.q_index is not None:
                o.q_index.close()
