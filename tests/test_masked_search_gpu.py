"""Masked beam search on the device (pann_batch_search_masked*, DESIGN.md "Masked search") against the restatement
tests/masked_ref.py, bit for bit on integer-valued data.  Every case is run with the mask as ONE shared bitmap and -- same
content -- as one row per query; the traversal fields are also compared with batch_search of the same handle.  That the cases
meet their regimes (short rows, results from beyond the cutoff, from unmerged candidates, re-compared points, ...) is asserted
from the restatement here and, without a GPU, in tests/test_masked_ref_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import masked_cases as mc
import masked_ref
from parlayann_amd import DeviceIndex, PannError, _capi, allow_bitmap

pytestmark = pytest.mark.gpu

F = np.float32
TRAVERSAL = ("frontier_size", "visited_count", "dist_cmps", "degree_sum")
_handles = {}


def _index(layout, deg):
    """one handle per (layout, degree), made once"""
    if (layout, deg) not in _handles:
        rows, _, _ = mc.device_rows(layout)
        kind, d, metric = mc.LAYOUTS[layout]
        if kind in ("u4", "i4"):
            ix = DeviceIndex.from_packed(rows, d, kind, graph=mc.graph(deg))
        else:
            ix = DeviceIndex(rows, mc.graph(deg), metric=metric)
        _handles[(layout, deg)] = ix
    return _handles[(layout, deg)]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for ix in _handles.values():
        ix.close()
    _handles.clear()


def _same(ref, got, scale=1.0, plain=None):
    """every output of the masked call equals the restatement; the traversal fields also equal the plain search's"""
    assert got["status"][0] == 0
    np.testing.assert_array_equal(ref["ids"], got["ids"], err_msg="ids")
    assert got["dists"].dtype == F and not np.isnan(got["dists"]).any()
    np.testing.assert_array_equal(ref["dists"] * F(scale), got["dists"], err_msg="dists")
    for f in TRAVERSAL + ("result_count", "allowed_cmps"):
        np.testing.assert_array_equal(ref[f], got[f], err_msg=f)
    for i in range(len(ref["ids"])):
        nv = int(ref["visited_count"][i])
        np.testing.assert_array_equal(ref["visited_ids"][i, :nv], got["visited_ids"][i, :nv], err_msg="visited_ids")
        np.testing.assert_array_equal(ref["visited_dists"][i, :nv] * F(scale), got["visited_dists"][i, :nv], err_msg="visited_dists")
    if plain is not None:
        for f in TRAVERSAL:
            np.testing.assert_array_equal(plain[f], got[f], err_msg="plain " + f)
        np.testing.assert_array_equal(plain["ids"], ref["frontier_ids"], err_msg="plain ids")
        for i in range(len(ref["ids"])):
            nv = int(ref["visited_count"][i])
            np.testing.assert_array_equal(plain["visited_ids"][i, :nv], got["visited_ids"][i, :nv])


def _run(layout, deg, kw, m, ref):
    ix = _index(layout, deg)
    _, Qd, scale = mc.device_rows(layout)
    skw = mc.search_kw(kw)
    q = dict(query_ids=mc.QUERY_IDS) if kw.get("query_ids") else dict(queries=Qd)
    plain = ix.batch_search(**q, **skw)
    rows = np.broadcast_to(m, (mc.NQ, mc.N))
    per_query = ix.batch_search_masked(allow=mc.pack(rows), **q, **skw)
    _same(ref, per_query, scale, plain)
    if m.ndim == 1:                       # one shared bitmap: packed with the dead bits set, and as a boolean array
        shared = ix.batch_search_masked(allow=mc.pack(m), **q, **skw)
        _same(ref, shared, scale)
        _same(ref, ix.batch_search_masked(allow=m, **q, **skw), scale)
    else:                                 # per-query rows with a stride larger than a row
        wide = np.zeros((mc.NQ, mc.WORDS + 3), np.uint32)
        wide[:, :mc.WORDS] = mc.pack(rows)
        wide[:, mc.WORDS:] = 0xFFFFFFFF
        _same(ref, ix.batch_search_masked(allow=wide, **q, **skw), scale)
    found = per_query["ids"][per_query["ids"] != 0xFFFFFFFF]
    qi = np.nonzero(per_query["ids"] != 0xFFFFFFFF)[0]
    assert rows[qi, found].all()          # hard: a disallowed id is never returned


@pytest.mark.parametrize("case", mc.CASES, ids=mc.CASE_IDS)
def test_masked_search_equals_the_restatement(case):
    name, layout, deg, kw, mkind, regime = case
    ref = mc.case_reference(case)
    if regime == "recompared":
        assert ref["recompared_in_result"].sum() > 0
    if regime == "beyond_cutoff":
        assert ref["from_beyond_cutoff"].sum() > 0
    if regime == "unmerged":
        assert ref["from_unmerged"].sum() > 0
    if regime == "short":
        assert (ref["result_count"] < kw["out_k"]).any()
    if regime == "empty":
        assert (ref["result_count"] == 0).all()
    _run(layout, deg, kw, mc.mask(mkind, layout, kw.get("starts", (0,))), ref)


@pytest.mark.parametrize("beam", mc.KIND_BEAMS)
@pytest.mark.parametrize("mkind", mc.MASK_KINDS)
def test_every_mask_kind_on_both_kernels(mkind, beam):
    kw = dict(beam=beam, k=10, out_k=10)
    if mkind == "rand5":
        kw["limit"] = 4                    # four visits compare about a hundred points: five allowed ones, fewer than out_k
    m = mc.mask(mkind, mc.KIND_LAYOUT)
    ref = mc.reference(mc.KIND_LAYOUT, 32, kw, m, key=("kinds", mkind, beam))
    if mkind == "zeros":
        assert (ref["result_count"] == 0).all() and (ref["ids"] == 0xFFFFFFFF).all()
    if mkind == "only_start":
        assert (ref["result_count"] == 1).all()
    if mkind == "rand5":
        assert (ref["result_count"] < 10).any()                # short rows
    if mkind == "start_off":
        assert not (ref["ids"] == 0).any() and (ref["frontier_ids"] == 0).any()
    _run(mc.KIND_LAYOUT, 32, kw, m, ref)


def test_host_entry_repeats_the_batch_on_a_dropped_list_overflow():
    """cut = 1.0 on a line keeps the frontier short: > 256 visited vertices leave it, the default dropped list overflows, the
    host entry grows it and runs the batch again -- the result list must be the second run's alone"""
    X, G, Q, allow = mc.line_case()
    for beam in (16, 100, 300):
        kw = dict(k=1, beam=beam, cut=1.0, out_k=2, visited_cap=2048)
        ref = masked_ref.masked_batch_search(X, G, allow, queries=Q, **kw)
        assert ref["visited_count"].max() > 600
        ix = DeviceIndex(X, G)
        try:
            assert ix.dropped_capacity == 256
            got = ix.batch_search_masked(Q, allow=allow, **kw)
            assert ix.dropped_capacity > 256
            _same(ref, got, plain=ix.batch_search(Q, **kw))
        finally:
            ix.close()


def test_dev_entry_on_a_stream_equals_the_host_entry():
    import torch
    lib = _capi.load()
    dev = torch.device("cuda", 0)
    # f16 / f32 at beam <= 64: the masked register-frontier kernel; u8 at 64: its fallback to the generic one; 65, 300: generic
    for layout, beam, mkind in (("f16", 64, "rand50"), ("f32", 64, "rows_differ"), ("u8", 64, "rand50"), ("f16", 65, "rows_differ"),
                                ("f32", 300, "rand5")):
        ix = _index(layout, 32)
        _, Qd, _ = mc.device_rows(layout)
        m = mc.mask(mkind, layout)
        packed = mc.pack(m)
        kw = dict(k=10, beam=beam, cut=1.35, out_k=10, visited_cap=2048)
        host = ix.batch_search_masked(Qd, allow=packed, **kw)
        nq, ok, vc = mc.NQ, 10, 2048
        stream = torch.cuda.Stream(device=dev)
        assert stream.cuda_stream != 0
        t_q = torch.from_numpy(np.ascontiguousarray(Qd).view(np.uint8).reshape(nq, -1)).to(dev)
        t_allow = torch.from_numpy(packed.view(np.int32)).to(dev)
        t_st = torch.zeros(1, dtype=torch.int32, device=dev)
        t_ids = torch.zeros((nq, ok), dtype=torch.int32, device=dev)
        t_dist = torch.zeros((nq, ok), dtype=torch.float32, device=dev)
        t_cnt = [torch.zeros(nq, dtype=torch.int32, device=dev) for _ in range(6)]
        t_vid = torch.zeros((nq, vc), dtype=torch.int32, device=dev)
        t_vd = torch.zeros((nq, vc), dtype=torch.float32, device=dev)
        t_status = torch.full((1,), 77, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        qp = _capi.QueryParams(k=10, beam=beam, cut=1.35, limit=mc.N, degree_limit=32, rerank_factor=100, pad=1.0)
        out = _capi.SearchOut(ids=t_ids.data_ptr(), dists=t_dist.data_ptr(), out_k=ok, frontier_size=t_cnt[0].data_ptr(),
                              visited_count=t_cnt[1].data_ptr(), dist_cmps=t_cnt[2].data_ptr(), degree_sum=t_cnt[3].data_ptr(),
                              visited_ids=t_vid.data_ptr(), visited_dists=t_vd.data_ptr(), visited_cap=vc, status=t_status.data_ptr())
        _capi.check(lib.pann_batch_search_masked_dev(ix.handle, C.c_void_p(t_q.data_ptr()), None, nq, t_q.shape[1],
                                                     C.c_void_p(t_st.data_ptr()), 1, C.byref(qp), C.c_void_p(t_allow.data_ptr()),
                                                     mc.WORDS if m.ndim == 2 else 0, C.byref(out), C.c_void_p(t_cnt[4].data_ptr()),
                                                     C.c_void_p(t_cnt[5].data_ptr()), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        assert int(t_status.cpu()[0]) == 0                      # the status word, read after the synchronisation
        got = {"ids": t_ids, "dists": t_dist, "frontier_size": t_cnt[0], "visited_count": t_cnt[1], "dist_cmps": t_cnt[2],
               "degree_sum": t_cnt[3], "result_count": t_cnt[4], "allowed_cmps": t_cnt[5]}
        for f, t in got.items():
            np.testing.assert_array_equal(t.cpu().numpy().view(host[f].dtype), host[f], err_msg=f"{layout} b{beam} {f}")
        vids, vds = t_vid.cpu().numpy().view(np.uint32), t_vd.cpu().numpy()
        for i in range(nq):
            nv = int(host["visited_count"][i])
            np.testing.assert_array_equal(vids[i, :nv], host["visited_ids"][i, :nv])
            np.testing.assert_array_equal(vds[i, :nv], host["visited_dists"][i, :nv])


def test_refusals():
    ix = _index("u8", 32)
    _, Q, _ = mc.device_rows("u8")
    lib = _capi.load()
    ones = mc.pack(np.ones(mc.N, bool))

    def code(fn):
        with pytest.raises(PannError) as e:
            fn()
        assert str(e.value)
        return e.value.code

    assert code(lambda: ix.batch_search_masked(Q, allow=None, k=10, beam=64)) == _capi.PANN_ERR_BAD_ARG          # null bitmap
    short = np.ones((mc.NQ, mc.WORDS - 1), np.uint32)
    ids = np.zeros((mc.NQ, 10), np.uint32)
    st = np.zeros(1, np.uint32)
    qp = _capi.QueryParams(k=10, beam=64, cut=1.35, limit=mc.N, degree_limit=32, rerank_factor=100, pad=1.0)

    def call(allow, stride, out_k=10, beam=64):
        qp.beam = beam
        out = _capi.SearchOut(ids=np.zeros((mc.NQ, out_k), np.uint32).ctypes.data_as(C.c_void_p) if out_k != 10 else ids.ctypes.data_as(C.c_void_p),
                              out_k=out_k)
        return lambda: _capi.check(lib.pann_batch_search_masked(
            ix.handle, Q.ctypes.data_as(C.c_void_p), None, mc.NQ, Q.shape[1], st.ctypes.data_as(C.c_void_p), 1, C.byref(qp),
            None if allow is None else allow.ctypes.data_as(C.c_void_p), stride, C.byref(out), None, None))

    call(ones, 0)()                                                                   # the valid call
    assert code(call(None, 0)) == _capi.PANN_ERR_BAD_ARG                              # null bitmap
    assert code(call(short, mc.WORDS - 1)) == _capi.PANN_ERR_BAD_ARG                  # stride shorter than a bitmap
    assert code(call(short, 1)) == _capi.PANN_ERR_BAD_ARG
    assert code(call(ones, 0, out_k=65, beam=128)) == _capi.PANN_ERR_UNSUPPORTED      # out_k > 64
    assert code(call(ones, 0, out_k=65, beam=64)) == _capi.PANN_ERR_BAD_ARG           # out_k > beam
    assert code(call(ones, 0, out_k=64, beam=32)) == _capi.PANN_ERR_BAD_ARG
    # a mask together with the sketch filter cannot be expressed: no entry point takes both (DESIGN.md "Masked search")
    with pytest.raises(TypeError):
        ix.batch_search_masked(Q, allow=ones, k=10, beam=64, sketch_queries=np.zeros((mc.NQ, 16), np.uint8))
    with pytest.raises(ValueError):
        ix.batch_search_masked(Q, allow=np.ones((mc.NQ + 1, mc.WORDS), np.uint32), k=10, beam=64)    # rows != queries
    # the device entry checks the same arguments before it launches anything
    out = _capi.SearchOut(ids=None, out_k=10)
    qp.beam = 64
    assert lib.pann_batch_search_masked_dev(ix.handle, None, None, mc.NQ, 128, None, 1, C.byref(qp), None, 0, C.byref(out), None, None,
                                            None) == _capi.PANN_ERR_BAD_ARG
    g = ix.batch_search_masked(Q, allow=ones, k=10, beam=64)                          # the handle still works
    assert (g["result_count"] == 10).all()


def test_tombstone_round_trip(oracle):
    """mark in the bitmap -> masked searches return no marked id -> vamana_delete_batch -> the plain search returns none either"""
    from parlayann_amd import datasets
    n, R, L = 2000, 32, 64
    X = datasets.sift_like(n, 32, seed=1001, dtype=np.uint8)
    Q = datasets.sift_like(64, 32, seed=2001, dtype=np.uint8)
    ix = DeviceIndex(X, max_degree=R)
    try:
        ix.vamana_build(R, L, 1.2, num_passes=1, seed=1)
        deleted = np.random.default_rng(3).choice(np.arange(1, n), n // 5, replace=False).astype(np.uint32)
        allow = allow_bitmap(n, deleted_ids=deleted)
        before = ix.batch_search(Q, k=10, beam=32)
        assert np.isin(before["ids"], deleted).any()                    # the plain search does return doomed ids
        g = ix.batch_search_masked(Q, allow=allow, k=10, beam=32)
        assert (g["result_count"] == 10).all() and not np.isin(g["ids"], deleted).any()
        for f in TRAVERSAL:
            np.testing.assert_array_equal(g[f], before[f])
        ref = masked_ref.masked_batch_search(X, ix.get_graph(), allow, queries=Q, k=10, beam=32)
        np.testing.assert_array_equal(ref["ids"], g["ids"]); np.testing.assert_array_equal(ref["dists"], g["dists"])
        ix.vamana_delete_batch(deleted, R, 1.2)
        after = ix.batch_search(Q, k=10, beam=32)
        assert not np.isin(after["ids"], deleted).any()
        # once consolidated the bits can be cleared or kept: a masked search of the new graph returns no deleted id either way
        again = ix.batch_search_masked(Q, allow=allow, k=10, beam=32)
        assert not np.isin(again["ids"], deleted).any()
    finally:
        ix.close()


def test_python_mirror_routes_allow_to_the_masked_search(tmp_path):
    """float32 rows at beam 64: the mirror's plain path on the masked register-frontier kernel"""
    from parlayann_amd import io
    from parlayann_amd.graph_index import FloatEuclidianIndex
    X, Q, _, _ = mc.layout_data("f32")
    G = mc.graph(32)
    io.write_bin(tmp_path / "b.bin", X)
    io.write_bin(tmp_path / "q.bin", Q)
    io.write_graph(tmp_path / "g.graph", G)
    m = mc.mask("rand50", "f32")
    gi = FloatEuclidianIndex(str(tmp_path / "b.bin"), str(tmp_path / "g.graph"))
    try:
        plain = gi.batch_search(Q, 10, 64, visit_limit=1000)
        ids, dists = gi.batch_search(Q, 10, 64, visit_limit=1000, allow=m)
        ref = mc.reference("f32", 32, dict(beam=64, k=10, out_k=10, limit=1000), m)
        np.testing.assert_array_equal(ids, ref["ids"]); np.testing.assert_array_equal(dists, ref["dists"])
        ids2, _ = gi.batch_search_from_string(str(tmp_path / "q.bin"), 10, 64, visit_limit=1000, allow=mc.pack(m))
        np.testing.assert_array_equal(ids2, ids)
        again = gi.batch_search(Q, 10, 64, visit_limit=1000)                  # absent: unchanged
        np.testing.assert_array_equal(again[0], plain[0]); np.testing.assert_array_equal(again[1], plain[1])
        with pytest.raises(ValueError):                                           # not in the quantised / rerank paths
            gi.batch_search(Q, 10, 64, quant=True, visit_limit=1000, allow=m)
    finally:
        gi.index.close()
        if gi.q_index is not None:
            gi.q_index.close()
