"""Label-predicate search on the device (pann_batch_search_labeled*, DESIGN.md "Label predicates").  The rule: a labeled call
returns what the bitmap call returns for the rows { i : pred_q(label[i]) }.  Every run is compared, output by output and bit for
bit, with the CPU restatement tests/masked_ref.py fed with label_allow(...) -- the independent reference -- and, second, with
batch_search_masked of the same handle on the packed rows.  The cases are those of tests/label_cases.py, which
tests/test_label_cases_cpu.py shows to be what they claim; the mask reproductions meet the references of the existing masked
cases unchanged."""
import ctypes as C

import numpy as np
import pytest

import label_cases as lc
import masked_cases as mc
from parlayann_amd import DeviceIndex, PannError, _capi
from parlayann_amd.index import label_allow

pytestmark = pytest.mark.gpu

F = np.float32
FIELDS = ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum", "result_count", "allowed_cmps")
_handles = {}


def _index(layout, deg):
    """one handle per (layout, degree), made once; its labels are set by each run"""
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


def _same_as_ref(ref, got, scale=1.0):
    assert got["status"][0] == 0
    np.testing.assert_array_equal(ref["ids"], got["ids"], err_msg="ids")
    assert got["dists"].dtype == F and not np.isnan(got["dists"]).any()
    np.testing.assert_array_equal(ref["dists"] * F(scale), got["dists"], err_msg="dists")
    for f in FIELDS[2:]:
        np.testing.assert_array_equal(ref[f], got[f], err_msg=f)
    for i in range(len(ref["ids"])):
        nv = int(ref["visited_count"][i])
        np.testing.assert_array_equal(ref["visited_ids"][i, :nv], got["visited_ids"][i, :nv], err_msg="visited_ids")
        np.testing.assert_array_equal(ref["visited_dists"][i, :nv] * F(scale), got["visited_dists"][i, :nv], err_msg="visited_dists")


def _same_as_bitmap(bm, got):
    for f in FIELDS:
        np.testing.assert_array_equal(bm[f], got[f], err_msg="bitmap entry: " + f)
    for i in range(len(bm["ids"])):
        nv = int(bm["visited_count"][i])
        np.testing.assert_array_equal(bm["visited_ids"][i, :nv], got["visited_ids"][i, :nv])
        np.testing.assert_array_equal(bm["visited_dists"][i, :nv], got["visited_dists"][i, :nv])


def _run(layout, deg, kw, labels, kind, preds, ref):
    """labeled search of one case against `ref` (masked_ref on the expanded mask) and against the bitmap entry"""
    ix = _index(layout, deg)
    ix.set_labels(labels)
    assert ix.has_labels
    _, Qd, scale = mc.device_rows(layout)
    skw = mc.search_kw(kw)
    q = dict(query_ids=mc.QUERY_IDS) if kw.get("query_ids") else dict(queries=Qd)
    got = ix.batch_search_labeled(where=(kind, preds), **q, **skw)
    _same_as_ref(ref, got, scale)
    rows = np.broadcast_to(label_allow(labels, kind, preds), (mc.NQ, mc.N))
    _same_as_bitmap(ix.batch_search_masked(allow=mc.pack(rows), **q, **skw), got)
    if np.asarray(preds).ndim == 1:          # the same predicate once per query: the per-query form of the kernel
        _same_as_ref(ref, ix.batch_search_labeled(where=(kind, lc.preds_rows(preds)), **q, **skw), scale)
    found = got["ids"] != 0xFFFFFFFF
    assert rows[np.nonzero(found)[0], got["ids"][found]].all()          # hard: a disallowed id is never returned
    return got


def _ref(layout, deg, kw, labels, kind, preds, key):
    return mc.reference(layout, deg, kw, label_allow(labels, kind, preds), key=key)


# ---- the mask reproductions: the references of the existing masked cases, unchanged ----

@pytest.mark.parametrize("beam", mc.KIND_BEAMS)
@pytest.mark.parametrize("mkind", lc.MASK_KINDS)
def test_mask_reproductions_meet_the_existing_references(mkind, beam):
    kw = dict(beam=beam, k=10, out_k=10)
    if mkind == "rand5":
        kw["limit"] = 4                    # as tests/test_masked_search_gpu.py: short rows
    labels, kind, preds, _ = lc.CASES["mask-" + mkind]
    # same key, same mask: the reference test_every_mask_kind_on_both_kernels uses
    ref = mc.reference(mc.KIND_LAYOUT, 32, kw, mc.mask(mkind, mc.KIND_LAYOUT), key=("kinds", mkind, beam))
    if mkind == "zeros":
        assert (ref["result_count"] == 0).all()
    if mkind == "rand5":
        assert (ref["result_count"] < 10).any()
    _run(mc.KIND_LAYOUT, 32, kw, labels, kind, preds, ref)


def test_recompared_points_on_the_vamana_graph():
    """beam 8 on the oracle's Vamana graph: 1 024 filter slots for 3 001 ids, points are compared again and reach the result"""
    case = next(c for c in mc.CASES if c[0] == "f16-vamana-b8-rand50")
    ref = mc.case_reference(case)
    assert ref["recompared_in_result"].sum() > 0
    labels, kind, preds, _ = lc.CASES["mask-rand50"]
    _run("f16", "vamana", case[3], labels, kind, preds, ref)


# ---- every kernel route, with one predicate for the batch and with one per query ----

# layout, degree, beam, out_k: f16 b64 register-frontier kernel; f16 b65 generic kernel, filter in LDS; u8 b64 generic fallback
# (no masked beam-64 form); f32d200 rows of 64-byte granules, degree 96; i8mips b300 filter in HBM, persistent grid; u4; bf16d200
# generic fallback
ROUTES = [("f16", 32, 64, 10), ("f16", 32, 65, 10), ("u8", 32, 64, 10), ("f32d200", 96, 8, 8), ("i8mips", 32, 300, 10),
          ("u4", 32, 64, 10), ("bf16d200", 32, 64, 10)]
ROUTE_IDS = [f"{r[0]}-deg{r[1]}-b{r[2]}" for r in ROUTES]
# shared / per-query predicates alternate between the MATCH and the RANGE cases over the routes
SHARED = ["tenant-shared", "range-straddle"]
ROWS = ["range-rows", "tenant"]


@pytest.mark.parametrize("form", ["shared", "rows", "query_ids"])
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_every_route_equals_the_restatement(route, form):
    layout, deg, beam, out_k = route
    i = ROUTES.index(route)
    name = ROWS[i % 2] if form == "rows" else SHARED[(i + (form == "query_ids")) % 2]
    kw = dict(beam=beam, k=min(10, out_k), out_k=out_k)
    if form == "query_ids":
        kw["query_ids"] = True
    labels, kind, preds, _ = lc.CASES[name]
    ref = _ref(layout, deg, kw, labels, kind, preds, key=("label", layout, deg, beam, form, name))
    assert (ref["result_count"] > 0).all() and (ref["allowed_cmps"] < ref["dist_cmps"]).all()      # the predicate did filter
    got = _run(layout, deg, kw, labels, kind, preds, ref)
    if form == "rows":
        assert len({r.tobytes() for r in got["ids"]}) > 1


@pytest.mark.parametrize("name", ["match-all", "match-none", "any-zero", "range-empty", "range-high"])
@pytest.mark.parametrize("beam", [64, 65])
def test_degenerate_predicates(name, beam):
    labels, kind, preds, claim = lc.CASES[name]
    kw = dict(beam=beam, k=10, out_k=10)
    # everything / nothing allowed: the masks of the existing "ones" / "zeros" kinds, and their references
    key = {"all": ("kinds", "ones", beam), "none": ("kinds", "zeros", beam)}.get(claim, ("label", name, beam))
    ref = _ref("f16", 32, kw, labels, kind, preds, key=key)
    if claim == "none":
        assert (ref["result_count"] == 0).all() and (ref["ids"] == 0xFFFFFFFF).all() and (ref["allowed_cmps"] == 0).all()
    if claim == "all":
        np.testing.assert_array_equal(ref["allowed_cmps"], ref["dist_cmps"])
    _run("f16", 32, kw, labels, kind, preds, ref)


# ---- labels on the handle ----

def test_set_labels_range_update_and_round_trip():
    ix = _index("f16", 32)
    _, Qd, _ = mc.device_rows("f16")
    labels, kind, preds, _ = lc.CASES["tenant"]
    kw = dict(beam=64, k=10, out_k=10)
    ix.set_labels(labels)
    np.testing.assert_array_equal(ix.labels(), labels)
    before = ix.batch_search_labeled(Qd, where=(kind, preds), **mc.search_kw(kw))
    # rows 100..199 rewritten: every one of them becomes a live point of tenant 1
    new = labels.copy()
    new[100:200] = np.uint32(0x00ABCD01)
    ix.set_labels(new[100:200], first_row=100)
    np.testing.assert_array_equal(ix.labels(), new)
    np.testing.assert_array_equal(ix.labels(150, 70), new[150:220])
    np.testing.assert_array_equal(ix.labels(mc.N - 1, 1), new[-1:])
    ref = _ref("f16", 32, kw, new, kind, preds, key=("label", "range-update"))
    old = _ref("f16", 32, kw, labels, kind, preds, key=("label", "f16", 32, 64, "rows", "tenant"))
    assert not np.array_equal(ref["ids"], old["ids"]) or not np.array_equal(ref["allowed_cmps"], old["allowed_cmps"])
    got = ix.batch_search_labeled(Qd, where=(kind, preds), **mc.search_kw(kw))
    _same_as_ref(ref, got)
    _same_as_ref(old, before)
    # a range outside [0, n) and a null pointer are refused and write nothing
    lib = _capi.load()
    one = np.zeros(8, np.uint32)
    p = one.ctypes.data_as(C.c_void_p)
    assert lib.pann_index_set_labels(ix.handle, mc.N - 7, p, 8) == _capi.PANN_ERR_BAD_ARG
    assert lib.pann_index_set_labels(ix.handle, mc.N + 1, p, 0) == _capi.PANN_ERR_BAD_ARG
    assert lib.pann_index_set_labels(ix.handle, 0, None, 8) == _capi.PANN_ERR_BAD_ARG
    assert lib.pann_index_get_labels(ix.handle, mc.N - 7, 8, p) == _capi.PANN_ERR_BAD_ARG
    assert lib.pann_index_get_labels(ix.handle, 0, 8, None) == _capi.PANN_ERR_BAD_ARG
    assert lib.pann_index_set_labels(None, 0, p, 8) == _capi.PANN_ERR_BAD_ARG
    assert (one == 0).all()
    np.testing.assert_array_equal(ix.labels(), new)


def test_set_labels_dev_and_a_fresh_handle_starts_at_zero():
    import torch
    lib = _capi.load()
    dev = torch.device("cuda", 0)
    X, _, _ = mc.device_rows("f16")
    ix = DeviceIndex(X, mc.graph(32))
    try:
        assert not ix.has_labels
        part = lc.range_labels()[500:1500]
        t = torch.from_numpy(part.view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        _capi.check(lib.pann_index_set_labels_dev(ix.handle, 500, C.c_void_p(t.data_ptr()), len(part)))     # the first call allocates
        assert ix.has_labels
        want = np.zeros(mc.N, np.uint32)
        want[500:1500] = part
        np.testing.assert_array_equal(ix.labels(), want)                  # (waits for the handle's stream)
        assert lib.pann_index_set_labels_dev(ix.handle, 2500, C.c_void_p(t.data_ptr()), len(part)) == _capi.PANN_ERR_BAD_ARG
        np.testing.assert_array_equal(ix.labels(), want)
        ix.drop_labels()
        assert not ix.has_labels
        with pytest.raises(PannError):
            ix.labels()
        # the quantised copy of a labeled handle has none
        Xf, _, _ = mc.device_rows("f32")
        fx = DeviceIndex(Xf, mc.graph(32))
        try:
            fx.set_labels(lc.tenant_labels())
            qx, _ = fx.quantized("euclid_u8")
            assert fx.has_labels and not qx.has_labels
            qx.close()
        finally:
            fx.close()
    finally:
        ix.close()


# ---- the device entry ----

def test_dev_entry_on_a_stream_equals_the_host_entry():
    import torch
    lib = _capi.load()
    dev = torch.device("cuda", 0)
    # f16 at 64: the label form of the register-frontier kernel; u8 at 64: its fallback; 65 / 300: the generic kernel
    for layout, beam, name in (("f16", 64, "tenant"), ("f16", 64, "range-straddle"), ("u8", 64, "range-rows"), ("f16", 65, "tenant"),
                               ("i8mips", 300, "tenant-shared")):
        ix = _index(layout, 32)
        labels, kind, preds, _ = lc.CASES[name]
        ix.set_labels(labels)
        _, Qd, _ = mc.device_rows(layout)
        kw = dict(k=10, beam=beam, cut=1.35, out_k=10, visited_cap=2048)
        host = ix.batch_search_labeled(Qd, where=(kind, preds), **kw)
        p = np.ascontiguousarray(np.asarray(preds, np.uint32).reshape(-1, 2))
        nq, ok, vc = mc.NQ, 10, 2048
        stream = torch.cuda.Stream(device=dev)
        assert stream.cuda_stream != 0
        t_q = torch.from_numpy(np.ascontiguousarray(Qd).view(np.uint8).reshape(nq, -1)).to(dev)
        t_p = torch.from_numpy(p.view(np.int32)).to(dev)
        t_st = torch.zeros(1, dtype=torch.int32, device=dev)
        t_ids = torch.zeros((nq, ok), dtype=torch.int32, device=dev)
        t_dist = torch.zeros((nq, ok), dtype=torch.float32, device=dev)
        t_cnt = [torch.zeros(nq, dtype=torch.int32, device=dev) for _ in range(6)]
        t_vid = torch.zeros((nq, vc), dtype=torch.int32, device=dev)
        t_vd = torch.zeros((nq, vc), dtype=torch.float32, device=dev)
        t_status = torch.full((1,), 77, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        _, d, _ = mc.LAYOUTS[layout]
        qp = _capi.QueryParams(k=10, beam=beam, cut=1.35, limit=mc.N, degree_limit=32, rerank_factor=100, pad=1.0)
        out = _capi.SearchOut(ids=t_ids.data_ptr(), dists=t_dist.data_ptr(), out_k=ok, frontier_size=t_cnt[0].data_ptr(),
                              visited_count=t_cnt[1].data_ptr(), dist_cmps=t_cnt[2].data_ptr(), degree_sum=t_cnt[3].data_ptr(),
                              visited_ids=t_vid.data_ptr(), visited_dists=t_vd.data_ptr(), visited_cap=vc, status=t_status.data_ptr())
        _capi.check(lib.pann_batch_search_labeled_dev(ix.handle, C.c_void_p(t_q.data_ptr()), None, nq, t_q.shape[1],
                                                      C.c_void_p(t_st.data_ptr()), 1, C.byref(qp), _capi.PANN_PRED_MATCH if kind == "match"
                                                      else _capi.PANN_PRED_RANGE, C.c_void_p(t_p.data_ptr()), len(p), C.byref(out),
                                                      C.c_void_p(t_cnt[4].data_ptr()), C.c_void_p(t_cnt[5].data_ptr()),
                                                      C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        assert int(t_status.cpu()[0]) == 0
        got = {"ids": t_ids, "dists": t_dist, "frontier_size": t_cnt[0], "visited_count": t_cnt[1], "dist_cmps": t_cnt[2],
               "degree_sum": t_cnt[3], "result_count": t_cnt[4], "allowed_cmps": t_cnt[5]}
        for f, t in got.items():
            np.testing.assert_array_equal(t.cpu().numpy().view(host[f].dtype), host[f], err_msg=f"{layout} b{beam} {f}")
        vids, vds = t_vid.cpu().numpy().view(np.uint32), t_vd.cpu().numpy()
        for i in range(nq):
            nv = int(host["visited_count"][i])
            np.testing.assert_array_equal(vids[i, :nv], host["visited_ids"][i, :nv])
            np.testing.assert_array_equal(vds[i, :nv], host["visited_dists"][i, :nv])
        # a predicate pointer that is not 8-byte aligned is refused before anything is launched
        assert lib.pann_batch_search_labeled_dev(ix.handle, C.c_void_p(t_q.data_ptr()), None, nq, t_q.shape[1], C.c_void_p(t_st.data_ptr()),
                                                 1, C.byref(qp), 1, C.c_void_p(t_p.data_ptr() + 4), 1, C.byref(out), None, None,
                                                 C.c_void_p(stream.cuda_stream)) == _capi.PANN_ERR_BAD_ARG


# ---- status ----

def test_refusals_leave_the_outputs_untouched():
    lib = _capi.load()
    _, Q, _ = mc.device_rows("u8")
    X, _, _ = mc.device_rows("u8")
    bare = DeviceIndex(X, mc.graph(32))                                   # a handle without labels
    ix = _index("u8", 32)
    ix.set_labels(lc.tenant_labels())
    preds = lc.TENANT_PREDS
    st = np.zeros(1, np.uint32)
    qp = _capi.QueryParams(k=10, beam=64, cut=1.35, limit=mc.N, degree_limit=32, rerank_factor=100, pad=1.0)
    MARK = 0xABABABAB

    def call(handle, kind=_capi.PANN_PRED_MATCH, p=preds, npreds=mc.NQ, out_k=10, beam=64):
        """-> (status code, every output still holds its marker)"""
        qp.beam = beam
        ids = np.full((mc.NQ, out_k), MARK, np.uint32)
        dists = np.full((mc.NQ, out_k), MARK, np.uint32)
        cnt = [np.full(mc.NQ, MARK, np.uint32) for _ in range(6)]
        out = _capi.SearchOut(ids=ids.ctypes.data_as(C.c_void_p), dists=dists.ctypes.data_as(C.c_void_p), out_k=out_k,
                              frontier_size=cnt[0].ctypes.data_as(C.c_void_p), visited_count=cnt[1].ctypes.data_as(C.c_void_p),
                              dist_cmps=cnt[2].ctypes.data_as(C.c_void_p), degree_sum=cnt[3].ctypes.data_as(C.c_void_p))
        rc = lib.pann_batch_search_labeled(handle, Q.ctypes.data_as(C.c_void_p), None, mc.NQ, Q.shape[1], st.ctypes.data_as(C.c_void_p), 1,
                                           C.byref(qp), kind, None if p is None else p.ctypes.data_as(C.c_void_p), npreds, C.byref(out),
                                           cnt[4].ctypes.data_as(C.c_void_p), cnt[5].ctypes.data_as(C.c_void_p))
        untouched = all((a == MARK).all() for a in [ids, dists, *cnt])
        if rc != _capi.PANN_OK:
            assert lib.pann_last_error()
        return rc, untouched

    try:
        assert call(ix.handle) == (_capi.PANN_OK, False)                                      # the valid call
        assert call(bare.handle) == (_capi.PANN_ERR_BAD_ARG, True)                            # no labels
        assert call(ix.handle, kind=3) == (_capi.PANN_ERR_BAD_ARG, True)                      # unknown kinds
        assert call(ix.handle, kind=-1) == (_capi.PANN_ERR_BAD_ARG, True)
        assert call(ix.handle, p=None) == (_capi.PANN_ERR_BAD_ARG, True)                      # null predicates
        assert call(ix.handle, npreds=2) == (_capi.PANN_ERR_BAD_ARG, True)                    # npreds = 2 with nq = 8
        assert call(ix.handle, npreds=0) == (_capi.PANN_ERR_BAD_ARG, True)
        assert call(ix.handle, out_k=65, beam=128) == (_capi.PANN_ERR_UNSUPPORTED, True)      # as the bitmap twin
        assert call(ix.handle, out_k=65, beam=64) == (_capi.PANN_ERR_BAD_ARG, True)           # out_k > beam
        assert call(ix.handle, npreds=1) == (_capi.PANN_OK, False)                            # preds[0] for the whole batch
        with pytest.raises(ValueError):
            ix.batch_search_labeled(Q, where=("match", np.zeros((mc.NQ + 1, 2), np.uint32)), k=10, beam=64)
        with pytest.raises(ValueError):
            ix.batch_search_labeled(Q, where=("sometimes", (1, 1)), k=10, beam=64)
        with pytest.raises(PannError) as e:
            bare.batch_search_labeled(Q, where=("any", (1, 0)), k=10, beam=64)
        assert e.value.code == _capi.PANN_ERR_BAD_ARG and "labels" in str(e.value)
        # nq == 0 is fine, and the handle still works
        assert lib.pann_batch_search_labeled(ix.handle, Q.ctypes.data_as(C.c_void_p), None, 0, Q.shape[1], st.ctypes.data_as(C.c_void_p), 1,
                                             C.byref(qp), 1, preds.ctypes.data_as(C.c_void_p), 1,
                                             C.byref(_capi.SearchOut(ids=None, out_k=10)), None, None) == _capi.PANN_OK
        g = ix.batch_search_labeled(Q, where=("match", (0, 0)), k=10, beam=64)
        assert (g["result_count"] == 10).all()
    finally:
        bare.close()


# ---- the Python mirror ----

def test_python_mirror_routes_where_to_the_labeled_search(tmp_path):
    from parlayann_amd import io
    from parlayann_amd.graph_index import FloatEuclidianIndex
    X, Q, _, _ = mc.layout_data("f32")
    io.write_bin(tmp_path / "b.bin", X)
    io.write_graph(tmp_path / "g.graph", mc.graph(32))
    labels, kind, preds, _ = lc.CASES["tenant"]
    gi = FloatEuclidianIndex(str(tmp_path / "b.bin"), str(tmp_path / "g.graph"), labels=labels)
    try:
        assert gi.index.has_labels and gi.q_index.has_labels
        rows = label_allow(labels, kind, preds)
        ids, dists = gi.batch_search(Q, 10, 64, visit_limit=1000, where=(kind, preds))
        ref = mc.reference("f32", 32, dict(beam=64, k=10, out_k=10, limit=1000), rows)
        np.testing.assert_array_equal(ids, ref["ids"]); np.testing.assert_array_equal(dists, ref["dists"])
        ids2, dists2 = gi.batch_search_masked(Q, 10, 64, visit_limit=1000, where=(kind, preds))
        np.testing.assert_array_equal(ids2, ids); np.testing.assert_array_equal(dists2, dists)
        # the quantised route equals the bitmap call of the same route
        a, b = gi.batch_search_masked(Q, 10, 64, quant=True, visit_limit=1000, where=(kind, preds))
        c, d = gi.batch_search_masked(Q, 10, 64, rows, quant=True, visit_limit=1000)
        np.testing.assert_array_equal(a, c); np.testing.assert_array_equal(b, d)
        # exact_below through label_count: the split equals the bitmap form's
        cnt = gi.index.label_count((kind, preds))
        np.testing.assert_array_equal(cnt, rows.sum(axis=1))
        cut = int(np.median(cnt))
        assert (cnt <= cut).any() and (cnt > cut).any()
        e1 = gi.batch_search_masked(Q, 10, 64, visit_limit=1000, exact_below=cut, where=(kind, preds))
        e2 = gi.batch_search_masked(Q, 10, 64, rows, visit_limit=1000, exact_below=cut)
        np.testing.assert_array_equal(e1[0], e2[0]); np.testing.assert_array_equal(e1[1], e2[1])
        assert not np.array_equal(e1[0], ids)                                   # some rows did take the exact route
        shared = gi.batch_search(Q, 10, 64, visit_limit=1000, where=("match", (0xFF, 2)), exact_below=mc.N)
        e3 = gi.batch_search(Q, 10, 64, visit_limit=1000, allow=label_allow(labels, "match", (0xFF, 2)), exact_below=mc.N)
        np.testing.assert_array_equal(shared[0], e3[0]); np.testing.assert_array_equal(shared[1], e3[1])
        with pytest.raises(ValueError):
            gi.batch_search(Q, 10, 64, visit_limit=1000, where=(kind, preds), allow=rows)
        with pytest.raises(ValueError):
            gi.batch_search_masked(Q, 10, 64, rows, visit_limit=1000, where=(kind, preds))
        with pytest.raises(ValueError):
            gi.batch_search(Q, 10, 64, quant=True, visit_limit=1000, where=(kind, preds))
    finally:
        gi.index.close()
        if gi.q_index is not None:
            gi.q_index.close()
