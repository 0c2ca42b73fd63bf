"""Steered masked search on the device (pann_batch_search_steered*, DESIGN.md "Steered masked search") against the restatement
tests/steered_ref.py, bit for bit on integer-valued data: ids, dists, result_count, allowed_cmps, the four plain counters, the
visited lists, bridge_rows and hop2_cmps.  The cases are those of tests/steered_cases.py; every shared mask also runs as one row
per query, the label forms run on the same content and must equal the bitmap form bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filtered_cases as fc
import steered_cases as sc
import steered_ref
from parlayann_amd import DeviceIndex, PannError, _capi

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("frontier_size", "visited_count", "dist_cmps", "degree_sum", "result_count", "allowed_cmps", "bridge_rows", "hop2_cmps")
_handles = {}


def _index(layout, deg):
    if (layout, deg) not in _handles:
        X, _, metric = sc.layout_data(layout)
        _handles[(layout, deg)] = DeviceIndex(X, sc.graph(layout, deg), metric=metric)
    return _handles[(layout, deg)]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for ix in _handles.values():
        ix.close()
    _handles.clear()


def _same(ref, got, what=""):
    assert got["status"][0] == 0
    np.testing.assert_array_equal(ref["ids"], got["ids"], err_msg=what + " ids")
    assert got["dists"].dtype == F and not np.isnan(got["dists"]).any()
    np.testing.assert_array_equal(ref["dists"], got["dists"], err_msg=what + " dists")
    for f in COUNTERS:
        np.testing.assert_array_equal(ref[f], got[f], err_msg=what + " " + f)
    if ref.get("visited_ids") is not None and got.get("visited_ids") is not None:
        for i in range(len(ref["ids"])):
            nv = int(ref["visited_count"][i])
            np.testing.assert_array_equal(ref["visited_ids"][i, :nv], got["visited_ids"][i, :nv], err_msg=what + " visited_ids")
            np.testing.assert_array_equal(ref["visited_dists"][i, :nv], got["visited_dists"][i, :nv], err_msg=what + " visited_dists")


def _query(layout, kw):
    return dict(query_ids=sc.QUERY_IDS) if kw.get("query_ids") else dict(queries=sc.layout_data(layout)[1])


@pytest.mark.parametrize("case", sc.CASES, ids=sc.CASE_IDS)
def test_steered_search_equals_the_restatement(case):
    name, layout, deg, kw, T, per_query, fill = case
    ref = sc.reference(case)
    m = sc.case_mask(case)
    G = sc.graph(layout, deg)
    if deg != 80:
        assert (G[:, 0] < deg).any()                             # truncated rows: shorter than max_deg, sentinel-padded on the device
    if T > 1:
        assert ref["bridge_rows"].sum() > 0 and ref["hop2_cmps"].sum() > 0
    if T == 0:                                                   # nobody allowed, the start neither: empty rows
        assert (ref["result_count"] == 0).all() and (ref["ids"] == 0xFFFFFFFF).all() and (ref["allowed_cmps"] == 0).all()
    if len(kw.get("starts", ())) == 3:
        assert (ref["dist_cmps"] == ref["allowed_cmps"] + 1).all()      # the disallowed start is the only disallowed point with a distance
    ix = _index(layout, deg)
    q, skw = _query(layout, kw), sc.search_kw(kw)
    rows = np.broadcast_to(m, (sc.NQ, sc.N))
    got = ix.batch_search_masked(allow=sc.pack(rows), steer=fill, **q, **skw)
    _same(ref, got, "per-query rows")
    if m.ndim == 1:                                              # one shared bitmap, dead bits set; and as a boolean array
        _same(ref, ix.batch_search_masked(allow=sc.pack(m), steer=fill, **q, **skw), "shared")
        _same(ref, ix.batch_search_masked(allow=m, steer=fill, **q, **skw), "boolean")
    else:                                                        # a stride larger than a row
        wide = np.full((sc.NQ, sc.WORDS + 3), 0xFFFFFFFF, np.uint32)
        wide[:, :sc.WORDS] = sc.pack(rows)
        _same(ref, ix.batch_search_masked(allow=wide, steer=fill, **q, **skw), "wide stride")
    found = got["ids"] != 0xFFFFFFFF
    assert rows[np.nonzero(found)[0], got["ids"][found]].all()   # hard: a disallowed id is never returned


LABEL_RUNS = [(layout, beam, T, pq, kind) for layout, beam, T in (("f16", 64, 20), ("u8", 100, 2), ("f32", 32, 0))
              for pq in (False, True) for kind in ("any", "match", "range")]


@pytest.mark.parametrize("layout,beam,T,per_query,kind", LABEL_RUNS,
                         ids=[f"{l}-b{b}-T{t}-{'rows' if p else 'shared'}-{k}" for l, b, t, p, k in LABEL_RUNS])
def test_labeled_equals_bitmap_and_restatement(layout, beam, T, per_query, kind):
    ix = _index(layout, 32)
    X, Q, metric = sc.layout_data(layout)
    m = sc.mask(T, per_query)
    kw = dict(k=10, beam=beam, out_k=10, cut=1.35, visited_cap=2048)
    key = ("label", layout, beam, T, per_query)
    if key not in sc._refs:
        sc._refs[key] = steered_ref.steered_batch_search(X, sc.graph(layout, 32), m, fill=16, metric=metric, queries=Q, **kw)
    ref = sc._refs[key]
    bitmap = ix.batch_search_masked(Q, allow=sc.pack(m), steer=16, **kw)
    _same(ref, bitmap, "bitmap")
    lab, preds = sc.labels_of(T, kind, per_query)
    ix.set_labels(lab)
    try:
        got = ix.batch_search_labeled(Q, where=(kind, preds), steer=16, **kw)
        _same(ref, got, "labeled")
        for f in ("ids", "dists", "visited_ids", "visited_dists") + COUNTERS:
            np.testing.assert_array_equal(bitmap[f], got[f], err_msg=f)        # the labeled result IS the bitmap result
        if not per_query:                                         # one predicate given as nq equal rows
            rows = np.ascontiguousarray(np.broadcast_to(np.asarray(preds, np.uint32), (sc.NQ, 2)))
            _same(ref, ix.batch_search_labeled(Q, where=(kind, rows), steer=16, **kw), "labeled rows")
    finally:
        ix.drop_labels()


@pytest.mark.parametrize("layout,beam", [("f16", 64), ("u8", 100), ("bf16", 200), ("i8mips", 8)])
def test_all_ones_mask_equals_the_masked_search_on_the_device(layout, beam):
    ix = _index(layout, 32)
    _, Q, _ = sc.layout_data(layout)
    kw = dict(k=min(10, beam), beam=beam, out_k=min(10, beam), cut=1.35, visited_cap=2048)
    ones = sc.pack(np.ones(sc.N, bool))
    want = ix.batch_search_masked(Q, allow=ones, **kw)
    assert "bridge_rows" not in want                             # steer=None is today's call
    for fill in (1, 16, 0, 37):
        got = ix.batch_search_masked(Q, allow=ones, steer=fill, **kw)
        for f in ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum", "result_count", "allowed_cmps"):
            np.testing.assert_array_equal(want[f], got[f], err_msg=f"fill {fill} {f}")
        for i in range(sc.NQ):
            nv = int(want["visited_count"][i])
            np.testing.assert_array_equal(want["visited_ids"][i, :nv], got["visited_ids"][i, :nv])
        assert not got["bridge_rows"].any() and not got["hop2_cmps"].any()


@pytest.mark.parametrize("n", [33, 64])
def test_last_bitmap_word(n):
    """n = 33: one live bit in the last word; n = 64: the last word is full.  Bits at positions >= n are set and ignored."""
    X, Q, _ = sc.layout_data("u8")
    X, Q = np.ascontiguousarray(X[:n]), np.ascontiguousarray(Q[:16])
    G = fc.random_graph(n, 16, 700 + n)                          # degrees 4..16
    m = np.random.default_rng(n).random(n) < 0.3
    m[n - 1] = True; m[0] = False
    packed = sc.pack(m, n)
    if n % 32:
        assert packed[-1] >> (n % 32) == (1 << (32 - n % 32)) - 1     # the dead bits are set
    kw = dict(k=5, beam=16, out_k=10, cut=1.35, visited_cap=64)
    ref = steered_ref.steered_batch_search(X, G, m, fill=0, queries=Q, **kw)
    assert (ref["ids"] == n - 1).any() and ref["bridge_rows"].sum() > 0
    ix = DeviceIndex(X, G)
    try:
        _same(ref, ix.batch_search_masked(Q, allow=packed, steer=0, **kw), "shared")
        _same(ref, ix.batch_search_masked(Q, allow=np.broadcast_to(packed, (16, len(packed))).copy(), steer=0, **kw), "rows")
    finally:
        ix.close()


def test_table_in_hbm_at_the_planned_beam(tmp_path):
    """the smallest beam at which make_plan moves the steered layout's filter table to HBM (persistent blocks), and the one below"""
    exe = str(tmp_path / "steer_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "steer_plan_check.cpp")])
    beam = int(subprocess.check_output([exe, "hbm_beam", "32", "32", "32", "1"], text=True))
    assert 64 < beam <= 300
    X, Q, metric = sc.layout_data("u8")
    ix = _index("u8", 32)
    m = sc.mask(20, True)[:16]
    for b in (beam - 1, beam):
        kw = dict(k=10, beam=b, out_k=10, cut=1.35, visited_cap=2048)
        ref = steered_ref.steered_batch_search(X, sc.graph("u8", 32), m, fill=0, metric=metric, queries=Q[:16], **kw)
        _same(ref, ix.batch_search_masked(Q[:16], allow=sc.pack(m), steer=0, **kw), f"beam {b}")


def test_graph_index_forwards_steer(tmp_path):
    from parlayann_amd import io
    from parlayann_amd.graph_index import UInt8EuclidianIndex
    X, Q, _ = sc.layout_data("u8")
    io.write_bin(tmp_path / "b.bin", X)
    io.write_graph(tmp_path / "g.graph", sc.graph("u8", 32))
    m = sc.mask(20, False)
    lab, preds = sc.labels_of(20, "match", False)
    gi = UInt8EuclidianIndex(str(tmp_path / "b.bin"), str(tmp_path / "g.graph"), labels=lab)
    try:
        want = _index("u8", 32).batch_search_masked(Q, allow=m, steer=8, k=10, beam=64, limit=1000)
        for kw in (dict(allow=m), dict(where=("match", preds))):
            ids, dists = gi.batch_search(Q, 10, 64, visit_limit=1000, steer=8, **kw)
            np.testing.assert_array_equal(ids, want["ids"]); np.testing.assert_array_equal(dists, want["dists"])
        plain = gi.batch_search(Q, 10, 64, visit_limit=1000, allow=m)        # steer=None: today's masked search
        assert (plain[0] != ids).any()
        with pytest.raises(ValueError):
            gi.batch_search(Q, 10, 64, steer=8)                               # steering needs a filter
    finally:
        gi.index.close()
        if gi.q_index is not None:
            gi.q_index.close()


def test_refusals():
    ix = _index("u8", 32)
    _, Q, _ = sc.layout_data("u8")
    lib = _capi.load()
    ones = sc.pack(np.ones(sc.N, bool))
    st = np.zeros(1, np.uint32)
    qp = _capi.QueryParams(k=10, beam=64, cut=1.35, limit=sc.N, degree_limit=32, rerank_factor=100, pad=1.0)
    POISON = 0xA5A5A5A5

    def refused(out_k, beam, k=10, allow=ones, stride=0):
        qp.beam, qp.k = beam, k
        ids = np.full((sc.NQ, out_k), POISON, np.uint32)
        steer = np.full((sc.NQ, 2), POISON, np.uint32)
        out = _capi.SearchOut(ids=ids.ctypes.data_as(C.c_void_p), out_k=out_k)
        rc = lib.pann_batch_search_steered(ix.handle, Q.ctypes.data_as(C.c_void_p), None, sc.NQ, Q.shape[1], st.ctypes.data_as(C.c_void_p), 1,
                                           C.byref(qp), None if allow is None else allow.ctypes.data_as(C.c_void_p), stride, C.byref(out),
                                           None, None, 8, steer.ctypes.data_as(C.c_void_p))
        if rc != 0:
            assert lib.pann_last_error()                                       # a non-empty message
            assert (ids == POISON).all() and (steer == POISON).all()           # and no output written
        return rc

    assert refused(10, 64) == 0                                                # the valid call
    assert refused(65, 128) == _capi.PANN_ERR_UNSUPPORTED                      # out_k > 64
    assert refused(65, 64) == _capi.PANN_ERR_BAD_ARG                           # out_k > beam
    assert refused(10, 8, k=10) == _capi.PANN_ERR_BAD_ARG                      # k > beam
    assert refused(10, 64, allow=None) == _capi.PANN_ERR_BAD_ARG               # null bitmap
    assert refused(10, 64, stride=sc.WORDS - 1) == _capi.PANN_ERR_BAD_ARG      # a stride shorter than a bitmap row
    # the sketch filter: no entry point takes a sketch together with a mask, steered or not
    with pytest.raises(TypeError):
        ix.batch_search_masked(Q, allow=ones, steer=0, k=10, beam=64, sketch_queries=np.zeros((sc.NQ, 16), np.uint8))
    with pytest.raises(ValueError):
        ix.batch_search_masked(Q, allow=ones, steer=-1, k=10, beam=64)
    with pytest.raises(PannError) as e:                                        # labeled form on a handle without labels
        ix.batch_search_labeled(Q, where=("any", (1, 0)), steer=0, k=10, beam=64)
    assert str(e.value)
    out = _capi.SearchOut(ids=None, out_k=10)
    qp.beam, qp.k = 64, 10
    assert lib.pann_batch_search_steered_dev(ix.handle, None, None, sc.NQ, 32, None, 1, C.byref(qp), None, 0, C.byref(out), None, None, 0, None,
                                             None) == _capi.PANN_ERR_BAD_ARG   # the device entry checks before it launches anything
    g = ix.batch_search_masked(Q, allow=ones, steer=0, k=10, beam=64)          # the handle still works
    assert (g["result_count"] == 10).all()
