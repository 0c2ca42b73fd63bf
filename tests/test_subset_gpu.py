"""pann_index_create_subset* on the device against the numpy restatement of its rule (tests/subset_ref.py), bit for bit, over the
case tables of tests/subset_cases.py; then the new handle as an index in its own right: searched against a twin created from
host memory, cross-checked with the exact masked kNN, built, compacted after deletions and grown."""
import ctypes as C

import numpy as np
import pytest

import subset_cases as sc
import subset_ref as sr
from parlayann_amd import DeviceIndex, PannError, _capi, allow_bitmap, datasets, label_allow, sketch
from parlayann_amd.index import pack_allow

pytestmark = pytest.mark.gpu

BAD_ARG, OVERFLOW = _capi.PANN_ERR_BAD_ARG, _capi.PANN_ERR_OVERFLOW
_src = {}


def make_index(layout, X, G):
    dtype, metric, d, _ = sc.LAYOUTS[layout]
    if dtype == "u4":
        return DeviceIndex.from_packed(X, d, "u4", graph=G)
    return DeviceIndex(X, G, metric=metric)


def source(layout, n, sketch_kind=None):
    """the source handle of a case, with labels (and a sketch of its own rows: f32 layouts only); made once, never changed"""
    key = (layout, n, sketch_kind)
    if key not in _src:
        X, G, L = sc.case(layout, n)
        ix = make_index(layout, X, G)
        ix.set_labels(L)
        if sketch_kind is not None:
            sketch.attach_sketch(ix, ix, sketch.sketch_params(ix, sketch_kind))
        _src[key] = ix
    return _src[key]


@pytest.fixture(scope="module", autouse=True)
def _close_sources():
    yield
    for ix in _src.values():
        ix.close()
    _src.clear()


def downloaded(ix, n2o=None, o2n=None):
    return dict(points=sc.points_bytes(ix.points()), graph=ix.get_graph(), labels=ix.labels() if ix.has_labels else None,
                sketch=sketch.download_sketch(ix) if sketch.attached_kind(ix) >= 0 else None, new_to_old=n2o, old_to_new=o2n)


def reference(layout, n, mask, n_out=0, copy_graph=True, sk=None):
    X, G, L = sc.case(layout, n)
    return sr.subset_ref(sc.points_bytes(X), G, L, sk, None if mask is None else sc.masks(n)[mask], n_out, copy_graph)


# (layout, n, mask, sketch kind): every layout x mask at the big size, the baseline layout at the two other sizes; the f32 layout
# carries a two-bit sketch, and a one-bit sketch in a case of its own
CONTENTS = [(lay, sc.N_BIG, m, "mips_2bit" if lay == "f32" else None) for lay in sc.LAYOUTS for m in sc.mask_names(sc.N_BIG)] + \
           [("f32", sc.N_BIG, "50pct", "euclid_bit")] + \
           [("u8", n, m, None) for n in (sc.N_BLOCK, sc.N_SMALL) for m in sc.mask_names(n)]


def _capacity(mask, m):
    """`none` needs room to exist at all; 1pct gets seven rows past the kept ones (zero rows, empty graph rows, zero labels)"""
    return 5 if mask == "none" else (m + 7 if mask == "1pct" else None)


@pytest.mark.parametrize("layout,n,mask,sk_kind", CONTENTS, ids=[f"{a}-{b}-{c}" + (f"-{d}" if d else "") for a, b, c, d in CONTENTS])
def test_contents_bit_for_bit(layout, n, mask, sk_kind):
    src = source(layout, n, sk_kind)
    before = downloaded(src)
    m = len(sr.kept_ids(sc.masks(n)[mask], n))
    cap = _capacity(mask, m)
    sub, n2o, o2n = src.subset(sc.masks(n)[mask], capacity=cap)
    try:
        ref = reference(layout, n, mask, cap or 0, sk=before["sketch"])
        assert sub.n == (cap or m) and sub.d == src.d and sub.max_degree == src.max_degree
        assert sr.same(downloaded(sub, n2o, o2n), ref) is None, sr.same(downloaded(sub, n2o, o2n), ref)
        assert sketch.attached_kind(sub) == sketch.attached_kind(src)
        if mask == "none":
            assert not sub.points().any() and not sub.get_graph().any() and not sub.labels().any() and len(n2o) == 0
        # the graph can be left out, and the maps with it
        bare = src.subset(sc.masks(n)[mask], capacity=cap, copy_graph=False, maps=False)
        try:
            assert sr.same(downloaded(bare, n2o, o2n), reference(layout, n, mask, cap or 0, copy_graph=False, sk=before["sketch"])) is None
        finally:
            bare.close()
    finally:
        sub.close()
    assert sr.same(downloaded(src), before) is None                                # src reads back unchanged
    X, G, L = sc.case(layout, n)
    assert np.array_equal(before["points"], sc.points_bytes(X)) and np.array_equal(before["graph"], G) and np.array_equal(before["labels"], L)


@pytest.mark.parametrize("layout", ["u8", "f16"])
def test_the_handle_is_whole_searches_equal_a_twin_from_host_memory(layout):
    """padding bytes, strides and per-handle state: the subset searched like an index created from the reference's arrays"""
    n = sc.N_BIG
    src = source(layout, n)
    sub = src.subset(sc.masks(n)["50pct"], maps=False)
    ref = reference(layout, n, "50pct")
    dtype, metric, _, _ = sc.LAYOUTS[layout]
    twin = DeviceIndex(ref["points"].view(dtype), ref["graph"], metric=metric)
    try:
        Q = sc.queries(layout)
        qids = np.arange(0, sub.n, 97, dtype=np.uint32)
        start = int(np.argmax(ref["graph"][:, 0]))                                 # a row with neighbours left: the walks go somewhere
        for beam in (64, 100):
            for kw in (dict(queries=Q), dict(query_ids=qids)):
                a, b = (ix.batch_search(k=10, beam=beam, starts=(start,), **kw) for ix in (sub, twin))
                for f in ("ids", "dists", "visited_count", "dist_cmps"):
                    assert np.array_equal(a[f], b[f]), (beam, list(kw), f)
                assert a["visited_count"].max() > 1
    finally:
        sub.close()
        twin.close()


@pytest.mark.parametrize("layout", ["u8", "i8"])
@pytest.mark.parametrize("mask", ["50pct", "1pct"])
def test_bruteforce_on_the_subset_is_the_exact_masked_knn_on_src(layout, mask):
    n = sc.N_BIG
    src = source(layout, n)
    sub, n2o, _ = src.subset(sc.masks(n)[mask])
    try:
        Q = sc.queries(layout)
        ids, dists = sub.bruteforce_knn(Q, 10)
        mids, mdists, counts = src.bruteforce_knn_masked(Q, 10, sc.masks(n)[mask])
        assert (counts == 10).all() and np.array_equal(n2o[ids], mids) and np.array_equal(dists, mdists)
    finally:
        sub.close()


def test_predicate_form_equals_the_bitmap_of_the_predicate():
    n = sc.N_BIG
    src = source("u8", n)
    where = ("match", (7, 3))
    allow = label_allow(sc.labels(n), *where)
    assert 0 < allow.sum() < n
    a, a_n2o, a_o2n = src.subset(where=where)
    b, b_n2o, b_o2n = src.subset(allow=allow)
    try:
        assert sr.same(downloaded(a, a_n2o, a_o2n), downloaded(b, b_n2o, b_o2n)) is None
        assert sr.same(downloaded(a, a_n2o, a_o2n), sr.subset_ref(sc.points_bytes(sc.points("u8", n)), sc.graph("u8", n), sc.labels(n), None,
                                                                   pack_allow(allow, n))) is None
        assert (a.labels() & 7 == 3).all()
        with pytest.raises(ValueError):
            src.subset(allow=allow, where=where)
    finally:
        a.close()
        b.close()
    X, G, _ = sc.case("u8", sc.N_SMALL)
    bare = DeviceIndex(X, G)
    try:
        with pytest.raises(PannError) as e:
            bare.subset(where=where)
        assert e.value.code == BAD_ARG
    finally:
        bare.close()


def test_dedicated_index_builds_like_a_twin_from_host_memory():
    n, layout = sc.N_BIG, "u8_w65"
    src = source(layout, n)
    sub, n2o, _ = src.subset(sc.masks(n)["1pct"], copy_graph=False)
    twin = DeviceIndex(sc.points(layout, n)[n2o], max_degree=sc.LAYOUTS[layout][3])
    try:
        assert not sub.get_graph().any()
        for ix in (sub, twin):
            ix.vamana_build(16, 32, 1.2, seed=1)
        g = sub.get_graph()
        assert np.array_equal(g, twin.get_graph()) and g[:, 0].min() > 0
    finally:
        sub.close()
        twin.close()


# ---- a dynamic index: built, deleted from, compacted; grown and inserted into ----
N_DYN, D_DYN, R_DYN, L_DYN, ALPHA = 2000, 24, 32, 64, 1.2


@pytest.fixture(scope="module")
def built():
    """(index with labels and a built graph, its rows): n = 2 000 uint8 points"""
    X = datasets.sift_like(N_DYN, D_DYN, seed=1234, dtype=np.uint8)
    ix = DeviceIndex(X, max_degree=R_DYN)
    ix.set_labels(sc.labels(N_DYN))
    ix.vamana_build(R_DYN, L_DYN, ALPHA, seed=1)
    yield ix, X
    ix.close()


def test_growth_then_insert(built):
    ix, X = built
    n = ix.n
    G = ix.get_graph()
    big, n2o, o2n = ix.subset(capacity=n + 100)
    try:
        assert big.n == n + 100 and np.array_equal(n2o, np.arange(n)) and np.array_equal(o2n, np.arange(n))
        ref = sr.subset_ref(sc.points_bytes(X), G, sc.labels(n), None, None, n + 100)
        assert sr.same(downloaded(big, n2o, o2n), ref) is None
        assert not big.points()[n:].any() and not big.get_graph()[n:].any() and not big.labels()[n:].any()
        new_rows = datasets.sift_like(100, D_DYN, seed=99, dtype=np.uint8)
        big.upload_points(n, new_rows)
        new_ids = np.arange(n, n + 100, dtype=np.uint32)
        big.vamana_insert_batch(new_ids, R_DYN, L_DYN, ALPHA, start=0)
        assert (big.get_graph()[n:, 0] > 0).all()                                  # the new rows are non-empty
        r = big.batch_search(query_ids=new_ids[:1], k=10, beam=64)                 # returns OK
        assert (r["ids"] < big.n).all()
    finally:
        big.close()
    assert np.array_equal(ix.get_graph(), G) and ix.n == n


def test_lifecycle_compaction_after_deletions(built):
    ix, X = built
    n = ix.n
    G0 = ix.get_graph()
    D = (1 + np.random.default_rng(8).choice(n - 1, 200, replace=False)).astype(np.uint32)       # never vertex 0, the start
    ix.vamana_delete_batch(D, R_DYN, ALPHA)
    try:
        G1 = ix.get_graph()
        live = np.arange(R_DYN)[None, :] < G1[:, :1]
        assert not (live & np.isin(G1[:, 1:], D)).any() and not G1[D].any()        # the consolidation left no edge into D
        allow = allow_bitmap(n, deleted_ids=D)
        sub, n2o, o2n = ix.subset(allow)
        try:
            assert sub.n == n - 200 and np.array_equal(n2o, np.setdiff1d(np.arange(n), D))
            g = sub.get_graph()
            assert np.array_equal(g[:, 0], G1[n2o, 0])                             # every row keeps its degree
            assert sr.same(downloaded(sub, n2o, o2n), sr.subset_ref(sc.points_bytes(X), G1, sc.labels(n), None, allow)) is None
            start = int(o2n[0])
            assert start != sr.DROPPED
            r = sub.batch_search(datasets.sift_like(16, D_DYN, seed=4321, dtype=np.uint8), k=10, beam=64, starts=(start,))
            assert (r["ids"] < sub.n).all() and (r["visited_count"] > 1).all()
        finally:
            sub.close()
    finally:
        ix.set_graph(G0)               # the module's index as the other tests expect it


def test_status_codes_leave_everything_as_it_was():
    n = sc.N_BIG
    src = source("u8", n)
    m50 = len(sr.kept_ids(sc.masks(n)["50pct"], n))

    def searchable():
        r = src.batch_search(query_ids=np.arange(8, dtype=np.uint32), k=5, beam=64)
        assert (r["ids"] < n).all()

    with pytest.raises(PannError) as e:
        src.subset(sc.masks(n)["50pct"], capacity=m50 - 1)
    assert e.value.code == BAD_ARG
    searchable()
    with pytest.raises(PannError) as e:
        src.subset(sc.masks(n)["none"])
    assert e.value.code == BAD_ARG
    searchable()
    with pytest.raises(PannError) as e:
        src.subset(capacity=(1 << 31) - 1)
    assert e.value.code == BAD_ARG
    # through the C-ABI: a new_to_old array one entry short
    lib = _capi.load()
    allow = sc.masks(n)["50pct"]
    FILL = 0xABCDEF01
    n2o, o2n = np.full(n, FILL, np.uint32), np.full(n, FILL, np.uint32)
    out, kept = C.c_void_p(), C.c_uint64(0)
    rc = lib.pann_index_create_subset(C.byref(out), src.handle, allow.ctypes.data_as(C.c_void_p), 0, 1, n2o.ctypes.data_as(C.c_void_p),
                                      m50 - 1, o2n.ctypes.data_as(C.c_void_p), C.byref(kept))
    assert rc == OVERFLOW and kept.value == m50 and out.value is None and (n2o == FILL).all() and (o2n == FILL).all()
    searchable()
    # ... and with exactly enough room it succeeds, writing m entries and no more
    rc = lib.pann_index_create_subset(C.byref(out), src.handle, allow.ctypes.data_as(C.c_void_p), 0, 1, n2o.ctypes.data_as(C.c_void_p),
                                      m50, None, C.byref(kept))
    assert rc == _capi.PANN_OK and out.value is not None
    lib.pann_index_destroy(out)
    assert np.array_equal(n2o[:m50], sr.kept_ids(allow, n)) and (n2o[m50:] == FILL).all() and (o2n == FILL).all()
