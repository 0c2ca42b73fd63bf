"""FP8 (E4M3) rows on the device (PANN_F8, PANN_QUANT_F8; include/pann.h, DESIGN.md "FP8 rows").  An FP8 value widens exactly to f32, so
every distance is the f32 distance of the widened rows.  Grid data (m * 2^s, |m| <= 8, s in {0, -3}) keeps every sum exact in any order:
results equal float64 and the oracle's f32 search bit for bit, with frequent ties.  Real data (every non-NaN code) is used in
exact-float-order mode.  (No exact-kNN cases: pann_bruteforce_knn refuses an FP8 handle, DESIGN.md "FP8 rows".)"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import float_cases as fc
import masked_ref
import oracle_api
from parlayann_amd import DeviceIndex, _capi, datasets, io, label_allow, quantize
from parlayann_amd import sketch as sk
from parlayann_amd.fp8 import TABLE, float8_e4m3, from_f8, to_f8
from parlayann_amd.graph_index import FloatEuclidianIndex, FloatMipsIndex
from test_quant4_gpu import CASES, _buf, _device_rows_dev, _same_search, _vp

pytestmark = pytest.mark.gpu
F, U32 = np.float32, np.uint32
CODES = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)
N, NQ, R, L = 2000, 64, 16, 32
METRICS = [("Euclidian", "l2"), ("mips", "mips")]


def _grid(n, d, seed):
    rng = np.random.default_rng(seed)
    return to_f8((rng.integers(-8, 9, (n, d)) * np.where(rng.random((n, 1)) < 0.5, 1.0, 0.125)).astype(F))


def _real(n, d, seed):
    return np.random.default_rng(seed).choice(CODES, (n, d)).view(float8_e4m3)


def test_every_code_widens_exactly():
    X = np.zeros((1, 16), np.uint8); X[0, 0] = 0x38                       # one-hot row: 1.0 at coordinate 0
    Q = np.zeros((len(CODES), 16), np.uint8); Q[:, 0] = CODES
    ix = DeviceIndex(X.view(float8_e4m3), max_degree=4, metric="mips")
    got = ix.query_distances(Q.view(float8_e4m3), [0])[:, 0]
    ix.close()
    assert np.array_equal((-got + F(0)).view(U32), (TABLE[CODES] + F(0)).view(U32))      # -(q * 1); the sign of a zero is no result


@pytest.mark.parametrize("d", [33, 128, 200])
@pytest.mark.parametrize("metric", ["Euclidian", "mips"])
def test_quantiser_parity(d, metric):
    rng = np.random.default_rng(d)
    X = (rng.standard_normal((257, d)) * 3).astype(F)
    Q = from_f8(_real(257, d, d + 1)) * F(0.5)                                           # x * 2 is every E4M3 value ...
    mid = (TABLE[CODES[:-1] & 0x7F][:120] + TABLE[(CODES[:-1] & 0x7F) + 1][:120]) / 4    # ... and x * 2 the midpoint of two codes
    Q[0, :33] = mid[:33]; Q[1, :33] = -mid[33:66]; Q[2, :33] = mid[66:99]                # ties, the subnormal range included
    Q[3, :6] = [224.0, 224.5, -300.0, 1e18, -0.0, 1e-18]                                 # at and beyond 448 after scaling, -0, underflow
    full = DeviceIndex(X, max_degree=4, metric=metric)
    try:
        p = full.quantize_params("f8")
        slope, M = quantize.f8_params(X)
        assert (p.kind, F(p.slope), p.offset, F(p.max_val)) == (_capi.PANN_QUANT_F8, slope, 0, M) and M * slope <= 448 < 2 * M * slope
        for par, s in ((p, slope), (quantize.device_params("f8", d, slope=2.0), F(2))):
            q8, _ = full.quantized("f8", params=par, copy_graph=False)
            assert q8.dtype == float8_e4m3 and q8.metric == full.metric
            np.testing.assert_array_equal(q8.points().view(np.uint8), quantize.f8_translate(X, s).view(np.uint8))
            q8.close()
            for nf in ((False, True) if metric == "mips" else (False,)):
                want = quantize.f8_translate(quantize.normalize_rows(Q) if nf else Q, s).view(np.uint8)
                assert not (want & 0x7F == 0x7F).any() and (not nf and s == 2) <= (want[3, :5].tolist() == [0x7E, 0x7E, 0xFE, 0x7E, 0x80])
                np.testing.assert_array_equal(quantize.device_quantize_rows(Q, par, normalize_first=nf).view(np.uint8), want)
                np.testing.assert_array_equal(_device_rows_dev(par, Q, nf), want)      # the fused call's query bytes: test 4
    finally:
        full.close()


@pytest.mark.parametrize("d", [33, 128, 200])
@pytest.mark.parametrize("metric,m", METRICS)
@pytest.mark.parametrize("exact", [False, True], ids=["grid", "real-exact-order"])
def test_distance_parity(oracle, d, metric, m, exact):
    X, Q = (_real if exact else _grid)(96, d, 3), (_real if exact else _grid)(8, d, 4)
    ix = DeviceIndex(X, max_degree=4, metric=metric, exact_float_order=exact)
    ids = np.arange(96, dtype=U32)
    qd, pd = ix.query_distances(Q, ids), ix.pair_distances(ids, ids[::-1])
    ix.close()
    if exact:
        Xw, Qw = from_f8(X), from_f8(Q)
        exp = np.array([[oracle.distance(q, x, m) for x in Xw] for q in Qw], F)
        exp_p = np.array([oracle.distance(Xw[i], Xw[95 - i], m) for i in ids], F)
    else:
        exp, exp_p = fc.ref_matrix(from_f8(Q), from_f8(X), m).astype(F), fc.ref_pairs(from_f8(X), from_f8(X[::-1]), m).astype(F)
    assert np.array_equal((qd + F(0)).view(U32), (exp + F(0)).view(U32)) and np.array_equal((pd + F(0)).view(U32), (exp_p + F(0)).view(U32))


@functools.lru_cache(None)
def _table(metric, d, real=False):
    """points, queries, the oracle's Vamana graph over the widened rows and the FP8 handle; made once, never changed"""
    X, Q = (_real if real else _grid)(N, d, 1), (_real if real else _grid)(NQ, d, 2)
    G, _ = oracle_api.load().vamana_build(from_f8(X), R, L, 1.2 if metric == "Euclidian" else 1.0, num_passes=1, seed=5, metric=dict(METRICS)[metric])
    return X, Q, G, DeviceIndex(X, G, metric=metric, exact_float_order=real)


# the last case: real data in exact-float-order mode (beam 64 then runs on the generic kernel)
@pytest.mark.parametrize("case", CASES + [dict(beam=32), dict(beam=128), dict(beam=64, real=True)], ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
@pytest.mark.parametrize("d", [33, 128, 200])
@pytest.mark.parametrize("metric,m", METRICS)
def test_search_parity(oracle, metric, m, d, case):
    X, Q, G, ix = _table(metric, d, case.get("real", False))
    kw = dict(dict(k=10, cut=1.35, visited_cap=2048), **{k: v for k, v in case.items() if k != "real"})
    kw["out_k"] = kw["beam"]
    _same_search(oracle.batch_search(from_f8(X), G, queries=from_f8(Q), metric=m, **kw), ix.batch_search(Q, **kw), 1.0)
    qids = np.arange(0, N, N // NQ, dtype=U32)[:NQ]
    _same_search(oracle.batch_search(from_f8(X), G, query_ids=qids, metric=m, **kw), ix.batch_search(query_ids=qids, **kw), 1.0)


@pytest.mark.parametrize("labeled", [False, True], ids=["masked", "labeled"])
@pytest.mark.parametrize("beam", [64, 100])
def test_masked_search_parity(labeled, beam):
    X, Q, G, ix = _table("Euclidian", 128)
    labels = U32(1) << (np.arange(N, dtype=U32) * U32(2654435761) >> U32(7)) % U32(5)
    allow = label_allow(labels, "any", (0b110, 0)) if labeled else np.random.default_rng(9).random(N) < 0.3
    kw = dict(k=10, beam=beam, cut=1.35, out_k=10, visited_cap=2048)
    ref = masked_ref.masked_batch_search(from_f8(X), G, allow, queries=from_f8(Q), **kw)
    if labeled:
        ix.set_labels(labels)
    got = ix.batch_search_labeled(Q, where=("any", (0b110, 0)), **kw) if labeled else ix.batch_search_masked(Q, allow=allow, **kw)
    for f in ("ids", "dists", "result_count", "allowed_cmps", "visited_count", "dist_cmps", "frontier_size"):
        np.testing.assert_array_equal(ref[f], got[f], err_msg=f)


def _float_index(mips, d):
    """real-valued float rows and queries, the float handle (mips: normalised) with its Vamana graph"""
    X, Q = (datasets.t2i_like(N, d, seed=1), datasets.t2i_like(NQ, d, seed=2)) if mips else ((datasets.deep_like(n, d, seed=s) * 2.0).astype(F) for n, s in ((N, 1), (NQ, 2)))
    full = DeviceIndex(X, max_degree=R, metric="mips" if mips else "Euclidian")
    if mips:
        full.normalize()
    full.vamana_build(R, L, 1.2, num_passes=1, seed=5)
    return SimpleNamespace(mips=mips, X=X, Q=Q, full=full, full_q=quantize.normalize_rows(Q) if mips else Q)


@pytest.fixture(scope="module", params=[(False, 33), (False, 128), (True, 33), (True, 128)], ids=lambda p: f"{'mips' if p[0] else 'l2'}_{p[1]}")
def fused(request):
    c = _float_index(*request.param)
    c.quant, c.qparams = c.full.quantized("f8")
    yield c
    c.full.close(); c.quant.close()


@pytest.mark.parametrize("beam", [32, 64])
def test_fused_rerank_parity(fused, beam):
    """search_rerank(quant = the FP8 copy) == quantize_rows, batch_search(out_k = beam), rerank(resort), bit for bit"""
    c, k, rf = fused, 10, 100
    qq = quantize.device_quantize_rows(c.Q, c.qparams, normalize_first=c.mips)
    assert qq.dtype == float8_e4m3 and qq.shape == c.Q.shape
    r = c.quant.batch_search(qq, k=k, beam=beam, out_k=beam)
    ids, dists = c.full.rerank(c.full_q, r["ids"], np.minimum(r["frontier_size"], k * rf).astype(U32), k, resort=True)
    got = c.full.search_rerank(c.quant, c.qparams, c.Q, k=k, beam=beam, rerank_factor=rf, normalize_first=c.mips)
    exp = {"ids": ids, "dists": dists, "frontier_size": r["frontier_size"], "visited_count": r["visited_count"], "dist_cmps": r["dist_cmps"]}
    for f, e in exp.items():
        assert got[f].dtype == e.dtype and np.array_equal(got[f].view(U32), e.view(U32)), f
    assert int(got["status"][0]) == 0 and (got["ids"] < N).all()


@pytest.mark.parametrize("metric", ["Euclidian", "mips"])
def test_graph_index_quant_f8(tmp_path, metric):
    mips = metric == "mips"
    c = _float_index(mips, 128)
    io.write_bin(tmp_path / "b.bin", c.X); io.write_graph(tmp_path / "g", c.full.get_graph())
    c.full.close()
    gi = (FloatMipsIndex if mips else FloatEuclidianIndex)(str(tmp_path / "b.bin"), str(tmp_path / "g"), quant_bits="f8")
    try:
        assert gi.q_index.dtype == float8_e4m3 and gi.qparams.kind == _capi.PANN_QUANT_F8
        ids, dists = gi.batch_search(c.Q, 10, 64, True, 1000)
        r = gi.index.search_rerank(gi.q_index, gi.qparams, c.Q, normalize_first=mips, rerank_factor=100, **gi._qp(10, 64, 1000))
        assert np.array_equal(ids, r["ids"]) and np.array_equal(dists.view(U32), r["dists"].view(U32))
    finally:
        gi.index.close(); gi.q_index.close()


def test_refusals():
    lib = _capi.load()
    n, d = 64, 8
    f8 = DeviceIndex(_grid(n, d, 1), max_degree=8)
    full = DeviceIndex(from_f8(_grid(n, d, 1)), max_degree=8)
    h, q, ids, off2, starts = f8.handle, _grid(4, d, 2), np.arange(16, dtype=U32), np.array([0, 16], np.uint64), np.zeros(1, U32)
    qp = _capi.QueryParams(k=4, beam=8, cut=1.35, limit=n, degree_limit=8, rerank_factor=100, pad=1.0)
    o_rows, o_ids, o_d, o_side, o_off, o_cnt = _buf((16, 9), U32), _buf((16, 4), U32), _buf((16, 4), F), _buf(16, np.uint8), _buf(5, np.uint64), _buf(4, U32)
    so = _capi.SearchOut(ids=_vp(o_ids), dists=_vp(o_d), out_k=4)
    ro = _capi.RerankOut(ids=_vp(o_ids), dists=_vp(o_d), frontier_size=_vp(o_cnt))
    sq, allow, pred, grp = np.zeros((4, 8), np.uint8), np.full(2, 0xFFFFFFFF, U32), np.array([[1, 0]], U32), np.zeros(4, U32)
    o_cen = _buf((1, d), F)
    sp, par = sk.make_params("euclid_bit", d), quantize.device_params("f8", d, slope=1.0)
    calls = {
        "pann_vamana_build": lambda: lib.pann_vamana_build(h, 8, 16, 1.2, 1, 1, 1, None),
        "pann_vamana_build_single_batch": lambda: lib.pann_vamana_build_single_batch(h, 8, 16, 1.2, 1, 4, 1, 1, None),
        "pann_hcnng_build": lambda: lib.pann_hcnng_build(h, 2, 16, 3, 1, None),
        "pann_vamana_insert_batch": lambda: lib.pann_vamana_insert_batch(h, _vp(ids), 16, 0, 8, 16, 1.2, None),
        "pann_robust_prune_batch": lambda: lib.pann_robust_prune_batch(h, _vp(ids[:1]), 1, _vp(ids), None, _vp(off2), 1.2, 8, 1, _vp(o_rows), _vp(o_cnt)),
        "pann_vamana_search_prune_dev": lambda: lib.pann_vamana_search_prune_dev(h, _vp(ids), 16, 0, 8, 16, 1.2, _vp(o_rows), None),      # device-pointer
        "pann_vamana_apply_rows_dev": lambda: lib.pann_vamana_apply_rows_dev(h, _vp(ids), 16, _vp(o_rows), 8, 1.2, None),                   # entries: refused
        "pann_hcnng_build_trees_dev": lambda: lib.pann_hcnng_build_trees_dev(h, 0, 1, 2, 16, 3, 1, _vp(o_rows), 6, None),                   # before any
        "pann_hcnng_assemble_dev": lambda: lib.pann_hcnng_assemble_dev(h, _vp(o_rows), 1, 6, 2, 3),                                         # pointer is used
        "pann_vamana_delete_batch": lambda: lib.pann_vamana_delete_batch(h, _vp(ids), 4, 8, 1.2, None),
        "pann_leaf_knn_batch": lambda: lib.pann_leaf_knn_batch(h, _vp(ids), _vp(off2), 1, 4, _vp(o_ids), _vp(o_d)),
        "pann_leaf_knn": lambda: lib.pann_leaf_knn(h, _vp(ids), 16, 4, _vp(o_ids), _vp(o_d)),
        "pann_pivot_split": lambda: lib.pann_pivot_split(h, _vp(ids), _vp(off2), 1, _vp(ids[:1]), _vp(ids[1:2]), _vp(o_side)),
        "pann_bruteforce_knn": lambda: lib.pann_bruteforce_knn(h, _vp(q), 4, d, 4, _vp(o_ids), _vp(o_d)),
        "pann_bruteforce_range": lambda: lib.pann_bruteforce_range(h, _vp(q), 4, d, 10.0, _vp(o_off), None, 0),
        "pann_range_search": lambda: lib.pann_range_search(h, _vp(q), None, 4, d, _vp(starts), 1, 0, 10.0, 4, _vp(o_ids), _vp(o_cnt), None, None),
        "pann_range_query": lambda: lib.pann_range_query(h, _vp(q), None, 4, d, _vp(starts), 1, C.byref(qp), 10.0, 4, _vp(o_ids), _vp(o_cnt), None, None, None, None),
        "pann_rerank": lambda: lib.pann_rerank(h, _vp(q), 4, d, _vp(ids), 4, None, 4, 1, _vp(o_ids), _vp(o_d)),
        "pann_batch_search_filtered": lambda: lib.pann_batch_search_filtered(h, _vp(q), None, 4, d, _vp(sq), 8, _vp(starts), 1, C.byref(qp), C.byref(so), _vp(o_cnt)),
        "pann_batch_search_filtered_dev": lambda: lib.pann_batch_search_filtered_dev(h, _vp(q), None, 4, d, _vp(sq), 8, _vp(starts), 1, C.byref(qp), C.byref(so), _vp(o_cnt), None),
        "pann_index_upload_sketch": lambda: lib.pann_index_upload_sketch(h, C.byref(sp), _vp(sq), 8),
        "pann_batch_search_rerank": lambda: lib.pann_batch_search_rerank(full.handle, h, C.byref(par), _vp(from_f8(q)), 4, 4 * d, 0, 1, _vp(starts), 1, C.byref(qp), C.byref(ro)),
        "pann_index_attach_sketch": lambda: lib.pann_index_attach_sketch(h, full.handle, C.byref(sp)),
        "pann_index_normalize": lambda: lib.pann_index_normalize(h),
        "pann_bruteforce_knn_masked": lambda: lib.pann_bruteforce_knn_masked(h, _vp(q), 4, d, 4, _vp(allow), 0, _vp(o_ids), _vp(o_d), _vp(o_cnt)),
        "pann_bruteforce_knn_labeled": lambda: lib.pann_bruteforce_knn_labeled(h, _vp(q), 4, d, 4, 0, _vp(pred), 1, _vp(o_ids), _vp(o_d), _vp(o_cnt)),
        "pann_bruteforce_knn_labeled_grouped": lambda: lib.pann_bruteforce_knn_labeled_grouped(h, _vp(q), 4, d, 4, 0, _vp(pred), 1, _vp(grp), 0, _vp(o_ids), _vp(o_d), _vp(o_cnt)),
        "pann_bruteforce_knn_masked_grouped": lambda: lib.pann_bruteforce_knn_masked_grouped(h, _vp(q), 4, d, 4, _vp(allow), 1, 2, _vp(grp), 0, _vp(o_ids), _vp(o_d), _vp(o_cnt)),
        "pann_filter_medoids_labeled": lambda: lib.pann_filter_medoids_labeled(h, 0, _vp(pred), 1, 4, 0, 0, _vp(o_ids), _vp(o_d), _vp(o_cnt), _vp(o_cen)),
        "pann_filter_medoids_masked": lambda: lib.pann_filter_medoids_masked(h, _vp(allow), 1, 2, 4, 0, 0, _vp(o_ids), _vp(o_d), _vp(o_cnt), _vp(o_cen)),
    }
    try:
        for name, fn in calls.items():
            assert lib.pann_index_set_option(full.handle, b"no-such-option", 0) == 1      # last error := another text
            rc, msg = fn(), lib.pann_last_error().decode()
            assert rc == _capi.PANN_ERR_UNSUPPORTED and "PANN_F8" in msg and name in msg, (name, rc, msg)
            for o in (o_rows, o_ids, o_d, o_side, o_off, o_cnt, o_cen):
                assert (o.view(np.uint8) == 0xA5).all(), name
        assert (f8.batch_search(q, k=4, beam=8)["frontier_size"] >= 1).all()               # the handle that refused still searches
    finally:
        f8.close(); full.close()
