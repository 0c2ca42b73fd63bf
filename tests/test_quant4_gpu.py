"""Four-bit rows on the device (PANN_U4 / L2, PANN_I4 / MIPS; include/pann.h, DESIGN.md "Four-bit rows").

Parity anchor.  Let V be the unpacked nibble values of a four-bit table, one per byte (uint8 for U4, int8 for I4).  A U4 / L2
search over the packed rows computes sum (a - q)^2 on the same integers as the oracle's uint8 / L2 search over V: every output
is equal.  An I4 / MIPS search computes 256 x the oracle's int8 / MIPS distance over V (distance_4 as written,
mips_point.h:342-354); multiplying every distance by 256 is exact and commutes with every comparison, so ids and counters are
equal and the distances are exactly 256 x the oracle's.  The quantisers are compared byte for byte with the numpy restatements
of parlayann_amd/quantize.py, which tests/test_quant4_cpu.py pins to hand-computed cases."""
import ctypes as C

import numpy as np
import pytest

from parlayann_amd import DeviceIndex, PannError, _capi, datasets, io, quantize
from parlayann_amd import sketch as sk
from parlayann_amd.graph_index import FloatEuclidianIndex, FloatMipsIndex

pytestmark = pytest.mark.gpu

DIMS = [1, 7, 32, 33, 128, 200]        # 33: an odd tail across a 16-byte step; 200: a 100-byte row on the 8-lane layout
F = np.float32
U32 = np.uint32


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- 1. translate parity ----------------------------------------------------------------------------------------------------

def _signed_rows(n, d, seed, scale=1.0):
    """signed, fractional rows; every 5th value a multiple of 1/8 (so that dyadic parameters meet exact rounding ties)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * scale).astype(F)
    t = rng.integers(-40, 41, (n, d)).astype(F) / F(8) * F(scale)
    m = rng.random((n, d)) < 0.2
    x[m] = t[m]
    return x


def _device_rows_dev(params, rows, normalize_first):
    """pann_quantize_rows_dev on device buffers"""
    import torch
    rb = quantize.quant_row_bytes(params.kind, params.dims)
    t_in = torch.from_numpy(rows).cuda()
    t_out = torch.full((len(rows), rb), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _capi.check(_capi.load().pann_quantize_rows_dev(C.byref(params), C.c_void_p(t_in.data_ptr()), len(rows), rows.shape[1] * 4,
                                                    1 if normalize_first else 0, C.c_void_p(t_out.data_ptr()), rb, None))
    torch.cuda.synchronize()
    return t_out.cpu().numpy()


def _check_translate(full, X, Q, params, expect, normalize_first=False):
    """create_quantized's rows and both forms of quantize_rows against expect(rows) -> nibble values"""
    d = X.shape[1]
    q4, p = full.quantized(params.kind, params=params, copy_graph=False)
    try:
        assert q4.dtype4 is not None and q4.row_bytes == (d + 1) // 2
        got = q4.points()
        assert got.dtype == np.uint8 and got.shape == (len(X), (d + 1) // 2)
        np.testing.assert_array_equal(got, quantize.pack_nibbles(expect(X)))
    finally:
        q4.close()
    Qn = quantize.normalize_rows(Q) if normalize_first else Q
    want = quantize.pack_nibbles(expect(Qn))
    np.testing.assert_array_equal(quantize.device_quantize_rows(Q, params, normalize_first=normalize_first).view(np.uint8), want)
    np.testing.assert_array_equal(_device_rows_dev(params, Q, normalize_first), want)


@pytest.mark.parametrize("d", DIMS)
def test_euclid_u4_translate_parity(d):
    X, Q = _signed_rows(257, d, 10 + d), _signed_rows(257, d, 20 + d, scale=1.5)       # queries reach beyond min / max
    full = DeviceIndex(X, max_degree=4)
    try:
        p = full.quantize_params("euclid_u4")
        ref = quantize.euclid_u4_params(X)
        assert p.kind == _capi.PANN_QUANT_EUCLID_U4 and (F(p.slope), int(p.offset), p.dims) == (ref.slope, int(ref.offset), d)
        assert Q.min() < X.min() and Q.max() > X.max()
        _check_translate(full, X, Q, p, lambda r: quantize.euclid_u4_translate(r, ref))
        # dyadic parameters: x * 2 lands on .5 for the multiples of 1/4 that are not multiples of 1/2 -- exact ties
        p2 = quantize.device_params("euclid_u4", d, slope=2.0, offset=-7)
        ref2 = quantize.EuclidParams.__new__(quantize.EuclidParams)
        ref2.range, ref2.dims, ref2.slope, ref2.offset = 15, d, F(2.0), np.int32(-7)
        assert ((np.abs(X * F(2.0)) % 1) == 0.5).any() and (X * F(2.0) > 8).any() and (X * F(2.0) < -7).any()
        _check_translate(full, X, Q, p2, lambda r: quantize.euclid_u4_translate(r, ref2))
    finally:
        full.close()


@pytest.mark.parametrize("trim", [True, False], ids=["trim", "notrim"])
@pytest.mark.parametrize("d", DIMS)
def test_mips_i4_translate_parity(d, trim):
    X, Q = _signed_rows(257, d, 30 + d), _signed_rows(257, d, 40 + d, scale=1.5)
    full = DeviceIndex(X, max_degree=4, metric="mips")
    try:
        p = full.quantize_params("mips_i4", trim=trim)
        mv = quantize.mips_i8_max_val(X, trim=trim)                   # the parameters are exactly those of MIPS_I8
        assert p.kind == _capi.PANN_QUANT_MIPS_I4 and F(p.max_val) == mv and p.dims == d
        assert np.abs(Q).max() > mv
        _check_translate(full, X, Q, p, lambda r: quantize.mips_i4_translate(r, mv))
        _check_translate(full, X, Q, p, lambda r: quantize.mips_i4_translate(r, mv), normalize_first=True)
        # max_val 3.5: scale = 2, ties as above; values beyond +-3.5 are capped at +-7
        p2 = quantize.device_params("mips_i4", d, max_val=3.5)
        assert ((np.abs(X * F(2.0)) % 1) == 0.5).any() and (np.abs(X) > 3.5).any()
        _check_translate(full, X, Q, p2, lambda r: quantize.mips_i4_translate(r, F(3.5)))
    finally:
        full.close()


# ---- 2. distance parity -----------------------------------------------------------------------------------------------------

def _all_pairs_table(d, seed):
    """32 rows of nibbles: row i < 16 is (i + 3 j) mod 16 at coordinate j -- rows a, b meet as (a, b) at coordinate 0, so the 256
    row pairs hold every ordered pair of nibble values, 0x8 included -- and 16 random rows"""
    rng = np.random.default_rng(seed)
    j = np.arange(d)[None, :]
    A = ((np.arange(16)[:, None] + 3 * j) % 16).astype(np.uint8)
    return np.concatenate([A, rng.integers(0, 16, (16, d)).astype(np.uint8)])


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dt", ["u4", "i4"])
def test_distance_parity(d, dt):
    nib = _all_pairs_table(d, 50 + d)
    signed = dt == "i4"
    rows = quantize.pack_nibbles(nib)
    V = quantize.unpack_nibbles(rows, d, signed).astype(np.int64)       # 8..15 are -8..-1 for i4
    assert len({(int(a), int(b)) for a in V[:16, 0] for b in V[:16, 0]}) == 256 and (not signed or V.min() == -8)
    if signed:
        exp = (-256 * (V[:, None, :] * V[None, :, :]).sum(-1)).astype(F)   # exact: multiples of 256 below 2^24 * 256
    else:
        exp = ((V[:, None, :] - V[None, :, :]) ** 2).sum(-1).astype(F)
    ix = DeviceIndex.from_packed(rows, d, dt, max_degree=4)
    try:
        np.testing.assert_array_equal(ix.points(), rows)                   # upload / download move packed rows
        a, b = (g.ravel().astype(U32) for g in np.meshgrid(np.arange(32), np.arange(32), indexing="ij"))
        assert np.array_equal(ix.pair_distances(a, b), exp[a, b])
        assert np.array_equal(ix.query_distances(rows, np.arange(32, dtype=U32)), exp)
    finally:
        ix.close()


# ---- 3. search parity -------------------------------------------------------------------------------------------------------

N, NQ, R, L = 2000, 64, 16, 32
_tables = {}


def _table(dt, d):
    """nibble values V of N clustered points and NQ queries (quantised by the numpy restatement), the graph the device Vamana
    builds on the one-byte handle of V, and the four-bit handle with that graph; built once per (type, d), never changed"""
    if (dt, d) not in _tables:
        if dt == "u4":
            X, Q = datasets.deep_like(N, d, seed=1), datasets.deep_like(NQ, d, seed=2)
            p = quantize.euclid_u4_params(X)
            V, Vq, metric = quantize.euclid_u4_translate(X, p), quantize.euclid_u4_translate(Q, p), "Euclidian"
        else:
            X, Q = quantize.normalize_rows(datasets.t2i_like(N, d, seed=1)), quantize.normalize_rows(datasets.t2i_like(NQ, d, seed=2))
            mv = quantize.mips_i8_max_val(X, trim=True)
            V, Vq, metric = quantize.mips_i4_translate(X, mv), quantize.mips_i4_translate(Q, mv), "mips"
        one = DeviceIndex(V, max_degree=R, metric=metric)
        one.vamana_build(R, L, 1.2 if dt == "u4" else 1.0, num_passes=1, seed=5)
        G = one.get_graph()
        one.close()
        ix4 = DeviceIndex.from_packed(quantize.pack_nibbles(V), d, dt, max_degree=R)
        ix4.set_graph(G)
        _tables[(dt, d)] = (V, Vq, G, ix4, "l2" if dt == "u4" else "mips")
    return _tables[(dt, d)]


@pytest.fixture(scope="module", autouse=True)
def _close_tables():
    yield
    for t in _tables.values():
        t[3].close()
    _tables.clear()


def _same_dists(exp, got):
    """equal as float VALUES, every one of them (no tolerance; +inf pads included).  Not compared as bit patterns: a dot product
    of zero is -0.0 in the oracle (-(float) 0) and +0.0 on the device, whose (dist, id) sort key folds the two zeros into one
    (f2ord, pann_device.h) for every element type -- the sign of a zero takes part in no comparison and is not a result."""
    assert got.dtype == F and exp.dtype == F and not np.isnan(got).any()
    np.testing.assert_array_equal(exp, got)


def _same_search(o, g, scale):
    for f in ("frontier_size", "visited_count", "dist_cmps", "degree_sum"):
        np.testing.assert_array_equal(o[f], g[f], err_msg=f)
    np.testing.assert_array_equal(o["ids"], g["ids"])
    _same_dists(o["dists"] * F(scale), g["dists"])
    for i in range(len(o["ids"])):
        nv = o["visited_count"][i]
        order = np.lexsort((g["visited_ids"][i, :nv], g["visited_dists"][i, :nv]))      # sorted (dist, id) rows, as test_search_gpu
        np.testing.assert_array_equal(o["visited_ids"][i, :nv], g["visited_ids"][i, :nv][order])
        _same_dists(o["visited_dists"][i, :nv] * F(scale), g["visited_dists"][i, :nv][order])


# beam 1 / 10: generic, 64: frontier in registers, 100: two entries per lane, 200: generic again; k = 10 except where the beam is
# smaller (k > beam is refused, beamSearch.h:368-372)
CASES = [dict(beam=1, k=1), dict(beam=10), dict(beam=64), dict(beam=100), dict(beam=200),
         dict(beam=64, limit=20), dict(beam=64, degree_limit=8)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
@pytest.mark.parametrize("d", [33, 128, 200])
@pytest.mark.parametrize("dt", ["u4", "i4"])
def test_search_parity(oracle, dt, d, case):
    V, Vq, G, ix4, metric = _table(dt, d)
    kw = dict(k=10, cut=1.35, visited_cap=2048)          # >= N: a visited list always fits
    kw.update(case)
    kw["out_k"] = kw["beam"]
    scale = 256.0 if dt == "i4" else 1.0
    Pq = quantize.pack_nibbles(Vq)
    o = oracle.batch_search(V, G, queries=Vq, metric=metric, **kw)
    _same_search(o, ix4.batch_search(Pq, **kw), scale)
    qids = np.arange(0, N, N // NQ, dtype=U32)[:NQ]
    o = oracle.batch_search(V, G, query_ids=qids, metric=metric, **kw)
    _same_search(o, ix4.batch_search(query_ids=qids, **kw), scale)


def test_copied_graph_searches_like_a_set_graph():
    """a four-bit handle gets its graph from pann_index_set_graph or from create_quantized(copy_graph): both search the same"""
    V, Vq, G, ix4, metric = _table("u4", 128)
    full = DeviceIndex(V.astype(F), G)
    try:
        p = quantize.device_params("euclid_u4", 128, slope=1.0, offset=0)        # V's values are their own translation
        q4, _ = full.quantized("euclid_u4", params=p, copy_graph=True)
        try:
            np.testing.assert_array_equal(q4.points(), quantize.pack_nibbles(V))
            np.testing.assert_array_equal(q4.get_graph(), ix4.get_graph())
            a = q4.batch_search(quantize.pack_nibbles(Vq), k=10, beam=100, out_k=100)
            b = ix4.batch_search(quantize.pack_nibbles(Vq), k=10, beam=100, out_k=100)
            for f in ("ids", "dists", "visited_count", "dist_cmps"):
                np.testing.assert_array_equal(a[f], b[f])
        finally:
            q4.close()
    finally:
        full.close()


# ---- 4. fused rerank parity -------------------------------------------------------------------------------------------------

class Fused:
    def __init__(self, mips, d):
        self.mips = mips
        if mips:
            self.X, self.Q = datasets.t2i_like(N, d, seed=1), datasets.t2i_like(NQ, d, seed=2)
        else:
            self.X = (datasets.deep_like(N, d, seed=1) * 2.0).astype(F)
            self.Q = (datasets.deep_like(NQ, d, seed=2) * 2.0).astype(F)
        self.full = DeviceIndex(self.X, max_degree=R, metric="mips" if mips else "Euclidian")
        if mips:
            self.full.normalize()
        self.full.vamana_build(R, L, 1.2, num_passes=1, seed=5)
        self.quant, self.qparams = self.full.quantized("mips_i4" if mips else "euclid_u4")
        self.full_q = quantize.normalize_rows(self.Q) if mips else self.Q

    def close(self):
        self.full.close(); self.quant.close()


@pytest.fixture(scope="module", params=[(False, 33), (False, 128), (True, 33), (True, 128)], ids=lambda p: f"{'mips' if p[0] else 'l2'}_{p[1]}")
def fused(request):
    c = Fused(*request.param)
    yield c
    c.close()


@pytest.mark.parametrize("beam", [32, 64])
def test_fused_rerank_parity(fused, beam):
    import torch
    c, k, rf = fused, 10, 100
    qq = quantize.device_quantize_rows(c.Q, c.qparams, normalize_first=c.mips)
    assert qq.shape == (NQ, (c.X.shape[1] + 1) // 2)
    r = c.quant.batch_search(qq, k=k, beam=beam, out_k=beam)
    counts = np.minimum(r["frontier_size"], k * rf).astype(U32)
    ids, dists = c.full.rerank(c.full_q, r["ids"], counts, k, resort=True)
    got = c.full.search_rerank(c.quant, c.qparams, c.Q, k=k, beam=beam, rerank_factor=rf, normalize_first=c.mips)
    exp = {"ids": ids, "dists": dists, "frontier_size": r["frontier_size"], "visited_count": r["visited_count"], "dist_cmps": r["dist_cmps"]}
    for f, e in exp.items():
        assert got[f].dtype == e.dtype and np.array_equal(got[f].view(U32), e.view(U32)), f
    assert int(got["status"][0]) == 0 and (got["ids"] < N).all()
    # the returned distances are the float handle's own distances to the returned ids
    for i in range(0, NQ, 7):
        exact = c.full.query_distances(c.full_q[i:i + 1], got["ids"][i])
        assert np.array_equal(exact[0].view(U32), got["dists"][i].view(U32))
    # the _dev form, on a caller's stream
    t_q = torch.from_numpy(c.Q).cuda()
    t_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    t_ids = torch.zeros((NQ, k), dtype=torch.int32, device="cuda")
    t_d = torch.zeros((NQ, k), dtype=torch.float32, device="cuda")
    t_cnt = [torch.zeros(NQ, dtype=torch.int32, device="cuda") for _ in range(3)]
    t_status = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    c.full.search_rerank_dev(c.quant, c.qparams, t_q.data_ptr(), NQ, 4 * c.X.shape[1], t_st.data_ptr(), 1, t_ids.data_ptr(), t_d.data_ptr(),
                             k=k, beam=beam, normalize_first=c.mips, d_frontier_size_ptr=t_cnt[0].data_ptr(),
                             d_visited_count_ptr=t_cnt[1].data_ptr(), d_dist_cmps_ptr=t_cnt[2].data_ptr(),
                             d_status_ptr=t_status.data_ptr(), stream_ptr=stream.cuda_stream)
    stream.synchronize()
    dev = {"ids": t_ids, "dists": t_d, "frontier_size": t_cnt[0], "visited_count": t_cnt[1], "dist_cmps": t_cnt[2]}
    for f, t in dev.items():
        assert np.array_equal(t.cpu().numpy().view(U32), exp[f].view(U32)), f
    assert int(t_status.cpu()[0]) == 0


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------

SENT = 0xA5


def _buf(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = SENT
    return a


def test_refusals(oracle):
    lib = _capi.load()
    n, d = 64, 8
    rng = np.random.default_rng(7)
    rows = quantize.pack_nibbles(rng.integers(0, 16, (n, d)).astype(np.uint8))
    Xf = rng.standard_normal((n, d)).astype(F)
    u4 = DeviceIndex.from_packed(rows, d, "u4", max_degree=8)
    i4 = DeviceIndex.from_packed(rows, d, "i4", max_degree=8)
    full = DeviceIndex(Xf, max_degree=8)
    full_m = DeviceIndex(Xf, max_degree=8, metric="mips")
    q = rows[:4].copy()
    ids = np.arange(16, dtype=U32)
    off2 = np.array([0, 16], np.uint64)
    starts = np.zeros(1, U32)
    qp = _capi.QueryParams(k=4, beam=8, cut=1.35, limit=n, degree_limit=8, rerank_factor=100, pad=1.0)
    sp = sk.make_params("euclid_bit", d)
    sq = np.zeros((4, 8), np.uint8)
    p_u4 = quantize.device_params("euclid_u4", d, slope=1.0, offset=0)
    p_i4 = quantize.device_params("mips_i4", d, max_val=1.0)
    p_u8 = quantize.device_params("euclid_u8", d, slope=2.0, offset=0)
    Qf = Xf[:4].copy()

    def refused(name, fn, outs, code=_capi.PANN_ERR_UNSUPPORTED, text=None):
        assert lib.pann_index_set_option(full.handle, b"no-such-option", 0) == 1          # last error := another text
        rc = fn()
        msg = lib.pann_last_error().decode()
        assert rc == code and msg and "no-such-option" not in msg, (name, rc, msg)
        if text:
            assert text in msg, (name, msg)
        for o in outs:
            assert (o.view(np.uint8) == SENT).all(), name

    try:
        for h, tname in ((u4.handle, "PANN_U4"), (i4.handle, "PANN_I4")):
            def un(name, fn, outs=()):
                refused(name, fn, outs, text=tname)
                assert name in lib.pann_last_error().decode(), name                         # the message names the entry point
            o_rows, o_dc = _buf((16, 9), U32), _buf(16, U32)
            o_ids, o_d = _buf((16, 4), U32), _buf((16, 4), F)
            o_side, o_off, o_cnt = _buf(16, np.uint8), _buf(5, np.uint64), _buf(4, U32)
            s_out = {f: _buf((4, 8), U32) for f in ("ids", "dists")}
            so = _capi.SearchOut(ids=_vp(s_out["ids"]), dists=_vp(s_out["dists"]), out_k=8)
            o_pr = _buf(4, U32)
            ro = _capi.RerankOut(ids=_vp(o_ids), dists=_vp(o_d), frontier_size=_vp(o_cnt))
            qout = _capi.QuantParams()
            un("pann_vamana_build", lambda: lib.pann_vamana_build(h, 8, 16, 1.2, 1, 1, 1, None))
            un("pann_vamana_build_single_batch", lambda: lib.pann_vamana_build_single_batch(h, 8, 16, 1.2, 1, 4, 1, 1, None))
            un("pann_hcnng_build", lambda: lib.pann_hcnng_build(h, 2, 16, 3, 1, None))
            un("pann_vamana_insert_batch", lambda: lib.pann_vamana_insert_batch(h, _vp(ids), 16, 0, 8, 16, 1.2, None))
            # the two-phase build seams take device pointers; a four-bit handle is refused before any pointer is used
            un("pann_vamana_search_prune_dev", lambda: lib.pann_vamana_search_prune_dev(h, _vp(ids), 16, 0, 8, 16, 1.2, _vp(o_rows), None), (o_rows,))
            un("pann_vamana_apply_rows_dev", lambda: lib.pann_vamana_apply_rows_dev(h, _vp(ids), 16, _vp(o_rows), 8, 1.2, None), (o_rows,))
            un("pann_hcnng_build_trees_dev", lambda: lib.pann_hcnng_build_trees_dev(h, 0, 1, 2, 16, 3, 1, _vp(o_rows), 6, None), (o_rows,))
            un("pann_hcnng_assemble_dev", lambda: lib.pann_hcnng_assemble_dev(h, _vp(o_rows), 1, 6, 2, 3), (o_rows,))
            un("pann_robust_prune_batch", lambda: lib.pann_robust_prune_batch(h, _vp(ids[:1]), 1, _vp(ids), None, _vp(off2), 1.2, 8, 1,
                                                                               _vp(o_rows), _vp(o_dc)), (o_rows, o_dc))
            un("pann_leaf_knn", lambda: lib.pann_leaf_knn(h, _vp(ids), 16, 4, _vp(o_ids), _vp(o_d)), (o_ids, o_d))
            un("pann_leaf_knn_batch", lambda: lib.pann_leaf_knn_batch(h, _vp(ids), _vp(off2), 1, 4, _vp(o_ids), _vp(o_d)), (o_ids, o_d))
            un("pann_pivot_split", lambda: lib.pann_pivot_split(h, _vp(ids), _vp(off2), 1, _vp(ids[:1]), _vp(ids[1:2]), _vp(o_side)), (o_side,))
            un("pann_bruteforce_knn", lambda: lib.pann_bruteforce_knn(h, _vp(q), 4, 4, 4, _vp(o_ids), _vp(o_d)), (o_ids, o_d))
            un("pann_bruteforce_range", lambda: lib.pann_bruteforce_range(h, _vp(q), 4, 4, 10.0, _vp(o_off), None, 0), (o_off,))
            un("pann_range_search", lambda: lib.pann_range_search(h, _vp(q), None, 4, 4, _vp(starts), 1, 0, 10.0, 4, _vp(o_ids), _vp(o_cnt),
                                                                   None, None), (o_ids, o_cnt))
            un("pann_range_query", lambda: lib.pann_range_query(h, _vp(q), None, 4, 4, _vp(starts), 1, C.byref(qp), 10.0, 4, _vp(o_ids),
                                                                 _vp(o_cnt), None, None, None, None), (o_ids, o_cnt))
            un("pann_rerank", lambda: lib.pann_rerank(h, _vp(q), 4, 4, _vp(ids), 4, None, 4, 1, _vp(o_ids), _vp(o_d)), (o_ids, o_d))
            un("pann_batch_search_filtered", lambda: lib.pann_batch_search_filtered(h, _vp(q), None, 4, 4, _vp(sq), 8, _vp(starts), 1, C.byref(qp),
                                                                                    C.byref(so), _vp(o_pr)), (s_out["ids"], s_out["dists"], o_pr))
            un("pann_batch_search_filtered_dev", lambda: lib.pann_batch_search_filtered_dev(h, _vp(q), None, 4, 4, _vp(sq), 8, _vp(starts), 1,
                                                                                            C.byref(qp), C.byref(so), _vp(o_pr), None),
               (s_out["ids"], s_out["dists"], o_pr))             # refused before any pointer is used
            src = full if tname == "PANN_U4" else full_m
            par = p_u4 if tname == "PANN_U4" else p_i4
            un("pann_batch_search_rerank", lambda: lib.pann_batch_search_rerank(src.handle, h, C.byref(par), _vp(Qf), 4, 4 * d, 0, 1, _vp(starts), 1,
                                                                                C.byref(qp), C.byref(ro)), (o_ids, o_d, o_cnt))
            un("pann_index_attach_sketch", lambda: lib.pann_index_attach_sketch(h, full.handle, C.byref(sp)))
            assert lib.pann_index_sketch_kind(h) == -1
            un("pann_index_normalize", lambda: lib.pann_index_normalize(h))
            before = qout.kind, qout.dims, qout.slope, qout.max_val
            refused("pann_quantize_params", lambda: lib.pann_quantize_params(h, _capi.PANN_QUANT_EUCLID_U4, 0, C.byref(qout)), (),
                    text="pann_quantize_params")                 # a source that is not f32: as before
            assert (qout.kind, qout.dims, qout.slope, qout.max_val) == before
            # a kind that does not match quant's element type
            for bad in (p_u8, p_i4 if tname == "PANN_U4" else p_u4):
                refused("kind mismatch", lambda: lib.pann_batch_search_rerank(src.handle, h, C.byref(bad), _vp(Qf), 4, 4 * d, 0, 0, _vp(starts), 1,
                                                                               C.byref(qp), C.byref(ro)),
                        (o_ids, o_d, o_cnt), code=_capi.PANN_ERR_BAD_ARG)
        # pairings refused at creation
        for code, metric in ((_capi.PANN_U4, _capi.PANN_MIPS), (_capi.PANN_I4, _capi.PANN_L2)):
            hnew = C.c_void_p()
            refused("pann_index_create", lambda: lib.pann_index_create(C.byref(hnew), _vp(rows), n, d, code, 4, metric, None, 8, 0), (),
                    text="pann_index_create")
            assert not hnew.value
            refused("pann_index_create_empty", lambda: lib.pann_index_create_empty(C.byref(hnew), n, d, code, metric, 8, 0), ())
            assert not hnew.value
        with pytest.raises(PannError):
            DeviceIndex.from_packed(rows, d, "u4", max_degree=8, metric="mips")
        # the handles that refused still search, and so does an ordinary u8 handle in the same process
        r = u4.batch_search(q, k=4, beam=8)
        assert (r["frontier_size"] >= 1).all()
        X = datasets.sift_like(1000, 32, seed=3)
        Q = datasets.sift_like(20, 32, seed=4)
        ix = DeviceIndex(X, max_degree=16)
        try:
            ix.vamana_build(16, 32, 1.2, num_passes=1, seed=5)
            g = ix.batch_search(Q, k=10, beam=64)
            o = oracle.batch_search(X, ix.get_graph(), queries=Q, k=10, beam=64)
            for f in ("ids", "dists", "visited_count", "dist_cmps"):
                np.testing.assert_array_equal(g[f], o[f])
        finally:
            ix.close()
    finally:
        for x in (u4, i4, full, full_m):
            x.close()


# ---- 6. GraphIndex(quant_bits=4) --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["Euclidian", "mips"])
def test_graph_index_quant_bits(tmp_path, metric):
    d = 128
    mips = metric == "mips"
    X = datasets.t2i_like(N, d, seed=1) if mips else (datasets.deep_like(N, d, seed=1) * 2.0).astype(F)
    Q = datasets.t2i_like(NQ, d, seed=2) if mips else (datasets.deep_like(NQ, d, seed=2) * 2.0).astype(F)
    b = DeviceIndex(X, max_degree=R, metric=metric)
    if mips:
        b.normalize()
    b.vamana_build(R, L, 1.2, num_passes=1, seed=5)
    io.write_bin(tmp_path / "b.bin", X)
    io.write_graph(tmp_path / "g", b.get_graph())
    b.close()
    cls = FloatMipsIndex if mips else FloatEuclidianIndex
    i4 = cls(str(tmp_path / "b.bin"), str(tmp_path / "g"), quant_bits=4)
    i8 = cls(str(tmp_path / "b.bin"), str(tmp_path / "g"), quant_bits=8)
    i0 = cls(str(tmp_path / "b.bin"), str(tmp_path / "g"))
    try:
        assert i4.q_index.dtype4 == (_capi.PANN_I4 if mips else _capi.PANN_U4)
        assert i4.qparams.kind == (_capi.PANN_QUANT_MIPS_I4 if mips else _capi.PANN_QUANT_EUCLID_U4)
        ids, dists = i4.batch_search(Q, 10, 64, True, 1000)
        r = i4.index.search_rerank(i4.q_index, i4.qparams, Q, normalize_first=mips, use_filter=False, rerank_factor=100,
                                   **i4._qp(10, 64, 1000))
        assert np.array_equal(ids, r["ids"]) and np.array_equal(dists.view(U32), r["dists"].view(U32))
        a_ids, a_d = i8.batch_search(Q, 10, 64, True, 1000)
        b_ids, b_d = i0.batch_search(Q, 10, 64, True, 1000)
        assert i8.q_index.dtype4 is None and i8.qparams.kind == i0.qparams.kind
        assert np.array_equal(a_ids, b_ids) and np.array_equal(a_d.view(U32), b_d.view(U32))
    finally:
        for i in (i4, i8, i0):
            i.index.close(); i.q_index.close()
