"""pann_batch_search_masked_rerank / _dev (csrc/search_rerank.hip, DESIGN.md "Masked search on the fused path"): the masked
search of the quantised copy with an exact rerank of its result list, as ONE call that never leaves the device, against the
composition of entry points that their own tests already pin:

    pann_quantize_rows  ->  pann_batch_search_masked on the quantised handle, out_k = pool = min(k * rerank_factor, beam, 64)
    ->  pann_rerank on the float handle with counts = result_count, resort = 1

The fused call must equal the composition bit for bit in ids, dists, result_count, allowed_cmps, frontier_size, visited_count
and dist_cmps; its traversal counters must be the plain fused call's; in exact-float-order mode it must equal the CPU
restatement of tests/masked_rerank_cases.py (whose regimes tests/test_masked_rerank_cases_cpu.py asserts)."""
import ctypes as C

import numpy as np
import pytest

import masked_rerank_cases as rc
from parlayann_amd import DeviceIndex, PannError, _capi, allow_bitmap, io, quantize
from parlayann_amd.graph_index import FloatEuclidianIndex, FloatMipsIndex

pytestmark = pytest.mark.gpu

N, NQ, R = rc.N, rc.NQ, rc.R
SENT = rc.SENT
FIELDS = ("ids", "dists", "result_count", "allowed_cmps", "frontier_size", "visited_count", "dist_cmps")
TRAVERSAL = ("frontier_size", "visited_count", "dist_cmps")


class Case:
    """a float index with its graph (the oracle's for the restated datasets, built on the device otherwise), its quantised copy
    and the queries"""

    def __init__(self, name):
        d, metric, bits = rc.DATASETS[name]
        self.name, self.mips = name, metric == "mips"
        self.X, self.Q = rc.data(name)
        if name in rc.RESTATED:
            self.full = DeviceIndex(self.X, rc.graph(name))
        else:
            self.full = DeviceIndex(self.X, max_degree=R, metric="mips" if self.mips else "Euclidian")
            if self.mips:
                self.full.normalize()                                # graph_index.cpp:94-95
            self.full.vamana_build(R, rc.L, 1.2, num_passes=1, seed=5)
        kind = ("mips_i" if self.mips else "euclid_u") + str(bits)
        self.quant, self.qparams = self.full.quantized(kind)
        assert self.mips or bits == 4 or not self.qparams.identity   # real-valued data: the u8 quantiser is not a cast
        self.full_q = quantize.normalize_rows(self.Q) if self.mips else self.Q

    def compose(self, k, beam, rf, allow, **qp):
        """the three existing calls, one after the other.  pann_rerank pads a row with counts < k as the rule does (0xFFFFFFFF /
        +inf behind the counts entries); the rows are padded here on the host all the same, so that the expectation states the
        rule and not what pann_rerank happens to do"""
        pool = rc.pool(beam, k, rf)
        qq = quantize.device_quantize_rows(self.Q, self.qparams, normalize_first=self.mips)
        r = self.quant.batch_search_masked(qq, allow=allow, k=k, beam=beam, out_k=pool, **qp)
        ids, dists = self.full.rerank(self.full_q, r["ids"], r["result_count"], k, resort=True)
        pad = np.arange(k)[None, :] >= r["result_count"][:, None]
        ids[pad] = SENT; dists[pad] = np.inf
        exp = {"ids": ids, "dists": dists, "list_ids": r["ids"], "list_dists": r["dists"]}
        for f in FIELDS[2:]:
            exp[f] = r[f]
        return exp

    def fused(self, k, beam, rf, allow=None, **qp):
        return self.full.search_rerank(self.quant, self.qparams, self.Q, k=k, beam=beam, rerank_factor=rf,
                                       normalize_first=self.mips, allow=allow, **qp)

    def set_exact(self, on):
        _capi.check(self.full._lib.pann_index_set_exact_float_order(self.full.handle, 1 if on else 0))

    def close(self):
        self.full.close(); self.quant.close()


@pytest.fixture(scope="module")
def cases():
    """the datasets of this module, each built on first use and shared; closed at the end"""
    built = {}

    def get(name):
        if name not in built:
            built[name] = Case(name)
        return built[name]
    yield get
    for c in built.values():
        c.close()


@pytest.fixture
def case(request, cases):
    c = cases(request.param)
    yield c
    c.set_exact(False)


def _same(got, exp, fields=FIELDS, msg=""):
    for f in fields:
        assert got[f].dtype == exp[f].dtype and np.array_equal(got[f].view(np.uint32), exp[f].view(np.uint32)), (msg, f)


def _padded(got, k):
    """the padding rule: min(k, result_count) entries, then 0xFFFFFFFF / +inf"""
    pad = np.arange(k)[None, :] >= got["result_count"][:, None]
    assert (got["ids"][pad] == SENT).all() and np.isposinf(got["dists"][pad]).all()
    assert (got["ids"][~pad] < N).all() and np.isfinite(got["dists"][~pad]).all()


# ---- 1. fused == composition ----
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact_order"])
@pytest.mark.parametrize("beam,k,rf", rc.SWEEP)
@pytest.mark.parametrize("case", list(rc.DATASETS), indirect=True)
def test_fused_equals_the_composition(case, beam, k, rf, exact):
    case.set_exact(exact)
    pool = rc.pool(beam, k, rf)
    for mkind in rc.MASK_KINDS:
        m = rc.mask(mkind, case.name)
        packed = rc.pack(m)
        exp, got = case.compose(k, beam, rf, packed), case.fused(k, beam, rf, packed)
        _same(got, exp, msg=mkind)
        assert int(got["status"][0]) == 0, mkind                     # a short row raises no SHORT_FRONTIER
        assert (got["result_count"] <= pool).all()
        _padded(got, k)
        allowed = np.broadcast_to(m, (NQ, N))
        real = got["ids"] != SENT
        assert allowed[np.nonzero(real)[0], got["ids"][real]].all(), mkind
        if mkind == "ones":
            assert (got["result_count"] == pool).all()               # the list is full: the rerank reads `pool` candidates
        if mkind == "zeros":
            assert (got["result_count"] == 0).all() and (got["allowed_cmps"] == 0).all()
        if mkind == "start_off":
            assert not (got["ids"] == 0).any()
    if (beam, k, rf) == (64, 2, 3):
        assert pool == 6
    if beam == 16:               # the walk stopped early: the 5 % mask leaves lists shorter than k (masked_rerank_cases.SHORT_LIMIT)
        packed = rc.pack(rc.mask("rand5", case.name))
        exp, got = case.compose(k, beam, rf, packed, limit=rc.SHORT_LIMIT), case.fused(k, beam, rf, packed, limit=rc.SHORT_LIMIT)
        _same(got, exp, msg="rand5 short")
        _padded(got, k)
        assert int(got["status"][0]) == 0
        assert (got["result_count"] < k).any()


# ---- 2. the traversal is the plain fused call's ----
@pytest.mark.parametrize("beam", [16, 64, 100])
@pytest.mark.parametrize("case", list(rc.DATASETS), indirect=True)
def test_traversal_is_the_plain_fused_calls(case, beam):
    k, rf = 10, 100
    plain = case.fused(k, beam, rf)
    assert "result_count" not in plain
    for mkind in rc.MASK_KINDS:
        got = case.fused(k, beam, rf, rc.pack(rc.mask(mkind, case.name)))
        _same(got, plain, TRAVERSAL, msg=mkind)
    if beam <= 64:
        # all ones and pool = beam: nothing is cut from the list, which holds the best `beam` points the walk compared -- the
        # frontier is a subset of those, so rank for rank the masked result is at least as near
        got = case.fused(k, beam, rf, rc.pack(rc.mask("ones", case.name)))
        assert (plain["frontier_size"] >= k).all() and (got["dists"] <= plain["dists"]).all()


# ---- 3. exact-order mode == the oracle-based restatement ----
@pytest.mark.parametrize("beam,k,rf,mkind,qp", [(16, 10, 100, "rand5", dict(limit=rc.SHORT_LIMIT)), (16, 10, 100, "rand5", {}),
                                                (64, 10, 100, "rand50", {}), (64, 2, 3, "rand50", {}), (64, 10, 100, "far_only", {}),
                                                (64, 10, 100, "zeros", {}), (100, 10, 100, "rows_differ", {})])
@pytest.mark.parametrize("case", rc.RESTATED, indirect=True)
def test_exact_order_equals_the_restatement(case, oracle, beam, k, rf, mkind, qp):
    case.set_exact(True)
    slope, offset, _, _ = rc.quantised(case.name)
    assert (np.float32(case.qparams.slope), int(case.qparams.offset)) == (slope, offset)
    ref = rc.restate(case.name, beam, k, rf, mkind, **qp)
    got = case.fused(k, beam, rf, rc.pack(rc.mask(mkind, case.name)), **qp)
    np.testing.assert_array_equal(got["ids"], ref["rr_ids"])
    assert np.array_equal(got["dists"].view(np.uint32), ref["rr_dists"].view(np.uint32))
    for f in ("result_count", "allowed_cmps") + TRAVERSAL:
        np.testing.assert_array_equal(got[f], ref[f], err_msg=f)


# ---- 4. host entry == _dev entry on a caller's stream, per-query bitmaps resident on the device ----
@pytest.mark.parametrize("case", ["l2_64", "l2_96", "mips_100_i4"], indirect=True)
def test_dev_entry_on_a_callers_stream(case):
    import torch
    k, beam, d = 10, 64, case.X.shape[1]
    packed = rc.pack(rc.mask("rows_differ", case.name))
    assert packed.shape == (NQ, rc.WORDS)
    host = case.fused(k, beam, 100, packed)
    stride_w = rc.WORDS + 3                                          # bitmap rows further apart than a row is long
    wide = np.full((NQ, stride_w), 0xFFFFFFFF, np.uint32)
    wide[:, :rc.WORDS] = packed
    for rows, sw in ((packed, rc.WORDS), (wide, stride_w)):
        t_q = torch.from_numpy(case.Q.copy()).cuda()
        t_allow = torch.from_numpy(rows.view(np.int32)).cuda()
        t_st = torch.zeros(1, dtype=torch.int32, device="cuda")
        t_ids = torch.zeros((NQ, k), dtype=torch.int32, device="cuda")
        t_d = torch.zeros((NQ, k), dtype=torch.float32, device="cuda")
        t_cnt = [torch.zeros(NQ, dtype=torch.int32, device="cuda") for _ in range(5)]
        t_status = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        assert stream.cuda_stream != 0
        for _ in range(2):                                            # the second launch finds the scratch at its size
            case.full.search_rerank_dev(case.quant, case.qparams, t_q.data_ptr(), NQ, 4 * d, t_st.data_ptr(), 1, t_ids.data_ptr(),
                                        t_d.data_ptr(), k=k, beam=beam, normalize_first=case.mips,
                                        d_frontier_size_ptr=t_cnt[0].data_ptr(), d_visited_count_ptr=t_cnt[1].data_ptr(),
                                        d_dist_cmps_ptr=t_cnt[2].data_ptr(), d_status_ptr=t_status.data_ptr(),
                                        stream_ptr=stream.cuda_stream, d_allow_ptr=t_allow.data_ptr(), allow_stride_words=sw,
                                        d_result_count_ptr=t_cnt[3].data_ptr(), d_allowed_cmps_ptr=t_cnt[4].data_ptr())
        stream.synchronize()
        got = {"ids": t_ids, "dists": t_d, "frontier_size": t_cnt[0], "visited_count": t_cnt[1], "dist_cmps": t_cnt[2],
               "result_count": t_cnt[3], "allowed_cmps": t_cnt[4]}
        for f, t in got.items():
            assert np.array_equal(t.cpu().numpy().view(np.uint32), host[f].view(np.uint32)), (sw, f)
        assert int(t_status.cpu()[0]) == 0
    # the optional outputs left out: the list's lengths stay in the handle's scratch
    t_ids2 = torch.zeros((NQ, k), dtype=torch.int32, device="cuda")
    t_d2 = torch.zeros((NQ, k), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    case.full.search_rerank_dev(case.quant, case.qparams, t_q.data_ptr(), NQ, 4 * d, t_st.data_ptr(), 1, t_ids2.data_ptr(),
                                t_d2.data_ptr(), k=k, beam=beam, normalize_first=case.mips, stream_ptr=stream.cuda_stream,
                                d_allow_ptr=t_allow.data_ptr(), allow_stride_words=stride_w)
    stream.synchronize()
    assert np.array_equal(t_ids2.cpu().numpy().view(np.uint32), host["ids"])
    assert np.array_equal(t_d2.cpu().numpy().view(np.uint32), host["dists"].view(np.uint32))


# ---- 5. the host entry repeats the batch on a dropped-list overflow ----
@pytest.mark.parametrize("beam", [16, 100])
def test_host_entry_repeats_the_batch_on_a_dropped_list_overflow(beam):
    X, G, Q, allow, _, _ = rc.line_case()
    c = Case.__new__(Case)
    c.name, c.mips, c.X, c.Q, c.full_q = "line", False, X, Q, Q
    c.full = DeviceIndex(X, G)
    c.quant, c.qparams = c.full.quantized("euclid_u8")
    try:
        assert not c.qparams.identity
        c.quant.reserve_dropped(64)
        before = c.quant.dropped_capacity
        got = c.fused(1, beam, 100, allow, cut=1.0)                   # first, on the fresh handle
        assert got["visited_count"].max() > 600 and int(got["status"][0]) == 0
        assert c.quant.dropped_capacity > before
        _same(got, c.compose(1, beam, 100, allow, cut=1.0))
        _same(got, c.fused(1, beam, 100, cut=1.0), TRAVERSAL)
    finally:
        c.close()


# ---- 6. refusals ----
@pytest.mark.parametrize("case", ["l2_96"], indirect=True)
def test_refusals_leave_the_outputs_alone(case):
    """every row of the refusals table, on the host entry and on the _dev entry, each with its code and a message of its own
    (pann_last_error is set to another text before every call)"""
    import torch
    lib = _capi.load()
    d, k = case.X.shape[1], 10
    other_n = DeviceIndex(np.zeros((N - 1, d), np.uint8), max_degree=R)
    stream = torch.cuda.Stream()
    ones = rc.pack(np.ones(N, bool))
    BAD, UNS = _capi.PANN_ERR_BAD_ARG, _capi.PANN_ERR_UNSUPPORTED

    class Bufs:
        def __init__(self, dev):
            self.dev = dev
            mk = (lambda a: torch.from_numpy(a).cuda()) if dev else (lambda a: a)
            self.q, self.st = mk(case.Q.copy()), mk(np.zeros(1, np.int32))
            self.allow = mk(np.tile(ones, (NQ, 1)).view(np.int32))
            self.ids = mk(np.full((NQ, 64), 0x25A5A5A5, np.int32)); self.dists = mk(np.full((NQ, 64), -7.0, np.float32))
            self.cnt = mk(np.full((5, NQ), 0x25A5A5A5, np.int32)); self.status = mk(np.full(1, 0x25A5A5A5, np.int32))

        def ptr(self, a):
            return C.c_void_p(a.data_ptr() if self.dev else a.ctypes.data)

        def host(self, a):
            return a.cpu().numpy() if self.dev else a

        def untouched(self):
            return ((self.host(self.ids) == 0x25A5A5A5).all() and (self.host(self.dists) == -7.0).all()
                    and (self.host(self.cnt) == 0x25A5A5A5).all() and (self.host(self.status) == 0x25A5A5A5).all())

    def call(B, full=case.full.handle, quant=case.quant.handle, nq=NQ, use_filter=0, kk=k, beam=64, allow=True, stride=0):
        q = _capi.QueryParams(k=kk, beam=beam, cut=1.35, limit=N, degree_limit=R, rerank_factor=100, pad=1.0)
        o = _capi.RerankOut(ids=B.ptr(B.ids), dists=B.ptr(B.dists), frontier_size=B.ptr(B.cnt[0]), visited_count=B.ptr(B.cnt[1]),
                            dist_cmps=B.ptr(B.cnt[2]), pruned_cmps=None, status=B.ptr(B.status))
        assert lib.pann_index_set_option(case.full.handle, b"no-such-option", 0) == 1      # last error := another text
        assert b"unknown option" in lib.pann_last_error()
        args = [full, quant, C.byref(case.qparams), B.ptr(B.q), nq, 4 * d, 0, use_filter, B.ptr(B.st), 1, C.byref(q),
                B.ptr(B.allow) if allow else None, stride, C.byref(o), B.ptr(B.cnt[3]), B.ptr(B.cnt[4])]
        rcode = (lib.pann_batch_search_masked_rerank_dev(*args, C.c_void_p(stream.cuda_stream)) if B.dev
                 else lib.pann_batch_search_masked_rerank(*args))
        msg = lib.pann_last_error().decode()
        assert rcode == 0 or (msg and "unknown option" not in msg), msg
        return rcode

    refused = [(dict(kk=0), BAD), (dict(kk=65, beam=64), BAD), (dict(kk=33, beam=32), BAD), (dict(kk=65, beam=128), UNS),
               (dict(use_filter=1), UNS), (dict(allow=False), BAD), (dict(stride=1), BAD), (dict(stride=rc.WORDS - 1), BAD),
               (dict(quant=other_n.handle), BAD), (dict(full=case.quant.handle), UNS), (dict(full=None), BAD)]
    try:
        for dev in (False, True):
            B = Bufs(dev)
            for kw, code in refused:
                assert call(B, **kw) == code, (dev, kw)
            assert call(B, nq=0) == 0
            if dev:
                stream.synchronize()
            assert B.untouched()
            assert call(B, stride=rc.WORDS) == 0                       # the handle still works after the refusals
            if dev:
                stream.synchronize()
            ids = B.host(B.ids).reshape(-1)[:NQ * k]
            assert (ids >= 0).all() and (ids < N).all() and int(B.host(B.status)[0]) == 0
            assert (B.host(B.cnt)[3] == 64).all()
    finally:
        other_n.close()
    with pytest.raises(PannError) as e:
        case.fused(10, 64, 100, ones, use_filter=True)                                    # the Python keyword passes it through
    assert e.value.code == UNS
    with pytest.raises(ValueError):
        case.fused(10, 64, 100, np.ones((NQ + 1, rc.WORDS), np.uint32))                    # rows != queries


# ---- 7. the Python mirror ----
def _mirror(tmp_path, cls, X, G, **kw):
    io.write_bin(tmp_path / "b.bin", X)
    io.write_graph(tmp_path / "g", G)
    return cls(str(tmp_path / "b.bin"), str(tmp_path / "g"), **kw)


def _close(gi):
    gi.index.close()
    if gi.q_index is not None:
        gi.q_index.close()


@pytest.mark.parametrize("name,bits", [("l2_96", 8), ("l2_96", 4), ("mips_200", 8), ("mips_200", 4)])
def test_graph_index_masked_quantised_search_is_the_fused_call(tmp_path, cases, name, bits):
    c = cases(name)
    mips = c.mips
    gi = _mirror(tmp_path, FloatMipsIndex if mips else FloatEuclidianIndex, c.X, c.full.get_graph(), quant_bits=bits)
    try:
        assert gi.use_quantization and (mips or bits == 4 or not gi.eparams.identity)
        m = rc.mask("rand50", name)
        ids, dists = gi.batch_search_masked(c.Q, 10, 64, m, quant=True, visit_limit=1000)
        r = gi.index.search_rerank(gi.q_index, gi.qparams, c.Q, normalize_first=mips, rerank_factor=100, allow=rc.pack(m),
                                   **gi._qp(10, 64, 1000))
        assert np.array_equal(ids, r["ids"]) and np.array_equal(dists.view(np.uint32), r["dists"].view(np.uint32))
        assert (r["result_count"] == 64).all() and m[ids].all()
        io.write_bin(tmp_path / "q.bin", c.Q)
        ids2, d2 = gi.batch_search_masked_from_string(str(tmp_path / "q.bin"), 10, 64, rc.pack(m), quant=True, visit_limit=1000)
        assert np.array_equal(ids2, ids) and np.array_equal(d2.view(np.uint32), dists.view(np.uint32))
        # quant=False: exactly what batch_search(..., allow=) does
        a = gi.batch_search_masked(c.Q, 10, 64, m, visit_limit=1000)
        b = gi.batch_search(c.Q, 10, 64, visit_limit=1000, allow=m)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        # short rows come back padded, no k-results check: nothing is allowed
        z, zd = gi.batch_search_masked(c.Q, 10, 64, np.zeros(N, bool), quant=True, visit_limit=1000)
        assert (z == SENT).all() and np.isposinf(zd).all()
        with pytest.raises(ValueError):                                # batch_search keeps refusing the combination
            gi.batch_search(c.Q, 10, 64, quant=True, visit_limit=1000, allow=m)
    finally:
        _close(gi)


def test_graph_index_identity_quantiser_takes_the_plain_masked_search(tmp_path):
    """integer-valued f32 rows (the masked_cases "f32" layout) quantise to themselves (slope 1): quant=True is the masked search
    of the u8 copy on the quantised queries, as the unmasked branch"""
    import masked_cases as mc
    X, Q, _, _ = mc.layout_data("f32")
    gi = _mirror(tmp_path, FloatEuclidianIndex, X, mc.graph(32))
    try:
        assert gi.eparams.identity
        m = mc.mask("rand50", "f32")
        ids, dists = gi.batch_search_masked(Q, 10, 64, m, quant=True, visit_limit=1000)
        qq = quantize.device_quantize_rows(Q, gi.qparams)
        r = gi.q_index.batch_search_masked(qq, allow=m, out_k=10, **gi._qp(10, 64, 1000))
        assert np.array_equal(ids, r["ids"]) and np.array_equal(dists.view(np.uint32), r["dists"].view(np.uint32))
        assert m[ids].all()
    finally:
        _close(gi)


def test_graph_index_second_level_refuses_masked_quantised_searches(tmp_path, cases):
    c = cases("l2_96")
    gi = _mirror(tmp_path, FloatEuclidianIndex, c.X, c.full.get_graph(), second_level="bit")
    try:
        m = rc.mask("rand50", "l2_96")
        with pytest.raises(ValueError):
            gi.batch_search_masked(c.Q, 10, 64, m, quant=True, visit_limit=1000)
        ids, _ = gi.batch_search_masked(c.Q, 10, 64, m, quant=False, visit_limit=1000)       # the float table still serves masks
        assert m[ids].all()
    finally:
        _close(gi)


# ---- 8. tombstones on the fast path ----
def test_tombstone_round_trip_on_the_fused_path():
    """mark in the bitmap -> fused masked searches return no marked id, every row full -> vamana_delete_batch on the float handle,
    a new quantised copy -> the plain fused search returns none either"""
    from parlayann_amd import datasets
    n, Rr, d = 2000, 32, 64
    X = (datasets.deep_like(n, d, seed=1001) * 2.0).astype(np.float32)
    Q = (datasets.deep_like(64, d, seed=2001) * 2.0).astype(np.float32)
    full = DeviceIndex(X, max_degree=Rr)
    quant = quant2 = None
    try:
        full.vamana_build(Rr, 64, 1.2, num_passes=1, seed=1)
        quant, qparams = full.quantized("euclid_u8")
        deleted = np.random.default_rng(3).choice(np.arange(1, n), n // 5, replace=False).astype(np.uint32)
        allow = allow_bitmap(n, deleted_ids=deleted)
        before = full.search_rerank(quant, qparams, Q, k=10, beam=32)
        assert np.isin(before["ids"], deleted).any()                    # the plain fused search does return doomed ids
        g = full.search_rerank(quant, qparams, Q, k=10, beam=32, allow=allow)
        assert (g["result_count"] == 32).all() and (g["ids"] != SENT).all() and not np.isin(g["ids"], deleted).any()
        for f in TRAVERSAL:
            np.testing.assert_array_equal(g[f], before[f])
        full.vamana_delete_batch(deleted, Rr, 1.2)
        quant2, qparams2 = full.quantized("euclid_u8", params=qparams)  # the copy carries the consolidated graph
        after = full.search_rerank(quant2, qparams2, Q, k=10, beam=32)
        assert int(after["status"][0]) == 0 and not np.isin(after["ids"], deleted).any()
        again = full.search_rerank(quant2, qparams2, Q, k=10, beam=32, allow=allow)
        assert not np.isin(again["ids"], deleted).any()
    finally:
        for ix in (full, quant, quant2):
            if ix is not None:
                ix.close()
