"""Exhaustive quantised scan + exact rerank (pann_scan_rerank*, DESIGN.md "Exhaustive quantised scan").

The scan is exact integer arithmetic: its candidate list is compared id for id with numpy on the unpacked rows of the copy and of
pann_quantize_rows (int64 distance, -256 x the dot product for PANN_I4, cast to float32 once, ordered by (distance, id)), the fused
result bit for bit with pann_rerank on the returned candidates.  Data: integer-valued floats under parameters that quantise them
to themselves; small ranges make ties plentiful, the "wide" cases use the whole range of the type at every coordinate."""
import ctypes as C

import numpy as np
import pytest

from parlayann_amd import DeviceIndex, _capi, quantize

pytestmark = pytest.mark.gpu
F, U32 = np.float32, np.uint32
# kind -> metric, identity parameters, (small range), (whole range the quantiser produces), four-bit
KINDS = {"euclid_u8": ("Euclidian", dict(slope=1.0, offset=0), (0, 3), (0, 255), False),
         "mips_i8": ("mips", dict(max_val=127.0), (-2, 2), (-127, 127), False),
         "euclid_u4": ("Euclidian", dict(slope=1.0, offset=0), (0, 2), (0, 15), True),
         "mips_i4": ("mips", dict(max_val=7.0), (-1, 1), (-7, 7), True)}


def _values(rows, kind, d):
    """rows of a copy, or quantised query rows -> int64 values"""
    if KINDS[kind][4]:
        return quantize.unpack_nibbles(rows, d, kind == "mips_i4").astype(np.int64)
    return rows.view(np.uint8 if kind == "euclid_u8" else np.int8).astype(np.int64)


def _reference(kind, B, A, c):
    """the first c ids by (float32 of the handle's integer distance, id), per query"""
    if KINDS[kind][0] == "Euclidian":
        dist = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2 * (A @ B.T)
    else:
        dist = -(A @ B.T) * (256 if kind == "mips_i4" else 1)
    return np.argsort(dist.astype(F), axis=1, kind="stable")[:, :c].astype(U32)


def _check_scan(kind, full, quant, p, Q, k, rf, **kw):
    d, c = Q.shape[1], min(k * rf, 64, quant.n)
    r = full.scan_rerank(quant, p, Q, k=k, rerank_factor=rf, candidates=True, **kw)
    norm = bool(kw.get("normalize_first"))
    Qs = quantize.normalize_rows(Q) if norm else Q
    want = _reference(kind, _values(quant.points(), kind, d), _values(quantize.device_quantize_rows(Q, p, normalize_first=norm), kind, d), c)
    assert r["cand_ids"].shape == (len(Q), c) and (r["cand_count"] == c).all()
    np.testing.assert_array_equal(r["cand_ids"], want)
    ei, ed = full.rerank(Qs, r["cand_ids"], r["cand_count"], k, resort=True)       # k > c: padded by both
    np.testing.assert_array_equal(r["ids"], ei)
    np.testing.assert_array_equal(r["dists"].view(U32), ed.view(U32))
    return r


def _pair(kind, V):
    """the float handle of the integer rows V and its copy under the identity parameters"""
    metric, pk = KINDS[kind][0], KINDS[kind][1]
    full = DeviceIndex(V.astype(F), max_degree=4, metric=metric)
    p = quantize.device_params(kind, V.shape[1], **pk)
    quant, _ = full.quantized(kind, params=p, copy_graph=False)
    return full, quant, p


# d (one-byte, four-bit), n, nq, k, rerank_factor, gt_pieces, whole range
SHAPES = [((1, 1), 5, 1, 1, 1, 0, False),            # c = 1
          ((24, 24), 63, 65, 4, 4, 0, False),        # c = 16: one list register; partial A and B tiles
          ((63, 63), 65, 130, 17, 1, 0, False),      # c = 17: several list registers; k tail, odd d; three A tiles
          ((65, 65), 1, 1, 10, 20, 0, False),        # one point: c clamps to n, k > c pads
          ((128, 128), 300, 65, 2, 100, 0, True),    # k * rerank_factor = 200 clamps to 64; every coordinate over the whole range
          ((272, 520), 65, 3, 8, 8, 0, True),        # c = 64; the second 256-byte segment
          ((24, 24), 9001, 130, 10, 2, 3, False)]    # three pieces per tile (nsplit > 1), shared thresholds, the merge


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"d{s[0][0]}-n{s[1]}-nq{s[2]}-k{s[3]}x{s[4]}" + ("-p3" if s[5] else ""))
@pytest.mark.parametrize("kind", list(KINDS))
def test_scan_candidates_bit_for_bit(kind, shape):
    d, (n, nq, k, rf, pieces, wide) = shape[0][KINDS[kind][4]], shape[1:]
    lo, hi = KINDS[kind][3 if wide else 2]
    rng = np.random.default_rng(n + d)
    full, quant, p = _pair(kind, rng.integers(lo, hi + 1, (n, d)))
    try:
        quant.set_option("gt_pieces", pieces)
        _check_scan(kind, full, quant, p, rng.integers(lo, hi + 1, (nq, d)).astype(F), k, rf)
    finally:
        quant.close(); full.close()


# every coordinate the largest or smallest value, longest rows; the quantisers clamp at -127 / -7, so -128 / 0x8 are raw rows only
EXTREMES = [("euclid_u8", 512, [255, 0], [0, 255]), ("mips_i8", 512, [-128, 127], [-127, 127]),
            ("euclid_u4", 1024, [15, 0], [0, 15]), ("mips_i4", 1024, [-8, 7], [-7, 7])]


@pytest.mark.parametrize("kind,d,rows,queries", EXTREMES, ids=[e[0] for e in EXTREMES])
def test_scan_extremes_at_the_longest_row(kind, d, rows, queries):
    metric, pk = KINDS[kind][:2]
    V = np.repeat(np.array(rows * 3)[:, None], d, axis=1)                      # six constant rows: ties, broken by id
    if KINDS[kind][4]:
        quant = DeviceIndex.from_packed(quantize.pack_nibbles(V), d, kind[-2:], max_degree=4)
    else:
        quant = DeviceIndex(V.astype(np.uint8 if kind == "euclid_u8" else np.int8), max_degree=4, metric=metric)
    full = DeviceIndex(V.astype(F), max_degree=4, metric=metric)
    try:
        Q = np.repeat(np.array(queries, F)[:, None], d, axis=1)
        r = _check_scan(kind, full, quant, quantize.device_params(kind, d, **pk), Q, 6, 1)
        if kind == "euclid_u8":                                                # 512 * 255^2 > 2^24: the far rows, the near rows
            assert r["cand_ids"].tolist() == [[1, 3, 5, 0, 2, 4], [0, 2, 4, 1, 3, 5]]
    finally:
        quant.close(); full.close()


@pytest.mark.parametrize("kind,normalize", [("euclid_u8", False), ("mips_i8", True), ("mips_i4", True), ("euclid_u4", False)])
def test_fused_result_host_and_dev(kind, normalize):
    """real-valued rows under generated parameters; the _dev entry on a stream of its own returns what the host entry returns"""
    import torch
    rng, (n, d, nq, k, rf) = np.random.default_rng(7), (500, 40, 70, 10, 3)
    full = DeviceIndex(rng.standard_normal((n, d)).astype(F), max_degree=4, metric=KINDS[kind][0])
    if normalize:
        full.normalize()
    quant, p = full.quantized(kind, copy_graph=False)
    try:
        Q = rng.standard_normal((nq, d)).astype(F)
        r = _check_scan(kind, full, quant, p, Q, k, rf, normalize_first=normalize)
        t_q = torch.from_numpy(Q).cuda()
        t_ids, t_cand = torch.zeros((nq, k), dtype=torch.int32, device="cuda"), torch.zeros((nq, k * rf), dtype=torch.int32, device="cuda")
        t_d, t_cnt = torch.zeros((nq, k), dtype=torch.float32, device="cuda"), torch.zeros(nq, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        full.scan_rerank_dev(quant, p, t_q.data_ptr(), nq, 4 * d, t_ids.data_ptr(), t_d.data_ptr(), k=k, rerank_factor=rf,
                             normalize_first=normalize, d_cand_ids_ptr=t_cand.data_ptr(), d_cand_count_ptr=t_cnt.data_ptr(),
                             stream_ptr=stream.cuda_stream)
        stream.synchronize()
        for name, t in (("ids", t_ids), ("dists", t_d), ("cand_ids", t_cand), ("cand_count", t_cnt)):
            np.testing.assert_array_equal(t.cpu().numpy().view(U32), r[name].view(U32), err_msg=name)
    finally:
        quant.close(); full.close()


@pytest.fixture(scope="module")
def handles():
    rng = np.random.default_rng(3)
    X = rng.integers(0, 200, (40, 8)).astype(F)
    h = {"full": DeviceIndex(X, max_degree=4), "small": DeviceIndex(X[:30], max_degree=4), "mips": DeviceIndex(X, max_degree=4, metric="mips"),
         "long": DeviceIndex(rng.integers(0, 200, (4, 513)).astype(F), max_degree=4)}
    h["u8"], h["p"] = h["full"].quantized("euclid_u8", copy_graph=False)
    h["f8"], h["pf8"] = h["full"].quantized("f8", copy_graph=False)
    h["small_u8"], _ = h["small"].quantized("euclid_u8", params=h["p"], copy_graph=False)
    h["i8"], h["pi8"] = h["mips"].quantized("mips_i8", copy_graph=False)
    h["long_u8"], h["plong"] = h["long"].quantized("euclid_u8", copy_graph=False)
    h["pu4"] = quantize.device_params("euclid_u4", 8)
    h["Q"] = X[:5].copy()
    yield h
    [v.close() for v in h.values() if isinstance(v, DeviceIndex)]


BAD, UNS = _capi.PANN_ERR_BAD_ARG, _capi.PANN_ERR_UNSUPPORTED
# name -> (expected code, text the message holds, overrides of the good call)
REFUSALS = {"null full": (BAD, "null index handle", dict(full=None)), "null quant": (BAD, "null index handle", dict(quant=None)),
            "null qparams": (BAD, "null parameters", dict(p=None)), "null ids": (BAD, "null parameters", dict(ids=None)),
            "null dists": (BAD, "null parameters", dict(dists=None)), "null queries": (BAD, "null queries", dict(q=None)),
            "k == 0": (BAD, "k must be at least 1", dict(k=0)), "rerank_factor < 1": (BAD, "rerank_factor", dict(rf=0)),
            "n differs": (BAD, "must agree", dict(quant="small_u8")), "metric differs": (BAD, "must agree", dict(quant="i8", p="pi8")),
            "kind does not fit": (BAD, "do not fit", dict(p="pu4")), "short stride": (BAD, "stride", dict(stride=28)),
            "odd stride": (BAD, "stride", dict(stride=34)), "full not f32": (UNS, "PANN_F32", dict(full="u8")),
            "FP8 quant": (UNS, "PANN_F8", dict(quant="f8", p="pf8")), "float quant": (UNS, "PANN_F32", dict(quant="full")),
            "long rows": (UNS, "512 bytes", dict(full="long", quant="long_u8", p="plong")), "nq == 0": (0, "", dict(nq=0))}


@pytest.mark.parametrize("entry", ["pann_scan_rerank", "pann_scan_rerank_dev"])
@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_write_nothing(handles, case, entry):
    import torch
    code, text, over = REFUSALS[case]
    a = dict(dict(full="full", quant="u8", p="p", q=True, ids=True, dists=True, k=3, rf=2, nq=5, stride=32), **over)
    dev = entry.endswith("_dev")
    bufs = {"q": handles["Q"], "ids": np.full((5, 3), 0xABABABAB, U32), "dists": np.full((5, 3), 7.5, F), "cand": np.full((5, 6), 0xABABABAB, U32)}
    if dev:
        bufs = {k: torch.from_numpy(v).cuda() for k, v in bufs.items()}
        torch.cuda.synchronize()
    ptr = (lambda t: C.c_void_p(t.data_ptr())) if dev else (lambda v: v.ctypes.data_as(C.c_void_p))
    hd = lambda name: None if name is None else handles[name].handle
    rc = getattr(_capi.load(), entry)(hd(a["full"]), hd(a["quant"]), None if a["p"] is None else C.byref(handles[a["p"]]),
                                      ptr(bufs["q"]) if a["q"] else None, a["nq"], a["stride"], 0, a["k"], a["rf"],
                                      ptr(bufs["ids"]) if a["ids"] else None, ptr(bufs["dists"]) if a["dists"] else None, ptr(bufs["cand"]),
                                      None, *([None] if dev else []))
    assert rc == code
    if code:
        msg = _capi.load().pann_last_error().decode()
        assert text in msg and entry in msg, msg
    if dev:
        torch.cuda.synchronize()
        bufs = {k: v.cpu().numpy() for k, v in bufs.items()}
    assert (bufs["ids"] == 0xABABABAB).all() and (bufs["dists"] == 7.5).all() and (bufs["cand"] == 0xABABABAB).all()


def test_graph_index_exhaustive(tmp_path):
    """GraphIndex.batch_search(quant=True, exhaustive=True) is the scan + rerank of its copy; filters are refused with it"""
    from parlayann_amd import io, graph_index, index
    rng = np.random.default_rng(11)
    X, Q = rng.standard_normal((300, 16)).astype(F), rng.standard_normal((9, 16)).astype(F)
    io.write_bin(tmp_path / "x.bin", X)
    io.write_graph(tmp_path / "g.bin", index.host_graph(300, 4))
    gi = graph_index.FloatEuclidianIndex(str(tmp_path / "x.bin"), str(tmp_path / "g.bin"), quant_bits=4)
    ids, dists = gi.batch_search(Q, 5, 64, quant=True, exhaustive=True)
    r = gi.index.scan_rerank(gi.q_index, gi.qparams, Q, k=5)
    assert np.array_equal(ids, r["ids"]) and np.array_equal(dists, r["dists"])
    for bad in (dict(quant=True, allow=np.ones(300, bool)), dict(quant=False)):
        with pytest.raises(ValueError):
            gi.batch_search(Q, 5, 64, exhaustive=True, **bad)
