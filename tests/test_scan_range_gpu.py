"""Quantised range scan + exact recheck (pann_scan_range*, DESIGN.md "Quantised range scan").

The scan is exact integer arithmetic: with radius = +inf the result is the candidate set, compared id for id with numpy on the unpacked
rows (int64 distance, -256 x the dot product for PANN_I4, cast to float32 once, <= scan_radius).  The recheck is compared with
query_distances on all ids, bit for bit.  Data as tests/test_scan_rerank_gpu.py: integer-valued floats under identity parameters."""
import ctypes as C

import numpy as np
import pytest

from parlayann_amd import DeviceIndex, _capi, quantize
from test_scan_rerank_gpu import KINDS, _pair, _values

pytestmark = pytest.mark.gpu
F, U32, INF = np.float32, np.uint32, float("inf")


def _dq(kind, quant, p, Q):
    """the copy's own distance of every (query, row) pair: exact integers, cast to float32 once"""
    d = Q.shape[1]
    B, A = _values(quant.points(), kind, d), _values(quantize.device_quantize_rows(Q, p), kind, d)
    if KINDS[kind][0] == "Euclidian":
        return ((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2 * (A @ B.T)).astype(F)
    return (-(A @ B.T) * (256 if kind == "mips_i4" else 1)).astype(F)


def _csr(inside):
    """boolean (nq, n) -> offsets, ids (ascending per query)"""
    return np.concatenate([[0], np.cumsum(inside.sum(1))]).astype(np.uint64), np.nonzero(inside)[1].astype(U32)


# d (one-byte, four-bit), n, nq, gt_pieces, whole range
SHAPES = [((1, 1), 5, 1, 0, False), ((24, 24), 63, 65, 0, False), ((63, 63), 65, 130, 0, False), ((128, 128), 300, 65, 0, True),
          ((272, 520), 65, 3, 0, True),              # the second 256-byte segment
          ((24, 24), 9001, 130, 3, False)]           # three pieces per tile


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"d{s[0][0]}-n{s[1]}-nq{s[2]}" + ("-p3" if s[3] else ""))
@pytest.mark.parametrize("kind", list(KINDS))
def test_scan_candidates_id_for_id(kind, shape):
    d, (n, nq, pieces, wide) = shape[0][KINDS[kind][4]], shape[1:]
    lo, hi = KINDS[kind][3 if wide else 2]
    rng = np.random.default_rng(n + d)
    full, quant, p = _pair(kind, rng.integers(lo, hi + 1, (n, d)))
    try:
        quant.set_option("gt_pieces", pieces)
        Q = rng.integers(lo, hi + 1, (nq, d)).astype(F)
        D = _dq(kind, quant, p, Q)
        # below the smallest distance: every list empty; a distance that occurs: == is inside; above the largest: every row, lists > 64
        for sr in (np.nextafter(D.min(), F(-INF)), np.sort(D, axis=None)[D.size // 2], np.nextafter(D.max(), F(INF))):
            r = full.scan_range(quant, p, Q, INF, scan_radius=float(sr))
            off, ids = _csr(D <= sr)
            np.testing.assert_array_equal(r["offsets"], off)
            np.testing.assert_array_equal(r["ids"], ids)
            assert r["cand_total"] == len(ids)
    finally:
        quant.close(); full.close()


@pytest.fixture(scope="module", params=[("euclid_u8", False), ("mips_i8", True), ("euclid_u4", False), ("mips_i4", True)], ids=lambda k: k[0])
def real(request):
    """real-valued rows under generated parameters (normalize_first for the MIPS kinds); D: full's exact distances to all ids, once"""
    kind, normalize = request.param
    rng, (n, d, nq) = np.random.default_rng(7), (500, 40, 70)
    full = DeviceIndex(rng.standard_normal((n, d)).astype(F), max_degree=4, metric=KINDS[kind][0])
    if normalize:
        full.normalize()
    quant, p = full.quantized(kind, copy_graph=False)
    Q = rng.standard_normal((nq, d)).astype(F)
    D = full.query_distances(quantize.normalize_rows(Q) if normalize else Q, np.arange(n))
    yield dict(full=full, quant=quant, p=p, Q=Q, D=D, normalize=normalize, radius=float(np.sort(D, axis=None)[D.size // 10]))
    quant.close(); full.close()


def test_recheck_bit_for_bit(real):
    """scan_radius = +inf: every row is a candidate, the result is the exact radius join; the radius is an entry of D"""
    r = real["full"].scan_range(real["quant"], real["p"], real["Q"], real["radius"], scan_radius=INF, normalize_first=real["normalize"], dists=True)
    inside = real["D"] <= F(real["radius"])
    off, ids = _csr(inside)
    np.testing.assert_array_equal(r["offsets"], off)
    np.testing.assert_array_equal(r["ids"], ids)
    np.testing.assert_array_equal(r["dists"].view(U32), real["D"][inside].view(U32))
    assert r["cand_total"] == real["D"].size


@pytest.mark.parametrize("kind", list(KINDS))
def test_both_radii_equal_bruteforce_range(kind):
    """integer rows under identity parameters: scan_radius = quantize.scan_radius(radius, slack 0) makes both sides exact"""
    lo, hi = KINDS[kind][2]
    rng = np.random.default_rng(5)
    full, quant, p = _pair(kind, rng.integers(lo, hi + 1, (300, 24)))
    try:
        Q = rng.integers(lo, hi + 1, (65, 24)).astype(F)
        radius = float(np.sort(full.query_distances(Q, np.arange(300)), axis=None)[3000])
        r = full.scan_range(quant, p, Q, radius)
        off, ids = full.bruteforce_range(Q, radius)
        assert len(ids) >= 3000 and r["cand_total"] == len(ids)
        np.testing.assert_array_equal(r["offsets"], off)
        np.testing.assert_array_equal(r["ids"], ids)
    finally:
        quant.close(); full.close()


def test_dev_entry_capacity_and_count_only(real):
    """the _dev entry on a stream of its own returns the host entry's bytes; one id short is PANN_ERR_OVERFLOW with the offsets
    written and the ids untouched; out_ids = NULL counts"""
    import torch
    full, quant, p, Q = real["full"], real["quant"], real["p"], real["Q"]
    sr = quantize.scan_radius(p.kind, p, real["radius"], 0.5)
    r = full.scan_range(quant, p, Q, real["radius"], scan_radius=sr, normalize_first=real["normalize"], dists=True)
    total, nq = len(r["ids"]), len(Q)
    assert 0 < total <= r["cand_total"] < real["D"].size
    t_q = torch.from_numpy(Q).cuda()
    t_off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    t_ids, t_d = torch.full((total,), -1, dtype=torch.int32, device="cuda"), torch.full((total,), 7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    call = lambda ids, cap: full.scan_range_dev(quant, p, t_q.data_ptr(), nq, Q.shape[1] * 4, real["radius"], sr, t_off.data_ptr(), ids,
                                                t_d.data_ptr(), cap, normalize_first=real["normalize"], stream_ptr=stream.cuda_stream)
    with pytest.raises(_capi.PannError) as e:
        call(t_ids.data_ptr(), total - 1)
    assert e.value.code == _capi.PANN_ERR_OVERFLOW
    np.testing.assert_array_equal(t_off.cpu().numpy().view(np.uint64), r["offsets"])
    assert (t_ids.cpu().numpy() == -1).all() and (t_d.cpu().numpy() == 7.5).all()
    t_off.zero_(); torch.cuda.synchronize()
    assert call(None, 0) == r["cand_total"]                                   # count only
    np.testing.assert_array_equal(t_off.cpu().numpy().view(np.uint64), r["offsets"])
    assert (t_ids.cpu().numpy() == -1).all()
    assert call(t_ids.data_ptr(), total) == r["cand_total"]
    for name, t in (("offsets", t_off), ("ids", t_ids), ("dists", t_d)):
        assert t.cpu().numpy().tobytes() == r[name].tobytes(), name


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


BAD, UNS, NAN = _capi.PANN_ERR_BAD_ARG, _capi.PANN_ERR_UNSUPPORTED, float("nan")
# name -> (expected code, text the message holds, overrides of the good call)
REFUSALS = {"null full": (BAD, "null index handle", dict(full=None)), "null quant": (BAD, "null index handle", dict(quant=None)),
            "null qparams": (BAD, "null parameters", dict(p=None)), "null offsets": (BAD, "null parameters", dict(off=None)),
            "null queries": (BAD, "null queries", dict(q=None)), "NaN radius": (BAD, "NaN", dict(radius=NAN)),
            "NaN scan_radius": (BAD, "NaN", dict(scan_radius=NAN)), "n differs": (BAD, "must agree", dict(quant="small_u8")),
            "metric differs": (BAD, "must agree", dict(quant="i8", p="pi8")), "kind does not fit": (BAD, "do not fit", dict(p="pu4")),
            "short stride": (BAD, "stride", dict(stride=28)), "odd stride": (BAD, "stride", dict(stride=34)),
            "full not f32": (UNS, "PANN_F32", dict(full="u8")), "FP8 quant": (UNS, "PANN_F8", dict(quant="f8", p="pf8")),
            "float quant": (UNS, "PANN_F32", dict(quant="full")), "long rows": (UNS, "512 bytes", dict(full="long", quant="long_u8", p="plong")),
            "nq == 0": (0, "", dict(nq=0))}


@pytest.mark.parametrize("entry", ["pann_scan_range", "pann_scan_range_dev"])
@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_write_nothing(handles, case, entry):
    import torch
    code, text, over = REFUSALS[case]
    a = dict(dict(full="full", quant="u8", p="p", q=True, off=True, radius=1e9, scan_radius=1e9, nq=5, stride=32), **over)
    dev = entry.endswith("_dev")
    bufs = {"q": handles["Q"], "off": np.full(6, 0xABABABAB, np.uint64), "ids": np.full(200, 0xABABABAB, U32), "dists": np.full(200, 7.5, F)}
    if dev:
        bufs = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).cuda() for k, v in bufs.items()}
        torch.cuda.synchronize()
    ptr = (lambda t: C.c_void_p(t.data_ptr())) if dev else (lambda v: v.ctypes.data_as(C.c_void_p))
    hd = lambda name: None if name is None else handles[name].handle
    total = C.c_uint64(0xABAB)
    rc = getattr(_capi.load(), entry)(hd(a["full"]), hd(a["quant"]), None if a["p"] is None else C.byref(handles[a["p"]]),
                                      ptr(bufs["q"]) if a["q"] else None, a["nq"], a["stride"], 0, a["radius"], a["scan_radius"],
                                      ptr(bufs["off"]) if a["off"] else None, ptr(bufs["ids"]), ptr(bufs["dists"]), 200, C.byref(total),
                                      *([None] if dev else []))
    assert rc == code
    if code:
        msg = _capi.load().pann_last_error().decode()
        assert text in msg and entry in msg, msg
    if dev:
        torch.cuda.synchronize()
        bufs = {k: v.cpu().numpy() for k, v in bufs.items()}
    assert (bufs["off"].view(np.uint64) == 0xABABABAB).all() and (bufs["ids"] == 0xABABABAB).all() and (bufs["dists"] == 7.5).all()
    assert total.value == 0xABAB
