"""Per-query filtered scan (pann_scan_rerank_masked_per_query* / _labeled_per_query*, DESIGN.md "Per-query filtered scan").

The reference is the sibling file's: a query's candidate list is numpy's on the unpacked integers of the rows ITS filter allows (int64
distance, -256 x the dot product for PANN_I4, cast to float32 once, stable order by (distance, id)), slots past min(c, allowed)
0xFFFFFFFF; ids / dists are pann_rerank on the returned candidates and counts, bit for bit.  Integer-valued data under identity
parameters, small ranges (ties by id are plentiful): exact arithmetic, assert_array_equal everywhere, no tolerance.
Rows of one batch cycle through six populations: 5 points (fewer than c), nothing, one point, exactly c, every point, {0, n - 1}."""
import ctypes as C

import numpy as np
import pytest

from parlayann_amd import _capi, index
from test_scan_filtered_gpu import _check, handles  # noqa: F401 (the module fixture of the refusal tests: n = 40, 5 queries)
from test_scan_rerank_gpu import KINDS, _pair

pytestmark = pytest.mark.gpu
F, U32, PAD = np.float32, np.uint32, 0xFFFFFFFF
FIVE, NONE_, ONE, CSET, ALL, ENDS = 16, 0, 64, 32, 128, 8                     # label bits of the populations (ALL: every point has it)
# per kind: the predicates the rows cycle through; the first six of "any" and "match" are the six populations
PREDS = {"any": [(FIVE, 0), (NONE_, 0), (ONE, 0), (CSET, 0), (ALL, 0), (ENDS, 0), (7, 0)],
         "match": [(FIVE, FIVE), (7, 99), (ONE, ONE), (CSET, CSET), (0, 0), (ENDS, ENDS), (7, 3), (PAD, ALL | 2)],
         "range": [(ALL + 2, ALL + 4), (5, 3), (ALL + ONE, ALL + ONE + 6), (0, ALL + 6), (0, PAD), (ALL + ENDS, ALL + ENDS + 6), (ALL + 6, ALL + 6)]}
# d (one-byte, four-bit), n, nq, k, rerank_factor, gt_pieces, whole range, pad words per bitmap row
CASES = {"c16": ((24, 24), 63, 65, 4, 4, 0, False, 0),           # one list register; partial A and B tiles, row clamping
         "c64": ((63, 63), 65, 130, 8, 8, 0, False, 3),          # four list registers, odd d, three A tiles, one column past a tile
         "one": ((24, 24), 300, 1, 4, 4, 0, False, 0),           # a single query: every row of the tile but one is a clamped one
         "twoseg": ((272, 520), 300, 7, 8, 8, 0, True, 0),       # the second 256-byte segment: the mask is applied once per tile
         "pieces": ((24, 24), 9001, 65, 8, 8, 3, False, 3)}      # pieces start at 3008 / 6016 (not multiples of 512 columns); 5 points < a share


def _filters(rng, n, nq, c, mode, pad):
    """labels (n,), the boolean rows (nq, n) and the keywords that state them: packed rows (tail bits and pad words all ones) or predicates"""
    labels = (np.arange(n) % 7 + ALL).astype(U32)
    for bit, ids in ((FIVE, rng.choice(n, 5, replace=False)), (ONE, [n // 2]), (CSET, rng.choice(n, min(c, n), replace=False)), (ENDS, [0, n - 1])):
        labels[ids] |= bit
    kind = "any" if mode == "bitmap" else mode
    preds = np.array([PREDS[kind][i % (6 if mode == "bitmap" else len(PREDS[kind]))] for i in range(nq)], U32)
    rows = index.label_allow(labels, kind, preds)
    if mode != "bitmap":
        return labels, rows, dict(where=(mode, preds), per_query=True)
    bits = np.concatenate([rows, np.ones((nq, -n % 32 + 32 * pad), bool)], axis=1)
    return labels, rows, dict(allow=np.packbits(bits, axis=1, bitorder="little").view(U32), per_query=True)


@pytest.mark.parametrize("mode", ["bitmap", "any", "match", "range"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_per_query_candidates_bit_for_bit(kind, case, mode):
    dd, n, nq, k, rf, pieces, wide, pad = CASES[case]
    d = dd[KINDS[kind][4]]
    lo, hi = KINDS[kind][3 if wide else 2]
    rng = np.random.default_rng(n + d + nq)
    labels, rows, kw = _filters(rng, n, nq, min(k * rf, 64, n), mode, pad)
    full, quant, p = _pair(kind, rng.integers(lo, hi + 1, (n, d)))
    try:
        full.set_labels(labels)
        quant.set_option("gt_pieces", pieces)
        r = _check(kind, full, quant, p, rng.integers(lo, hi + 1, (nq, d)).astype(F), k, rf, rows, np.arange(nq), **kw)
        assert (r["cand_count"] == np.minimum(rows.sum(1), r["cand_ids"].shape[1])).all()
    finally:
        quant.close(); full.close()


@pytest.mark.parametrize("kind", ["mips_i8", "euclid_u4"])
def test_equals_the_plain_scan_and_the_table_form(kind):
    """filters that allow everything: every output of pann_scan_rerank; mixed rows: every output of the table form with one entry per query"""
    rng, (n, d, nq, k, rf) = np.random.default_rng(5), (700, 40, 70, 10, 3)
    lo, hi = KINDS[kind][2]
    full, quant, p = _pair(kind, rng.integers(lo, hi + 1, (n, d)))
    try:
        full.set_labels(np.arange(n) % 7)
        Q = rng.integers(lo, hi + 1, (nq, d)).astype(F)
        run = lambda **kw: full.scan_rerank(quant, p, Q, k=k, rerank_factor=rf, candidates=True, **kw)
        rows, preds = rng.random((nq, n)) < rng.random((nq, 1)) ** 3, np.stack([np.arange(nq) % 5, np.arange(nq) % 9], 1).astype(U32)
        pairs = [(run(), dict(allow=np.ones((nq, n), bool))), (run(), dict(where=("match", np.zeros((nq, 2), U32)))),
                 (run(allow=rows, group_of_query=np.arange(nq)), dict(allow=rows)),
                 (run(where=("range", preds), group_of_query=np.arange(nq)), dict(where=("range", preds)))]
        for want, kw in pairs:
            r = run(per_query=True, **kw)
            for name in want:
                np.testing.assert_array_equal(r[name].view(U32), want[name].view(U32), err_msg=f"{sorted(kw)} {name}")
    finally:
        quant.close(); full.close()


@pytest.mark.parametrize("mode,stride", [("bitmap", 4), ("bitmap", 7), ("bitmap", 1 << 25), ("match", 0)])
def test_host_and_dev_entries_agree(mode, stride):
    """the _dev entry on a stream of its own (no synchronisation inside) returns the host entry's rows; at a stride of 2^25 words the
    slab is 5 GiB and rows from 32 on start past 4 GiB (only the first words of each row are set)"""
    import torch
    rng, (n, d, nq, k, rf) = np.random.default_rng(7), (100, 24, 40, 4, 4)
    labels, rows, kw = _filters(rng, n, nq, k * rf, mode, 0)
    full, quant, p = _pair("euclid_u8", rng.integers(0, 4, (n, d)))
    try:
        full.set_labels(labels)
        Q = rng.integers(0, 4, (nq, d)).astype(F)
        r = _check("euclid_u8", full, quant, p, Q, k, rf, rows, np.arange(nq), **kw)
        t_ids, t_cand = torch.zeros((nq, k), dtype=torch.int32, device="cuda"), torch.zeros((nq, k * rf), dtype=torch.int32, device="cuda")
        t_d, t_cnt = torch.zeros((nq, k), dtype=torch.float32, device="cuda"), torch.zeros(nq, dtype=torch.int32, device="cuda")
        t_q = torch.from_numpy(Q).cuda()
        if mode == "bitmap":
            t_f = torch.zeros((nq, stride), dtype=torch.int32, device="cuda")
            t_f[:, :4] = torch.from_numpy(kw["allow"].view(np.int32)).cuda()
            if 4 < stride < 100:
                t_f[:, 4:] = -1
            flt = dict(d_allow_ptr=t_f.data_ptr(), allow_stride_words=stride)
        else:
            t_f = torch.from_numpy(kw["where"][1].view(np.int32)).cuda()
            flt = dict(d_preds_ptr=t_f.data_ptr(), pred_kind=mode)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        full.scan_rerank_dev(quant, p, t_q.data_ptr(), nq, 4 * d, t_ids.data_ptr(), t_d.data_ptr(), k=k, rerank_factor=rf, per_query=True,
                             d_cand_ids_ptr=t_cand.data_ptr(), d_cand_count_ptr=t_cnt.data_ptr(), stream_ptr=stream.cuda_stream, **flt)
        stream.synchronize()
        for name, t in (("ids", t_ids), ("dists", t_d), ("cand_ids", t_cand), ("cand_count", t_cnt)):
            np.testing.assert_array_equal(t.cpu().numpy().view(U32), r[name].view(U32), err_msg=name)
    finally:
        quant.close(); full.close()


BAD, UNS = _capi.PANN_ERR_BAD_ARG, _capi.PANN_ERR_UNSUPPORTED
# name -> (entry family, expected code, text the message holds, overrides of the good call: 5 queries with a filter each, n = 40)
REFUSALS = {"masked null bitmap": ("masked", BAD, "null allow bitmap", dict(flt=None)),
            "masked short stride": ("masked", BAD, "allow_stride_words", dict(stride=1)),
            "masked zero stride": ("masked", BAD, "allow_stride_words", dict(stride=0)),
            "masked FP8 quant": ("masked", UNS, "PANN_F8", dict(quant="f8", p="pf8")),
            "masked k == 0": ("masked", BAD, "k must be at least 1", dict(k=0)),
            "labeled no labels": ("labeled", BAD, "no labels", dict(full="nolabels")),
            "labeled unknown kind": ("labeled", BAD, "unknown predicate kind", dict(kind=77)),
            "labeled null predicates": ("labeled", BAD, "null predicates", dict(flt=None)),
            "labeled misaligned predicates": ("labeled", BAD, "8-byte aligned", dict(misalign=4)),
            "labeled nq == 0": ("labeled", 0, "", dict(nq=0))}


# (host predicates have no alignment rule)
@pytest.mark.parametrize("case,dev", [(c, v) for c in REFUSALS for v in (False, True) if v or "misalign" not in REFUSALS[c][3]],
                         ids=lambda x: x if isinstance(x, str) else ("dev" if x else "host"))
def test_refusals_write_nothing(handles, case, dev):
    import torch
    family, code, text, over = REFUSALS[case]
    a = dict(dict(full="full", quant="u8", p="p", flt=True, stride=2, kind=_capi.PANN_PRED_MATCH, k=3, nq=5, misalign=0), **over)
    entry = f"pann_scan_rerank_{family}_per_query" + ("_dev" if dev else "")
    bufs = {"q": handles["Q"], "flt": np.full((6, 2), PAD, U32), "ids": np.full((5, 3), 0xABABABAB, U32), "dists": np.full((5, 3), 7.5, F),
            "cand": np.full((5, 6), 0xABABABAB, U32), "cnt": np.full(5, 0xABABABAB, U32)}
    if dev:
        bufs = {k: torch.from_numpy(v.view(np.int32) if v.dtype == U32 else v).cuda() for k, v in bufs.items()}
        torch.cuda.synchronize()
    ptr = (lambda t, off=0: C.c_void_p(t.data_ptr() + off)) if dev else (lambda v, off=0: C.c_void_p(v.ctypes.data + off))
    flt = ptr(bufs["flt"], a["misalign"]) if a["flt"] else None
    rc = getattr(_capi.load(), entry)(handles[a["full"]].handle, handles[a["quant"]].handle, C.byref(handles[a["p"]]), ptr(bufs["q"]), a["nq"], 32, 0,
                                      a["k"], 2, *([flt, a["stride"]] if family == "masked" else [a["kind"], flt]), ptr(bufs["ids"]),
                                      ptr(bufs["dists"]), ptr(bufs["cand"]), ptr(bufs["cnt"]), *([None] if dev else []))
    assert rc == code
    if code:
        msg = _capi.load().pann_last_error().decode()
        assert text in msg and entry in msg, msg
    if dev:
        torch.cuda.synchronize()
        bufs = {k: v.cpu().numpy() for k, v in bufs.items()}
    assert (bufs["ids"].view(U32) == 0xABABABAB).all() and (bufs["dists"] == 7.5).all()
    assert (bufs["cand"].view(U32) == 0xABABABAB).all() and (bufs["cnt"].view(U32) == 0xABABABAB).all()


def test_graph_index_per_query_exhaustive(tmp_path):
    """GraphIndex.batch_search_masked(quant=True, exhaustive=True, per_query=True) is DeviceIndex.scan_rerank(per_query=True)"""
    from parlayann_amd import io, graph_index
    rng = np.random.default_rng(11)
    X, Q = rng.standard_normal((300, 16)).astype(F), rng.standard_normal((9, 16)).astype(F)
    io.write_bin(tmp_path / "x.bin", X)
    io.write_graph(tmp_path / "g.bin", index.host_graph(300, 4))
    gi = graph_index.FloatEuclidianIndex(str(tmp_path / "x.bin"), str(tmp_path / "g.bin"), quant_bits=4)
    gi.index.set_labels(np.arange(300) % 5)
    for kw in (dict(allow=rng.random((9, 300)) < 0.3), dict(where=("match", np.array([[PAD, i % 4] for i in range(9)], U32)))):
        ids, dists = gi.batch_search_masked(Q, 5, 64, quant=True, exhaustive=True, per_query=True, **kw)
        r = gi.index.scan_rerank(gi.q_index, gi.qparams, Q, k=5, per_query=True, **kw)
        assert np.array_equal(ids, r["ids"]) and np.array_equal(dists, r["dists"])
        allowed = kw["allow"] if "allow" in kw else index.label_allow(np.arange(300) % 5, *kw["where"])
        assert allowed[np.arange(9)[:, None], ids].all()
