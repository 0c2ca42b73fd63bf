"""Filtered exhaustive scan (pann_scan_rerank_masked* / _labeled*, DESIGN.md "Filtered exhaustive scan").

Step 2 is exact integer arithmetic: a query's candidate list is numpy's on the unpacked integers of the ALLOWED rows (int64 distance,
cast to float32 once, stable argsort, ids mapped back), slots past min(c, allowed) 0xFFFFFFFF.  Step 3 is pann_rerank on the returned
candidates and counts, bit for bit.  No tolerance anywhere.  Filters are made from labels: table entry e allows the points whose
label is ent[e], as a bitmap row or as a "match" predicate; the labelled points are scattered over the table by a permutation."""
import ctypes as C

import numpy as np
import pytest

from parlayann_amd import DeviceIndex, _capi, quantize
from test_scan_rerank_gpu import KINDS, _pair, _reference, _values

pytestmark = pytest.mark.gpu
F, U32, PAD = np.float32, np.uint32, 0xFFFFFFFF
NOTHING = 999                                            # a label no point carries
FORMS = ["bitmap", "pred", "bitmap_table", "pred_table"]

# name: d (one-byte, four-bit), n, points per label, label of every table entry, queries per entry, entry of the one-filter forms,
#       k, rerank_factor, gt_pieces, max_list_ids of the second run (0: none), whole range
CASES = {
    # lists of 0 / 1 / 63 / 65 / 5 ids at c = 16: padding and counts (c_q < c), a partial B tile, one more than a tile
    "short": ((24, 24), 200, [0, 1, 63, 65, 5], [0, 1, 2, 3, 4], [2, 3, 1, 65, 2], 4, 4, 4, 0, 0, False),
    # ids scattered over 9001 rows (a gather, not a prefix), odd d, c = 17: several list registers; 130 queries = A tiles 64 / 64 / 2
    "scatter": ((63, 63), 9001, [130, 700], [0, 1], [130, 1], 0, 17, 1, 0, 0, False),
    # the second 256-byte segment under the gather, c = 64, every coordinate over the whole range
    "twoseg": ((272, 520), 300, [65, 100], [0, 1], [3, 2], 1, 8, 8, 0, 0, True),
    # three pieces per list: 130 ids = 64 + 64 + 2, 5 ids = one piece and two EMPTY ones, 0 ids = nothing
    "pieces": ((24, 24), 9001, [5, 130], [0, 1, NOTHING], [1, 65, 2], 1, 10, 2, 3, 0, False),
    # an entry no query names, an entry that allows nothing, a repeated entry; groups of 1 / 65 / 130 queries (A tiles that end inside
    # a segment); max_list_ids = 100 cuts the used entries (70 + 0 | 70 ids) into two chunks
    "table": ((24, 24), 500, [70, 30], [0, 1, NOTHING, 0], [1, 0, 65, 130], 3, 3, 3, 0, 100, False),
}


def _filters(rng, n, per_label, ent):
    """labels (n,), boolean rows (G, n), predicates (G, 2)"""
    labels, perm, at = np.full(n, 7777, U32), rng.permutation(n), 0
    for lab, cnt in enumerate(per_label):
        labels[perm[at:at + cnt]] = lab
        at += cnt
    return labels, labels[None, :] == np.array(ent, U32)[:, None], np.array([[PAD, e] for e in ent], U32)


def _check(kind, full, quant, p, Q, k, rf, rows, group, normalize=False, **kw):
    """scan_rerank(**kw) against numpy per table entry, then against pann_rerank on what it returned -> the result dict"""
    nq, d, c = len(Q), Q.shape[1], min(k * rf, 64, quant.n)
    r = full.scan_rerank(quant, p, Q, k=k, rerank_factor=rf, candidates=True, normalize_first=normalize, **kw)
    B, A = _values(quant.points(), kind, d), _values(quantize.device_quantize_rows(Q, p, normalize_first=normalize), kind, d)
    want, cnt = np.full((nq, c), PAD, U32), np.zeros(nq, U32)
    for g in np.unique(group):
        ids, qs = np.flatnonzero(rows[g]).astype(U32), np.flatnonzero(group == g)
        if len(ids):
            order = _reference(kind, B[ids], A[qs], c)
            want[qs, :order.shape[1]], cnt[qs] = ids[order], order.shape[1]
    assert r["cand_ids"].shape == (nq, c)
    np.testing.assert_array_equal(r["cand_count"], cnt)
    np.testing.assert_array_equal(r["cand_ids"], want)
    ei, ed = full.rerank(quantize.normalize_rows(Q) if normalize else Q, r["cand_ids"], r["cand_count"], k, resort=True)
    np.testing.assert_array_equal(r["ids"], ei)
    np.testing.assert_array_equal(r["dists"].view(U32), ed.view(U32))
    return r


def _form_kw(form, rows, preds, group, one):
    """the keywords of a filter form and the table index of every query under it"""
    if form == "bitmap":
        return dict(allow=rows[one]), np.full(len(group), one)
    if form == "pred":
        return dict(where=("match", tuple(int(x) for x in preds[one]))), np.full(len(group), one)
    if form == "bitmap_table":
        return dict(allow=rows, group_of_query=group), group
    return dict(where=("match", preds), group_of_query=group), group


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_filtered_candidates_bit_for_bit(kind, case, form):
    dd, n, per_label, ent, per_entry, one, k, rf, pieces, small, wide = CASES[case]
    d = dd[KINDS[kind][4]]
    lo, hi = KINDS[kind][3 if wide else 2]
    rng = np.random.default_rng(n + d)
    labels, rows, preds = _filters(rng, n, per_label, ent)
    group = rng.permutation(np.repeat(np.arange(len(ent)), per_entry)).astype(U32)      # the caller's order is not the sorted one
    full, quant, p = _pair(kind, rng.integers(lo, hi + 1, (n, d)))
    try:
        full.set_labels(labels)
        quant.set_option("gt_pieces", pieces)
        Q = rng.integers(lo, hi + 1, (len(group), d)).astype(F)
        kw, g = _form_kw(form, rows, preds, group, one)
        r = _check(kind, full, quant, p, Q, k, rf, rows, g, **kw)
        if small and form.endswith("table"):            # two chunks: the same answer
            r2 = full.scan_rerank(quant, p, Q, k=k, rerank_factor=rf, candidates=True, max_list_ids=small, **kw)
            for name in r:
                np.testing.assert_array_equal(r2[name].view(U32), r[name].view(U32), err_msg=name)
    finally:
        quant.close(); full.close()


@pytest.mark.parametrize("kind", ["mips_i8", "euclid_u4"])
def test_all_ones_filter_equals_the_plain_scan(kind):
    rng, (n, d, nq, k, rf) = np.random.default_rng(5), (700, 40, 70, 10, 3)
    lo, hi = KINDS[kind][2]
    full, quant, p = _pair(kind, rng.integers(lo, hi + 1, (n, d)))
    try:
        full.set_labels(np.zeros(n, U32))
        Q = rng.integers(lo, hi + 1, (nq, d)).astype(F)
        plain = full.scan_rerank(quant, p, Q, k=k, rerank_factor=rf, candidates=True)
        table = dict(allow=np.ones((2, n), bool), group_of_query=rng.integers(0, 2, nq))
        for kw in (dict(allow=np.ones(n, bool)), dict(where=("match", (0, 0))), table):
            r = full.scan_rerank(quant, p, Q, k=k, rerank_factor=rf, candidates=True, **kw)
            for name in plain:
                np.testing.assert_array_equal(r[name].view(U32), plain[name].view(U32), err_msg=f"{sorted(kw)} {name}")
    finally:
        quant.close(); full.close()


@pytest.mark.parametrize("kind,normalize", [("euclid_u8", False), ("mips_i8", True)])
def test_host_and_dev_entries_agree(kind, normalize):
    """real-valued rows under generated parameters, a bitmap table; the _dev entry on a stream of its own returns the host entry's rows"""
    import torch
    rng, (n, d, nq, k, rf, G) = np.random.default_rng(7), (500, 40, 70, 10, 3, 3)
    full = DeviceIndex(rng.standard_normal((n, d)).astype(F), max_degree=4, metric=KINDS[kind][0])
    if normalize:
        full.normalize()
    quant, p = full.quantized(kind, copy_graph=False)
    try:
        Q = rng.standard_normal((nq, d)).astype(F)
        rows, group = rng.random((G, n)) < np.array([0.5, 0.02, 0.2])[:, None], rng.integers(0, G, nq).astype(U32)
        r = _check(kind, full, quant, p, Q, k, rf, rows, group, normalize=normalize, allow=rows, group_of_query=group)
        packed = np.ascontiguousarray(np.packbits(rows, axis=1, bitorder="little")).copy()
        packed = np.concatenate([packed, np.zeros((G, -packed.shape[1] % 4), np.uint8)], axis=1).view(U32)
        t_q, t_rows, t_g = (torch.from_numpy(a).cuda() for a in (Q, packed.view(np.int32), group.view(np.int32)))
        t_ids, t_cand = torch.zeros((nq, k), dtype=torch.int32, device="cuda"), torch.zeros((nq, k * rf), dtype=torch.int32, device="cuda")
        t_d, t_cnt = torch.zeros((nq, k), dtype=torch.float32, device="cuda"), torch.zeros(nq, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        full.scan_rerank_dev(quant, p, t_q.data_ptr(), nq, 4 * d, t_ids.data_ptr(), t_d.data_ptr(), k=k, rerank_factor=rf, normalize_first=normalize,
                             d_cand_ids_ptr=t_cand.data_ptr(), d_cand_count_ptr=t_cnt.data_ptr(), stream_ptr=stream.cuda_stream,
                             d_allow_ptr=t_rows.data_ptr(), nrows=G, allow_stride_words=packed.shape[1], d_group_ptr=t_g.data_ptr())
        stream.synchronize()
        for name, t in (("ids", t_ids), ("dists", t_d), ("cand_ids", t_cand), ("cand_count", t_cnt)):
            np.testing.assert_array_equal(t.cpu().numpy().view(U32), r[name].view(U32), err_msg=name)
    finally:
        quant.close(); full.close()


@pytest.fixture(scope="module")
def handles():
    rng = np.random.default_rng(3)
    X = rng.integers(0, 200, (40, 8)).astype(F)
    h = {"full": DeviceIndex(X, max_degree=4), "nolabels": DeviceIndex(X, max_degree=4)}
    h["full"].set_labels(np.arange(40) % 3)
    h["u8"], h["p"] = h["full"].quantized("euclid_u8", copy_graph=False)
    h["f8"], h["pf8"] = h["full"].quantized("f8", copy_graph=False)
    h["Q"] = X[:5].copy()
    yield h
    [v.close() for v in h.values() if isinstance(v, DeviceIndex)]


BAD, UNS = _capi.PANN_ERR_BAD_ARG, _capi.PANN_ERR_UNSUPPORTED
# name -> (entry family, expected code, text the message holds, overrides of the good call: a table of 2 filters, 5 queries, n = 40)
REFUSALS = {"masked null bitmap": ("masked", BAD, "null allow bitmap", dict(flt=None)),
            "masked short stride": ("masked", BAD, "allow_stride_words", dict(stride=1)),
            "masked empty table": ("masked", BAD, "empty filter table", dict(count=0)),
            "masked index out of range": ("masked", BAD, "out of range", dict(group=[0, 1, 2, 0, 1])),
            "masked two rows, no index": ("masked", BAD, "one filter for the batch", dict(group=None)),
            "masked FP8 quant": ("masked", UNS, "PANN_F8", dict(quant="f8", p="pf8")),
            "masked k == 0": ("masked", BAD, "k must be at least 1", dict(k=0)),
            "labeled no labels": ("labeled", BAD, "no labels", dict(full="nolabels")),
            "labeled unknown kind": ("labeled", BAD, "unknown predicate kind", dict(kind=77)),
            "labeled null predicates": ("labeled", BAD, "null predicates", dict(flt=None)),
            "labeled misaligned predicates": ("labeled", BAD, "8-byte aligned", dict(misalign=4)),
            "labeled empty table": ("labeled", BAD, "empty filter table", dict(count=0)),
            "labeled index out of range": ("labeled", BAD, "out of range", dict(group=[0, 1, 0, 5, 1])),
            "labeled FP8 quant": ("labeled", UNS, "PANN_F8", dict(quant="f8", p="pf8")),
            "labeled nq == 0": ("labeled", 0, "", dict(nq=0))}


# (host predicates have no alignment rule)
@pytest.mark.parametrize("case,dev", [(c, v) for c in REFUSALS for v in (False, True) if v or "misalign" not in REFUSALS[c][3]],
                         ids=lambda x: x if isinstance(x, str) else ("dev" if x else "host"))
def test_refusals_write_nothing(handles, case, dev):
    import torch
    family, code, text, over = REFUSALS[case]
    a = dict(dict(full="full", quant="u8", p="p", flt=True, count=2, stride=2, kind=_capi.PANN_PRED_MATCH, group=[0, 1, 0, 1, 1], k=3, nq=5, misalign=0), **over)
    entry = f"pann_scan_rerank_{family}" + ("_dev" if dev else "")
    flt = np.full((2, 2), PAD, U32) if family == "masked" else np.array([[PAD, 0], [PAD, 1], [0, 0]], U32)
    bufs = {"q": handles["Q"], "flt": flt, "group": np.array(a["group"] or [0], U32), "ids": np.full((5, 3), 0xABABABAB, U32),
            "dists": np.full((5, 3), 7.5, F), "cand": np.full((5, 6), 0xABABABAB, U32), "cnt": np.full(5, 0xABABABAB, U32)}
    if dev:
        bufs = {k: torch.from_numpy(v.view(np.int32) if v.dtype == U32 else v).cuda() for k, v in bufs.items()}
        torch.cuda.synchronize()
    ptr = (lambda t, off=0: C.c_void_p(t.data_ptr() + off)) if dev else (lambda v, off=0: C.c_void_p(v.ctypes.data + off))
    mid = [ptr(bufs["flt"], a["misalign"]) if a["flt"] else None, a["count"]]
    mid = mid + [a["stride"]] if family == "masked" else [a["kind"]] + mid
    rc = getattr(_capi.load(), entry)(handles[a["full"]].handle, handles[a["quant"]].handle, C.byref(handles[a["p"]]), ptr(bufs["q"]), a["nq"], 32, 0,
                                      a["k"], 2, *mid, ptr(bufs["group"]) if a["group"] else None, 0, ptr(bufs["ids"]), ptr(bufs["dists"]),
                                      ptr(bufs["cand"]), ptr(bufs["cnt"]), *([None] if dev else []))
    assert rc == code
    if code:
        msg = _capi.load().pann_last_error().decode()
        assert text in msg and entry in msg, msg
    if dev:
        torch.cuda.synchronize()
        bufs = {k: v.cpu().numpy() for k, v in bufs.items()}
    assert (bufs["ids"].view(U32) == 0xABABABAB).all() and (bufs["dists"] == 7.5).all()
    assert (bufs["cand"].view(U32) == 0xABABABAB).all() and (bufs["cnt"].view(U32) == 0xABABABAB).all()


def test_graph_index_filtered_exhaustive(tmp_path):
    """GraphIndex.batch_search_masked(quant=True, exhaustive=True) is DeviceIndex.scan_rerank under the same filter"""
    from parlayann_amd import io, graph_index, index
    rng = np.random.default_rng(11)
    X, Q = rng.standard_normal((300, 16)).astype(F), rng.standard_normal((9, 16)).astype(F)
    io.write_bin(tmp_path / "x.bin", X)
    io.write_graph(tmp_path / "g.bin", index.host_graph(300, 4))
    gi = graph_index.FloatEuclidianIndex(str(tmp_path / "x.bin"), str(tmp_path / "g.bin"), quant_bits=4)
    gi.index.set_labels(np.arange(300) % 5)
    mask = rng.random(300) < 0.3
    ids, dists = gi.batch_search_masked(Q, 5, 64, allow=mask, quant=True, exhaustive=True)
    r = gi.index.scan_rerank(gi.q_index, gi.qparams, Q, k=5, allow=mask)
    assert np.array_equal(ids, r["ids"]) and np.array_equal(dists, r["dists"]) and np.isin(ids, np.flatnonzero(mask)).all()
    preds = np.array([[PAD, i % 2] for i in range(9)], U32)               # per-query predicates, two distinct ones
    ids, dists = gi.batch_search_masked(Q, 5, 64, where=("match", preds), quant=True, exhaustive=True)
    r = gi.index.scan_rerank(gi.q_index, gi.qparams, Q, k=5, where=("match", preds[:2]), group_of_query=np.arange(9) % 2)
    assert np.array_equal(ids, r["ids"]) and np.array_equal(dists, r["dists"]) and (np.arange(300)[ids] % 5 == (np.arange(9) % 2)[:, None]).all()
