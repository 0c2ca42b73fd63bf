"""Exact kNN by predicate group on the device (DESIGN.md "Exact kNN by predicate group"): a table of filters and one table index per
query, answered by one segmented dense launch per chunk of table entries.

    bit equality    ids, dists and counts equal tests/grouped_knn_cases.reference (the CPU oracle's brute force per distinct
                    filter, rows placed by the index array) for five element types, k = 1 / 10 / 128, f32 also in
                    exact-float-order mode, for the label form and the bitmap form; and equal the shared-route twin called once per
                    distinct filter; max_list_ids = 3000 (chunks end between groups, two groups exceed it alone) gives the same bits
    real values     rows equal the shared-route twin bit for bit on real-valued f16 and f32 data: a (query, row) distance is the
                    same instruction sequence wherever the pair sits in a tile
    _dev entries    behind a busy stream (tests/stream_order.py): inputs arrive late, outputs are poisoned late
    refusals        an index >= npreds leaves poisoned outputs untouched; k = 129; a four-bit handle; no labels
    Python          the dedup form of bruteforce_knn_grouped; GraphIndex exact_grouped=True equals False
The table, its regimes and the shapes: tests/grouped_knn_cases.py (tests/test_grouped_knn_cpu.py asserts them from the oracle)."""
import ctypes as C

import numpy as np
import pytest

import grouped_knn_cases as gc
import stream_order
from parlayann_amd import DeviceIndex, PannError, _capi
from parlayann_amd.index import label_allow

pytestmark = pytest.mark.gpu


def _same(got, want, msg):
    for g, w, f in zip(got, want, ("ids", "dists", "counts")):
        np.testing.assert_array_equal(np.asarray(g).view(np.uint32), np.asarray(w).view(np.uint32), err_msg=f"{msg}: {f}")


def _twin(ix, Q, k, g, call):
    """the shared-route twin once per distinct table entry, rows placed by the index array; call(queries, entry) -> (ids, dists, counts)"""
    ids = np.empty((len(Q), k), np.uint32); dists = np.empty((len(Q), k), np.float32); counts = np.empty(len(Q), np.uint32)
    for e in np.unique(g):
        sel = np.flatnonzero(g == e)
        ids[sel], dists[sel], counts[sel] = call(np.ascontiguousarray(Q[sel]), int(e))
    return ids, dists, counts


@pytest.mark.parametrize("tname,metric,d,exact", gc.GRID, ids=gc.GRID_IDS)
def test_equals_the_oracle_the_twin_and_itself_in_chunks(oracle, tname, metric, d, exact):
    X, Q = gc.data(tname, d)
    lab, g = gc.labels(), gc.group_of_query()
    ix = DeviceIndex(X, max_degree=4, metric=metric, exact_float_order=exact)
    try:
        ix.set_labels(lab)
        for k in gc.KS:
            want = gc.reference(oracle, tname, metric, d, k)
            table, rows = gc.table(k), gc.bitmap_rows(lab, k)
            by_label = ix.bruteforce_knn_grouped(Q, k, where=("range", table), group_of_query=g)
            _same(by_label, want, f"k={k} labels")
            by_rows = ix.bruteforce_knn_grouped(Q, k, allow=rows, group_of_query=g)
            _same(by_rows, want, f"k={k} bitmap rows")
            _same(ix.bruteforce_knn_grouped(Q, k, where=("range", table), group_of_query=g, max_list_ids=gc.CHUNK_IDS), want,
                  f"k={k} labels, max_list_ids={gc.CHUNK_IDS}")
            _same(ix.bruteforce_knn_grouped(Q, k, allow=rows, group_of_query=g, max_list_ids=gc.CHUNK_IDS), want,
                  f"k={k} bitmap rows, max_list_ids={gc.CHUNK_IDS}")
            _same(by_label, _twin(ix, Q, k, g, lambda q, e: ix.bruteforce_knn_labeled(q, k, ("range", tuple(table[e].tolist())))),
                  f"k={k} labels: twin")
            _same(by_rows, _twin(ix, Q, k, g, lambda q, e: ix.bruteforce_knn_masked(q, k, rows[e])), f"k={k} bitmap rows: twin")
    finally:
        ix.close()


def test_gt_pieces_is_honoured_and_changes_nothing(oracle):
    tname, metric, d, k = "f16", "l2", 128, 10
    X, Q = gc.data(tname, d)
    ix = DeviceIndex(X, max_degree=4, metric=metric)
    try:
        ix.set_labels(gc.labels())
        ix.set_option("gt_pieces", 3)
        _same(ix.bruteforce_knn_grouped(Q, k, where=("range", gc.table(k)), group_of_query=gc.group_of_query()),
              gc.reference(oracle, tname, metric, d, k), "gt_pieces = 3")
    finally:
        ix.close()


@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["f16", "f32"])
def test_real_valued_rows_equal_the_twin(dtype):
    """default float mode on real-valued data: not exact against the oracle, but the same bits as the shared route"""
    rng = np.random.default_rng(17)
    d, k = 100, 10
    X = rng.standard_normal((gc.N, d)).astype(dtype)
    Q = rng.standard_normal((gc.NQ, d)).astype(dtype)
    lab, g, table = gc.labels(), gc.group_of_query(), gc.table(k)
    ix = DeviceIndex(X, max_degree=4, metric="l2")
    try:
        ix.set_labels(lab)
        got = ix.bruteforce_knn_grouped(Q, k, where=("range", table), group_of_query=g)
        _same(got, _twin(ix, Q, k, g, lambda q, e: ix.bruteforce_knn_labeled(q, k, ("range", tuple(table[e].tolist())))), "twin")
        _same(ix.bruteforce_knn_grouped(Q, k, allow=gc.bitmap_rows(lab, k), group_of_query=g, max_list_ids=gc.CHUNK_IDS), got, "rows, chunks")
        assert len(np.unique(got[1][np.isfinite(got[1])])) > 500                # real-valued distances, not a grid of integers
    finally:
        ix.close()


@pytest.mark.parametrize("form", ["labels", "rows"])
def test_dev_entries_behind_a_busy_stream(oracle, form):
    """inputs arrive after the delay, outputs are poisoned after it; the call synchronises, so only the results are asserted"""
    import torch
    tname, metric, d, k = "i8", "mips", 100, 10
    lib = _capi.load()
    X, Q = gc.data(tname, d)
    lab, g = gc.labels(), gc.group_of_query()
    want = gc.reference(oracle, tname, metric, d, k)
    filt = gc.table(k).view(np.int32) if form == "labels" else gc.bitmap_rows(lab, k).view(np.int32)
    ix = DeviceIndex(X, max_degree=4, metric=metric)
    try:
        ix.set_labels(lab)
        dev = torch.device("cuda", 0)
        real = [torch.from_numpy(Q).to(dev), torch.from_numpy(filt).to(dev), torch.from_numpy(g.view(np.int32)).to(dev)]
        decoy_g = torch.from_numpy(np.roll(g, 7).view(np.int32)).to(dev)        # decoys: valid inputs, other answers
        bufs = [torch.from_numpy(np.ascontiguousarray(Q[::-1])).to(dev), torch.zeros_like(real[1]), decoy_g]
        o_ids = torch.zeros((gc.NQ, k), dtype=torch.int32, device=dev); o_d = torch.zeros((gc.NQ, k), dtype=torch.float32, device=dev)
        o_c = torch.zeros(gc.NQ, dtype=torch.int32, device=dev)
        stream = torch.cuda.Stream(device=dev)
        vp = lambda t: C.c_void_p(t.data_ptr())
        sp = C.c_void_p(stream.cuda_stream)

        def call():
            if form == "labels":
                _capi.check(lib.pann_bruteforce_knn_labeled_grouped_dev(ix.handle, vp(bufs[0]), gc.NQ, d, k, _capi.PANN_PRED_RANGE, vp(bufs[1]),
                                                                        len(filt), vp(bufs[2]), 0, vp(o_ids), vp(o_d), vp(o_c), sp))
            else:
                _capi.check(lib.pann_bruteforce_knn_masked_grouped_dev(ix.handle, vp(bufs[0]), gc.NQ, d, k, vp(bufs[1]), len(filt),
                                                                       filt.shape[1], vp(bufs[2]), 0, vp(o_ids), vp(o_d), vp(o_c), sp))
        stream_order.run_behind_delay(stream, list(zip(bufs, real)), [o_ids, o_d, o_c], [call])
        _same((o_ids.cpu().numpy(), o_d.cpu().numpy(), o_c.cpu().numpy()), want, f"dev {form}")
    finally:
        ix.close()


def test_refusals():
    import torch
    lib = _capi.load()
    d, k = 128, 10
    X, Q = gc.data("u8", d)
    lab, g, table = gc.labels(), gc.group_of_query(), gc.table(10)
    G = len(table)
    ix = DeviceIndex(X, max_degree=4)
    u4 = DeviceIndex.from_packed(X[:, :64] & 0x77, 128, "u4", max_degree=4)
    try:
        ix.set_labels(lab); u4.set_labels(lab)
        BAD, UNS = _capi.PANN_ERR_BAD_ARG, _capi.PANN_ERR_UNSUPPORTED

        def code(fn):
            with pytest.raises(PannError) as e:
                fn()
            assert str(e.value)
            return e.value.code
        # an index >= npreds on the device entries: reported after the call's synchronisation, poisoned outputs untouched
        bad_g = g.copy(); bad_g[77] = G
        dev = torch.device("cuda", 0)
        t_q, t_p, t_g = torch.from_numpy(Q).to(dev), torch.from_numpy(table.view(np.int32)).to(dev), torch.from_numpy(bad_g.view(np.int32)).to(dev)
        t_rows = torch.from_numpy(gc.bitmap_rows(lab, 10).view(np.int32)).to(dev)
        outs = [torch.zeros((gc.NQ, k), dtype=torch.int32, device=dev), torch.zeros((gc.NQ, k), dtype=torch.float32, device=dev),
                torch.zeros(gc.NQ, dtype=torch.int32, device=dev)]
        for o in outs:
            stream_order.poison(o)
        torch.cuda.synchronize()
        vp = lambda t: C.c_void_p(t.data_ptr())
        assert lib.pann_bruteforce_knn_labeled_grouped_dev(ix.handle, vp(t_q), gc.NQ, d, k, _capi.PANN_PRED_RANGE, vp(t_p), G, vp(t_g), 0,
                                                           vp(outs[0]), vp(outs[1]), vp(outs[2]), None) == BAD
        assert b"out of range" in lib.pann_last_error()
        assert lib.pann_bruteforce_knn_masked_grouped_dev(ix.handle, vp(t_q), gc.NQ, d, k, vp(t_rows), G, t_rows.shape[1], vp(t_g), 0,
                                                          vp(outs[0]), vp(outs[1]), vp(outs[2]), None) == BAD
        torch.cuda.synchronize()
        for o in outs:
            assert (o.cpu().numpy().view(np.uint8) == stream_order.POISON_BYTE).all()
        # ... and on the host entries, checked on the host
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        h_ids = np.full((gc.NQ, k), 7, np.uint32); h_d = np.full((gc.NQ, k), 7, np.float32); h_c = np.full(gc.NQ, 7, np.uint32)
        assert lib.pann_bruteforce_knn_labeled_grouped(ix.handle, p(Q), gc.NQ, d, k, _capi.PANN_PRED_RANGE, p(table), G, p(bad_g), 0,
                                                       p(h_ids), p(h_d), p(h_c)) == BAD
        assert (h_ids == 7).all() and (h_d == 7).all() and (h_c == 7).all()
        with pytest.raises(ValueError):
            ix.bruteforce_knn_grouped(Q, k, where=("range", table), group_of_query=bad_g)
        # what the twins refuse keeps its code
        assert code(lambda: ix.bruteforce_knn_grouped(Q, 129, where=("range", table), group_of_query=g)) == UNS
        assert code(lambda: ix.bruteforce_knn_grouped(Q, 129, allow=gc.bitmap_rows(lab, 10), group_of_query=g)) == UNS
        assert code(lambda: ix.bruteforce_knn_grouped(Q, 0, where=("range", table), group_of_query=g)) == BAD
        assert code(lambda: ix.bruteforce_knn_grouped(Q, k, where=(5, table), group_of_query=g)) == BAD           # unknown kind
        Q4 = np.ascontiguousarray(Q[:, :64] & 0x77)
        assert code(lambda: u4.bruteforce_knn_grouped(Q4, k, where=("range", table), group_of_query=g)) == UNS   # a four-bit handle
        assert lib.pann_bruteforce_knn_labeled_grouped(ix.handle, p(Q), gc.NQ, d, k, _capi.PANN_PRED_RANGE, p(table), 0, p(g), 0,
                                                       p(h_ids), p(h_d), p(h_c)) == BAD                              # an empty table
        assert lib.pann_bruteforce_knn_masked_grouped(ix.handle, p(Q), gc.NQ, d, k, p(gc.bitmap_rows(lab, 10)), G, 5, p(g), 0,
                                                      p(h_ids), p(h_d), p(h_c)) == BAD                               # a short stride
        assert lib.pann_bruteforce_knn_labeled_grouped(ix.handle, p(Q), 0, d, k, _capi.PANN_PRED_RANGE, p(table), G, p(g), 0,
                                                       p(h_ids), p(h_d), p(h_c)) == _capi.PANN_OK                    # nq == 0
        assert (h_ids == 7).all()
        ix.drop_labels()
        assert code(lambda: ix.bruteforce_knn_grouped(Q, k, where=("range", table), group_of_query=g)) == BAD     # no labels
        ids, _, cnt = ix.bruteforce_knn_grouped(Q, k, allow=gc.bitmap_rows(lab, 10), group_of_query=g)             # bitmaps need none
        assert (cnt == np.minimum(10, np.array([gc.wanted_counts(10)[gc.ENTRIES[e]] for e in g]))).all()
    finally:
        ix.close(); u4.close()


def test_python_dedup_form_equals_the_per_query_scan():
    """one predicate per query, few distinct ones: the table is deduplicated in Python; k = 10 is within the scan's reach"""
    tname, metric, d, k = "u8", "l2", 200, 10
    X, Q = gc.data(tname, d)
    lab, g = gc.labels(), gc.group_of_query()
    ix = DeviceIndex(X, max_degree=4, metric=metric)
    try:
        ix.set_labels(lab)
        preds = gc.table(k)[g]                                                  # (NQ, 2): 7 distinct filters among 200
        want = ix.bruteforce_knn_labeled(Q, k, ("range", preds))
        _same(ix.bruteforce_knn_grouped(Q, k, where=("range", preds)), want, "where, dedup")
        rows = label_allow(lab, "range", preds)
        _same(ix.bruteforce_knn_grouped(Q, k, allow=rows), want, "allow, dedup")
        with pytest.raises(ValueError):
            ix.bruteforce_knn_grouped(Q, k, where=("range", preds[:-1]))
        with pytest.raises(ValueError):
            ix.bruteforce_knn_grouped(Q, k, where=("range", preds), allow=rows)
    finally:
        ix.close()


def test_graph_index_exact_grouped(tmp_path):
    import label_cases as lc
    import masked_cases as mc
    from parlayann_amd import io
    from parlayann_amd.graph_index import FloatEuclidianIndex
    X, Q, _, _ = mc.layout_data("f32")
    io.write_bin(tmp_path / "b.bin", X)
    io.write_graph(tmp_path / "g.graph", mc.graph(32))
    labels, kind, preds, _ = lc.CASES["tenant"]
    gi = FloatEuclidianIndex(str(tmp_path / "b.bin"), str(tmp_path / "g.graph"), labels=labels)
    try:
        cnt = gi.index.label_count((kind, preds))
        cut = int(np.median(cnt))
        assert (cnt <= cut).any() and (cnt > cut).any()
        rows = label_allow(labels, kind, preds)
        for fn in (gi.batch_search, gi.batch_search_masked):
            for kw in (dict(where=(kind, preds)), dict(allow=rows)):
                a = fn(Q, 10, 64, visit_limit=1000, exact_below=cut, **kw)
                b = fn(Q, 10, 64, visit_limit=1000, exact_below=cut, exact_grouped=True, **kw)
                np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            walked = fn(Q, 10, 64, visit_limit=1000, where=(kind, preds), exact_grouped=True)       # without exact_below: nothing changes
            plain = fn(Q, 10, 64, visit_limit=1000, where=(kind, preds))
            np.testing.assert_array_equal(walked[0], plain[0])
    finally:
        gi.index.close()
        if gi.q_index is not None:
            gi.q_index.close()
