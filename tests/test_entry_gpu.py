"""Entry points on the device (DESIGN.md "Entry points"): the medoids of a table of filters, and the grouped labeled search that
starts every query at its own filter's row of starts.

    bit equality    filter_medoids equals tests/entry_ref.py in ids, dists, counts and centroids (the rows of the default float mode:
                    the grouped twin's bits and the oracle within a derived bound, see _oracle_bits): five element types (two with
                    a row stride beyond d elements), f32 also in exact-float-order mode, per_filter 1 / 10 / 128, the label table
                    and the bitmap table, allow=None, max_list_ids = 3000, fill_id 0 and 0xFFFFFFFF, and a table whose windows
                    hold exactly 1, P - 1, P, P + 1 and 3 P + 7 points (tests/entry_cases.py)
    real values     standard-normal f16 / f32 rows: every centroid coordinate within the derived bound of the exact mean, the
                    ids / dists rows equal bruteforce_knn_grouped on the converted centroids, two calls give the same bits
    grouped search  batch_search_grouped equals entry_ref.grouped_search_ref field for field and its twin called once per group
    _dev entries    behind a busy stream (tests/stream_order.py); a table index >= G gives padding and PANN_STATUS_BAD_GROUP
    refusals        leave poisoned outputs untouched
    Python          medoid(consider=) after a delete batch; GraphIndex.batch_search(entry="medoid")
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import entry_cases as ec
import entry_ref
import grouped_knn_cases as gc
import masked_knn_cases as kc
import steered_cases as sc
import stream_order
from parlayann_amd import DeviceIndex, PannError, _capi, allow_bitmap
from parlayann_amd.index import label_allow

pytestmark = pytest.mark.gpu

FIELDS = ("ids", "dists", "counts", "centroids")


def _same(got, want, msg, fields=FIELDS):
    for f in fields:
        np.testing.assert_array_equal(np.asarray(got[f]).view(np.uint32), np.asarray(want[f]).view(np.uint32), err_msg=f"{msg}: {f}")


def _oracle_bits(tname, exact):
    """Does the device's distance equal the oracle's bit for bit when the QUERY is a centroid?  A centroid is not integer-valued.
    Converted to u8 / i8 it is an integer again and every sum is exact; in exact-float-order mode the device adds in the oracle's
    order.  In the default float mode the device adds in its own order (DESIGN.md "Float summation order"), and with a fractional
    query row the f32 sums are no longer exact -- the existing exact-route tests meet the oracle there only because their queries are
    integer-valued.  For those configurations the rows are held bit for bit against what THE RULE names, the grouped twin on the
    device, and against the oracle within the bound of _float_eps."""
    return exact or tname in ("u8", "i8")


def _float_eps(tname, metric, d, dists, q_norm2, a_norm2_max):
    """|device - oracle| for one distance of d terms, both sides in f32 (u = 2^-24), as the sum of each side's bound against the exact
    value.  The bounds are the project's own, derived in DESIGN.md "Float summation order" and asserted against float64 by
    tests/test_fast_float_gpu.py; which one holds follows from the form the code computes:
      oracle   the difference form in sequence: a term fl(fl(q - a)^2) carries 2 d1 + d2 <= 3 u, the d - 1 additions one rounding
               each, (d + 2) u |dist| to first order; (d + 3) u |dist| leaves the second-order terms their room.
      device   the dense route (dense.hip).  f32 rows: the difference form with an fma per term, the same bound.  f16 / bf16 rows under
               L2: the NORM form |a|^2 + |q|^2 - 2 a.q on the matrix cores, three f32 sums rounded on their own, whose error scales
               with the norms and not with the distance: (d + 3) u (|a|^2 + |q|^2 + 2 sum |a_i q_i|) <= (d + 3) u (|a| + |q|)^2 by
               Cauchy-Schwarz; |a| is taken as the largest norm among the filter's rows, so that ONE eps holds for every candidate of
               a list (the order-statistic argument of _within_the_bound needs that).  MIPS: the products of two bf16 values are exact in
               f32, the sum adds at most d - 1 roundings: (d + 1) u sum |a_i q_i|, and on non-negative data sum |a_i q_i| = |dist|.
    dists (G, E): the oracle's; q_norm2, a_norm2_max (G,): |q|^2 of the query row and the largest |a|^2 of the entry's allowed rows."""
    u, wd = 2.0 ** -24, np.abs(np.asarray(dists, np.float64))
    if metric == "mips":
        return 2.0 * (d + 1) * u * wd
    if tname == "f32":
        return 2.0 * (d + 3) * u * wd
    both = (np.sqrt(np.asarray(a_norm2_max, np.float64)) + np.sqrt(np.asarray(q_norm2, np.float64))) ** 2
    return (d + 3) * u * (both[:, None] + wd)


def _within_the_bound(got, want, eps, next_dist, msg):
    """dists within eps of the oracle's (an order statistic of distances that each moved by at most eps moves by at most eps); ids equal
    except inside a near tie: where the oracle's neighbouring distances lie within 2 eps of each other.  The neighbour of the last slot
    is the first point left out: next_dist(g) is the oracle's distance of rank E + 1 under filter g (+inf if there is none)."""
    gd, wd = np.asarray(got["dists"], np.float64), np.asarray(want["dists"], np.float64)
    fin = np.isfinite(wd)
    assert np.array_equal(fin, np.isfinite(gd)), msg
    worst = float(np.max(np.abs(gd[fin] - wd[fin]) / np.maximum(eps[fin], 1e-300))) if fin.any() else 0.0
    print(f"{msg}: largest |device - oracle| / bound = {worst:.3g}")
    assert (np.abs(gd[fin] - wd[fin]) <= eps[fin]).all(), f"{msg}: dists"
    E = wd.shape[1]
    for g, j in np.argwhere(np.asarray(got["ids"]) != np.asarray(want["ids"])):
        near = [abs(wd[g, j] - wd[g, i]) for i in (j - 1, j + 1) if 0 <= i < E and fin[g, i]]
        if j == E - 1:
            near.append(abs(wd[g, j] - next_dist(int(g))))
        assert fin[g, j] and near and min(near) <= 2 * eps[g, j], f"{msg}: ids differ outside a near tie at {(g, j)}"


# ---- filter medoids ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tname,metric,d,exact", ec.GRID, ids=ec.GRID_IDS)
def test_filter_medoids_equal_the_reference(oracle, tname, metric, d, exact):
    X, _ = gc.data(tname, d)
    ix = DeviceIndex(X, max_degree=4, metric=metric, exact_float_order=exact)
    try:
        ix.set_labels(gc.labels())
        assert ix.get_option("centroid_piece_ids") == ec.P
        with pytest.raises(PannError) as e:
            ix.set_option("centroid_piece_ids", 64)                              # a compile-time constant
        assert e.value.code == _capi.PANN_ERR_BAD_ARG
        bits = _oracle_bits(tname, exact)
        if not bits and metric == "mips":
            assert (entry_ref.widen(X) >= 0).all()                               # _float_eps: sum |a_i q_i| = |dist|
        for E in ec.PER_FILTER:
            for which in ("groups", "pieces"):
                want = ec.reference(oracle, tname, metric, d, which, E)
                where, rows = ("range", ec.table(which, E)), ec.bitmap_rows(which, E)
                got = ix.filter_medoids(where=where, per_filter=E, centroids=True)
                if bits:
                    _same(got, want, f"E={E} {which} labels")
                else:                                                            # centroids and counts by bits; rows: the twin's bits, the oracle's bound
                    _same(got, want, f"E={E} {which} labels", ("counts", "centroids"))
                    q = np.ascontiguousarray(entry_ref.convert(want["centroids"], X.dtype))
                    ids, dists, counts = ix.bruteforce_knn_grouped(q, E, where=where, group_of_query=np.arange(len(q)))
                    _same(got, {"ids": ids, "dists": dists, "counts": counts}, f"E={E} {which} labels: the grouped twin", FIELDS[:3])
                    A, W = ec.allow_rows(which, E), entry_ref.widen(X)
                    n2 = (W * W).sum(axis=1)
                    eps = _float_eps(tname, metric, d, want["dists"], (entry_ref.widen(q) ** 2).sum(axis=1),
                                     [n2[a].max() if a.any() else 0.0 for a in A])

                    def next_dist(g, E=E, A=A, q=q):      # the oracle's distance of rank E + 1 under filter g
                        if A[g].sum() <= E:
                            return np.inf
                        return float(kc.reference(oracle, X, np.ascontiguousarray(q[g:g + 1]), A[g], E + 1, metric)[1][0, E])
                    _within_the_bound(got, want, eps, next_dist, f"{tname}-{metric} E={E} {which}")
                    want = got
                _same(ix.filter_medoids(allow=rows, per_filter=E, centroids=True), want, f"E={E} {which} bitmap rows")
                _same(ix.filter_medoids(where=where, per_filter=E, centroids=True, max_list_ids=gc.CHUNK_IDS, fill_id=0), ec.with_fill(want, 0),
                      f"E={E} {which} labels, max_list_ids={gc.CHUNK_IDS}, fill_id=0")
                _same(ix.filter_medoids(allow=rows, per_filter=E, max_list_ids=gc.CHUNK_IDS), want, f"E={E} {which} rows, chunks", FIELDS[:3])
                if which == "groups":
                    everything = ix.filter_medoids(per_filter=E, centroids=True)     # allow=None: the medoid of the index
                    a = gc.ENTRIES.index("all")
                    for f in FIELDS:
                        np.testing.assert_array_equal(everything[f][0], want[f][a], err_msg=f"allow=None {f}")
                    if E == 1:
                        assert ix.medoid() == int(want["ids"][a, 0])
    finally:
        ix.close()


@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["f16", "f32"])
def test_real_valued_centroids_within_the_bound(dtype):
    """Standard-normal rows: the double sums are not exact, so the centroid is pinned by a bound, not by bits.
    S = the exact sum of the c values of a coordinate, A = the sum of their magnitudes.  Recursive (or any fixed-order, pairwise or
    blocked) summation of c doubles returns S' with |S' - S| <= (c - 1) u A + O(u^2), u = 2^-53; the second-order terms are covered
    by a factor 2: |S' - S| <= 2 (c - 1) u A.  The division by c is one rounding: |q - S' / c| <= u |S' / c|, and |S' / c| <=
    |S / c| + 2 u A, so |q - S / c| <= 2 u A + u |S / c| (+ terms in u^2 A, inside the factor 2) = A 2^-52 + |S / c| 2^-53.  The
    rounding to f32 adds at most 2^-24 |q| <= 2^-24 |S / c| (1 + 2^-52) + 2^-24 A 2^-52, or half the smallest subnormal where q is
    below the normal range.  Together: A 2^-52 + |S / c| (2^-24 + 2^-52) + 2^-149 -- the issue's bound, for any summation order."""
    rng = np.random.default_rng(17)
    d, E = 100, 10
    X = rng.standard_normal((gc.N, d)).astype(dtype)
    table = ec.table("groups", E)
    A = label_allow(gc.labels(), "range", table)
    ix = DeviceIndex(X, max_degree=4, metric="l2")
    try:
        ix.set_labels(gc.labels())
        got = ix.filter_medoids(where=("range", table), per_filter=E, centroids=True)
        worst = Fraction(0)
        for g in range(len(table)):
            rows = X[A[g]]
            if len(rows) == 0:
                assert not got["centroids"][g].any()
                continue
            mean, mag = entry_ref.exact_mean(rows), entry_ref.exact_mean(np.abs(rows))
            for j in range(d):
                Asum = mag[j] * len(rows)
                bound = Asum * Fraction(1, 2 ** 52) + abs(mean[j]) * (Fraction(1, 2 ** 24) + Fraction(1, 2 ** 52)) + Fraction(1, 2 ** 149)
                err = abs(Fraction(float(got["centroids"][g, j])) - mean[j])
                assert err <= bound, (g, j, float(err), float(bound))
                worst = max(worst, err / bound)
        print(f"largest error / bound: {float(worst):.3g}")
        q = np.ascontiguousarray(entry_ref.convert(got["centroids"], X.dtype))
        ids, dists, counts = ix.bruteforce_knn_grouped(q, E, where=("range", table), group_of_query=np.arange(len(table)))
        _same(got, {"ids": ids, "dists": dists, "counts": counts}, "the grouped twin on the converted centroids", FIELDS[:3])
        assert len(np.unique(got["dists"][np.isfinite(got["dists"])])) > 30      # real-valued distances
        again = ix.filter_medoids(where=("range", table), per_filter=E, centroids=True)
        _same(again, got, "the same call again")
        _same(ix.filter_medoids(allow=ec.bitmap_rows("groups", E), per_filter=E, centroids=True), got, "bitmap rows")
    finally:
        ix.close()


@pytest.mark.parametrize("form", ["labels", "rows", "all"])
def test_medoid_dev_entries_behind_a_busy_stream(oracle, form):
    """inputs arrive after the delay, outputs are poisoned after it; the call synchronises once, so only the results are asserted"""
    import torch
    tname, metric, d, E = "i8", "mips", 100, 10
    lib = _capi.load()
    X, _ = gc.data(tname, d)
    lab = gc.labels()
    want = ec.reference(oracle, tname, metric, d, "groups", E)
    if form == "all":
        a = gc.ENTRIES.index("all")
        want = {f: want[f][a:a + 1] for f in FIELDS}
    G = len(want["counts"])
    filt = ec.table("groups", E).view(np.int32) if form == "labels" else ec.bitmap_rows("groups", E).view(np.int32)
    ix = DeviceIndex(X, max_degree=4, metric=metric)
    try:
        ix.set_labels(lab)
        dev = torch.device("cuda", 0)
        real = torch.from_numpy(filt).to(dev)
        buf = torch.zeros_like(real)                                             # the decoy: a valid table that allows other points
        o_ids = torch.zeros((G, E), dtype=torch.int32, device=dev); o_d = torch.zeros((G, E), dtype=torch.float32, device=dev)
        o_c = torch.zeros(G, dtype=torch.int32, device=dev); o_cen = torch.zeros((G, d), dtype=torch.float32, device=dev)
        stream = torch.cuda.Stream(device=dev)
        vp = lambda t: C.c_void_p(t.data_ptr())
        sp = C.c_void_p(stream.cuda_stream)

        def call():
            if form == "labels":
                _capi.check(lib.pann_filter_medoids_labeled_dev(ix.handle, _capi.PANN_PRED_RANGE, vp(buf), G, E, 0xFFFFFFFF, 0, vp(o_ids), vp(o_d),
                                                                vp(o_c), vp(o_cen), sp))
            elif form == "rows":
                _capi.check(lib.pann_filter_medoids_masked_dev(ix.handle, vp(buf), G, filt.shape[1], E, 0xFFFFFFFF, 0, vp(o_ids), vp(o_d), vp(o_c),
                                                               vp(o_cen), sp))
            else:
                _capi.check(lib.pann_filter_medoids_masked_dev(ix.handle, None, 1, 0, E, 0xFFFFFFFF, 0, vp(o_ids), vp(o_d), vp(o_c), vp(o_cen), sp))
        stream_order.run_behind_delay(stream, [] if form == "all" else [(buf, real)], [o_ids, o_d, o_c, o_cen], [call])
        _same({"ids": o_ids.cpu().numpy(), "dists": o_d.cpu().numpy(), "counts": o_c.cpu().numpy(), "centroids": o_cen.cpu().numpy()}, want,
              f"dev {form}")
    finally:
        ix.close()


def test_medoid_refusals():
    lib = _capi.load()
    d, E = 128, 10
    X, _ = gc.data("u8", d)
    lab, table = gc.labels(), ec.table("groups", E)
    G = len(table)
    ix = DeviceIndex(X, max_degree=4)
    u4 = DeviceIndex.from_packed(X[:, :64] & 0x77, 128, "u4", max_degree=4)
    BAD, UNS = _capi.PANN_ERR_BAD_ARG, _capi.PANN_ERR_UNSUPPORTED
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    try:
        ix.set_labels(lab); u4.set_labels(lab)
        rows = ec.bitmap_rows("groups", E)

        def refused(handle, per_filter, labeled=True, npreds=G, stride=None, allow=rows, kind=_capi.PANN_PRED_RANGE):
            w = max(per_filter, 1)
            ids = np.full((G, w), 7, np.uint32); dists = np.full((G, w), 7, np.float32); cnt = np.full(G, 7, np.uint32)
            cen = np.full((G, d), 7, np.float32)
            if labeled:
                rc = lib.pann_filter_medoids_labeled(handle, kind, p(table), npreds, per_filter, 0, 0, p(ids), p(dists), p(cnt), p(cen))
            else:
                rc = lib.pann_filter_medoids_masked(handle, None if allow is None else p(allow), npreds, rows.shape[1] if stride is None else stride,
                                                    per_filter, 0, 0, p(ids), p(dists), p(cnt), p(cen))
            if rc != 0:
                assert lib.pann_last_error()
                assert (ids == 7).all() and (dists == 7).all() and (cnt == 7).all() and (cen == 7).all()      # nothing written
            return rc
        assert refused(ix.handle, E) == 0 and refused(ix.handle, E, labeled=False) == 0      # the valid calls
        for labeled in (True, False):
            assert refused(ix.handle, 0, labeled) == BAD                          # per_filter 0
            assert refused(ix.handle, 129, labeled) == UNS                        # per_filter 129
            assert refused(ix.handle, 128, labeled) == 0
            assert refused(u4.handle, E, labeled) == UNS                          # a four-bit handle
            assert refused(ix.handle, E, labeled, npreds=0) == BAD                # an empty table
        assert refused(ix.handle, E, kind=5) == BAD                               # an unknown kind
        assert refused(ix.handle, E, labeled=False, stride=5) == BAD              # a short stride
        assert refused(ix.handle, E, labeled=False, allow=None) == BAD            # no bitmap with G rows
        assert refused(ix.handle, E, labeled=False, allow=None, npreds=1, stride=0) == 0      # ... with one: every point
        ix.drop_labels()
        assert refused(ix.handle, E) == BAD                                       # no labels
        assert refused(ix.handle, E, labeled=False) == 0                          # bitmaps need none
    finally:
        ix.close(); u4.close()


def test_medoid_after_a_delete_batch(oracle):
    """consider = the live set: the medoid is a live id, and the reference's"""
    X, _, metric = sc.layout_data("u8")
    ix = DeviceIndex(X, sc.graph("u8", 32), metric=metric)
    try:
        before = ix.medoid()
        near, _ = oracle.bruteforce_knn(X, X[before:before + 1], 40)              # delete the medoid and its surroundings
        dead = np.unique(np.concatenate([near[0], np.arange(0, sc.N, 7, dtype=np.uint32)]))
        ix.vamana_delete_batch(dead, 32, 1.2)
        live = np.ones(sc.N, bool); live[dead] = False
        want = int(entry_ref.filter_medoids(oracle, X, live[None, :], 1, metric)["ids"][0, 0])
        for consider in (live, allow_bitmap(sc.N, deleted_ids=dead)):
            got = ix.medoid(consider=consider)
            assert got == want and live[got] and got != before
        with pytest.raises(ValueError):
            ix.medoid(consider=np.zeros(sc.N, bool))
    finally:
        ix.close()


# ---- grouped labeled search ------------------------------------------------------------------------------------------------------

SEARCH_COUNTERS = ("frontier_size", "visited_count", "dist_cmps", "degree_sum", "result_count", "allowed_cmps")
G_TABLE = 8
UNNAMED = 5                                              # the table entry no query names


def _tenant_table(T, kind):
    """(labels, table uint32 (G_TABLE, 2)): entry g is tenant g % max(T, 1) as a predicate of `kind` (steered_cases.labels_of)"""
    lab, preds = sc.labels_of(T, kind, True, nq=G_TABLE)
    return lab, preds


def _group():
    """uint32 (NQ,): interleaved table indices, none of them UNNAMED"""
    g = (np.arange(sc.NQ, dtype=np.uint32) * 3 + 1) % G_TABLE
    g[g == UNNAMED] = 2
    return g


def _starts(lab, kind, table, nstarts, rows):
    """(rows, nstarts) start ids.  Row g holds points entry g allows, except rows 1 and 4, whose first start the entry DISALLOWS;
    with one row the starts are 0, 7, 1999 as in steered_cases."""
    if rows == 1:
        return np.array([0, 7, 1999][:nstarts], np.uint32)
    A = label_allow(lab, kind, table)
    out = np.empty((rows, nstarts), np.uint32)
    for g in range(rows):
        ok, no = np.flatnonzero(A[g]), np.flatnonzero(~A[g])
        out[g] = ok[(11 * g + np.arange(nstarts)) % len(ok)] if len(ok) else no[:nstarts]
        if g in (1, 4) and len(no):
            out[g, 0] = no[17 * g]
    return out


# layout, beam, tenants T, predicate kind, start rows (1 or G), nstarts, steer
SEARCHES = [
    ("f16", 64, 20, "match", G_TABLE, 3, None),
    ("f16", 64, 20, "match", G_TABLE, 3, 16),
    ("f16", 64, 20, "match", G_TABLE, 1, 0),
    ("u8", 100, 2, "range", 1, 1, None),
    ("u8", 100, 2, "any", 1, 3, 16),
    ("f32", 32, 20, "range", G_TABLE, 1, None),
]
SEARCH_IDS = [f"{l}-b{b}-T{t}-{k}-rows{r}-starts{s}-steer{f}" for l, b, t, k, r, s, f in SEARCHES]
_handles = {}


def _index(layout):
    if layout not in _handles:
        X, _, metric = sc.layout_data(layout)
        _handles[layout] = DeviceIndex(X, sc.graph(layout, 32), metric=metric)
    return _handles[layout]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for ix in _handles.values():
        ix.close()
    _handles.clear()


def _same_search(ref, got, steer, what):
    assert got["status"][0] == 0
    np.testing.assert_array_equal(ref["ids"], got["ids"], err_msg=what + " ids")
    np.testing.assert_array_equal(np.asarray(ref["dists"]).view(np.uint32), got["dists"].view(np.uint32), err_msg=what + " dists")
    for f in SEARCH_COUNTERS + (entry_ref.STEER_FIELDS if steer is not None else ()):
        np.testing.assert_array_equal(ref[f], got[f], err_msg=what + " " + f)
    for i in range(len(ref["ids"])):
        nv = int(ref["visited_count"][i])
        np.testing.assert_array_equal(ref["visited_ids"][i, :nv], got["visited_ids"][i, :nv], err_msg=what + " visited_ids")
        np.testing.assert_array_equal(ref["visited_dists"][i, :nv], got["visited_dists"][i, :nv], err_msg=what + " visited_dists")


@pytest.mark.parametrize("layout,beam,T,kind,rows,nstarts,steer", SEARCHES, ids=SEARCH_IDS)
def test_grouped_search_equals_the_restatement_and_the_twin(layout, beam, T, kind, rows, nstarts, steer):
    X, Q, metric = sc.layout_data(layout)
    lab, table = _tenant_table(T, kind)
    group = _group()
    assert UNNAMED not in group and len(np.unique(group)) == G_TABLE - 1 and (np.diff(group.astype(int)) != 0).any()
    starts = _starts(lab, kind, table, nstarts, rows)
    kw = dict(k=10, beam=beam, out_k=10, cut=1.35, visited_cap=2048)
    ref = entry_ref.grouped_search_ref(X, sc.graph(layout, 32), lab, kind, table, group, starts, steer=steer, queries=Q, metric=metric, **kw)
    if rows > 1:
        A = label_allow(lab, kind, table)
        assert not A[1, starts[1, 0]] and not A[4, starts[4, 0]] and A[2, starts[2]].all()      # two rows start outside their filter
        q1 = np.flatnonzero(group == 1)
        assert (ref["dist_cmps"][q1] >= ref["allowed_cmps"][q1] + 1).all()          # the disallowed start got a distance, and is no result
        assert not (ref["ids"][q1] == starts[1, 0]).any()
    ix = _index(layout)
    ix.set_labels(lab)
    try:
        got = ix.batch_search_grouped(Q, where=(kind, table), group_of_query=group, starts=starts, steer=steer, **kw)
        assert ("bridge_rows" in got) == (steer is not None)
        _same_search(ref, got, steer, "restatement")
        for g in np.unique(group):                                               # the twin, once per group, on the device
            sel = np.flatnonzero(group == g)
            twin = ix.batch_search_labeled(np.ascontiguousarray(Q[sel]), where=(kind, tuple(int(v) for v in table[g])),
                                           starts=starts if rows == 1 else starts[g], steer=steer, **kw)
            for f in ("ids", "dists") + SEARCH_COUNTERS + (entry_ref.STEER_FIELDS if steer is not None else ()):
                np.testing.assert_array_equal(twin[f], got[f][sel], err_msg=f"twin of entry {g}: {f}")
            for i, q in enumerate(sel):                                          # the visited lists, as far as they are written
                nv = int(twin["visited_count"][i])
                np.testing.assert_array_equal(twin["visited_ids"][i, :nv], got["visited_ids"][q, :nv], err_msg=f"twin of entry {g}: visited_ids")
                np.testing.assert_array_equal(twin["visited_dists"][i, :nv], got["visited_dists"][q, :nv], err_msg=f"twin of entry {g}: visited_dists")
        by_id = ix.batch_search_grouped(query_ids=sc.QUERY_IDS, where=(kind, table), group_of_query=group, starts=starts, steer=steer, **kw)
        twin = ix.batch_search_labeled(query_ids=sc.QUERY_IDS[group == 2], where=(kind, tuple(int(v) for v in table[2])),
                                       starts=starts if rows == 1 else starts[2], steer=steer, **kw)
        np.testing.assert_array_equal(twin["ids"], by_id["ids"][group == 2])
        found = got["ids"] != 0xFFFFFFFF
        A = label_allow(lab, kind, table)
        assert A[group[np.nonzero(found)[0]], got["ids"][found]].all()            # hard: only points the query's own filter allows
    finally:
        ix.drop_labels()


def test_grouped_search_in_growth_slices():
    """More queries than one slice of the dropped-list growth policy (host_staging.h: 2^30 bytes / (dcap * 8): 87 381 queries at the
    1 536 entries this graph needs): the gathered predicates and start rows are sliced with the queries.  Equal to the twin per group."""
    n, nq = 1500, 100_000
    X = np.zeros((n, 8), np.float32); X[:, 0] = np.arange(n)
    G = np.zeros((n, 5), np.uint32)
    for i in range(n):
        nb = [j for j in (i - 2, i - 1, i + 1, i + 2) if 0 <= j < n]
        G[i, 0] = len(nb); G[i, 1:1 + len(nb)] = nb
    rng = np.random.default_rng(3)
    Q = np.zeros((nq, 8), np.float32); Q[:, 0] = rng.integers(0, n, nq) + 0.25
    Q[7, 0] = n - 1.0; Q[nq - 3, 0] = 0.0                                         # walks of the whole line, from either end
    lab = (np.arange(n) % 3).astype(np.uint32)
    table = np.array([[0, 1], [2, 2]], np.uint32)                               # RANGE: labels 0..1, label 2
    group = (rng.random(nq) < 0.5).astype(np.uint32)
    group[7], group[nq - 3] = 0, 1
    starts = np.array([[0], [n - 1]], np.uint32)
    kw = dict(k=1, beam=16, cut=1.0, out_k=2)
    ix = DeviceIndex(X, G)
    try:
        ix.set_labels(lab)
        got = ix.batch_search_grouped(Q, where=("range", table), group_of_query=group, starts=starts, **kw)
        assert got["status"][0] == 0 and 256 < ix.dropped_capacity <= 2048 and got["visited_count"].max() > 600
        for g in (0, 1):
            sel = np.flatnonzero(group == g)
            twin = ix.batch_search_labeled(np.ascontiguousarray(Q[sel]), where=("range", tuple(int(v) for v in table[g])), starts=starts[g], **kw)
            for f in ("ids", "dists") + SEARCH_COUNTERS:
                np.testing.assert_array_equal(twin[f], got[f][sel], err_msg=f"entry {g}: {f}")
    finally:
        ix.close()


def _dev_search(lib, ix, t, nq, d_stride, nstarts, start_rows, qp, kind, G, steer, fill, stream):
    """pann_batch_search_grouped_labeled_dev on the tensors of dict t"""
    vp = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    out = _capi.SearchOut(ids=vp(t["ids"]), dists=vp(t["dists"]), out_k=t["ids"].shape[1], frontier_size=vp(t["frontier_size"]),
                          visited_count=vp(t["visited_count"]), dist_cmps=vp(t["dist_cmps"]), degree_sum=vp(t["degree_sum"]), status=vp(t["status"]))
    return lib.pann_batch_search_grouped_labeled_dev(ix.handle, vp(t["q"]), None, nq, d_stride, vp(t["starts"]), nstarts, start_rows, C.byref(qp),
                                                     kind, vp(t["table"]), G, vp(t["group"]), C.byref(out), vp(t["result_count"]),
                                                     vp(t["allowed_cmps"]), 1 if steer else 0, fill, vp(t.get("steer")), stream)


@pytest.mark.parametrize("steer", [None, 16], ids=["masked", "steered"])
def test_grouped_search_dev_behind_a_busy_stream_and_a_bad_index(steer):
    import torch
    layout, beam, T, kind, nstarts = "f16", 64, 20, "match", 3
    lib = _capi.load()
    X, Q, metric = sc.layout_data(layout)
    lab, table = _tenant_table(T, kind)
    group = _group()
    starts = _starts(lab, kind, table, nstarts, G_TABLE)
    kw = dict(k=10, beam=beam, out_k=10, cut=1.35)
    ix = _index(layout)
    ix.set_labels(lab)
    try:
        want = ix.batch_search_grouped(Q, where=(kind, table), group_of_query=group, starts=starts, steer=steer, **kw)
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(dev)
        real = {"q": up(Q), "table": up(table), "group": up(group), "starts": up(starts)}
        # decoys: valid inputs, other answers
        decoy = {"q": up(Q[::-1]), "table": torch.zeros_like(real["table"]), "group": up(np.roll(group, 5)), "starts": torch.zeros_like(real["starts"])}
        t = {k_: v.clone() for k_, v in decoy.items()}
        for f in ("frontier_size", "visited_count", "dist_cmps", "degree_sum", "result_count", "allowed_cmps"):
            t[f] = torch.zeros(sc.NQ, dtype=torch.int32, device=dev)
        t["ids"] = torch.zeros((sc.NQ, 10), dtype=torch.int32, device=dev); t["dists"] = torch.zeros((sc.NQ, 10), dtype=torch.float32, device=dev)
        t["status"] = torch.zeros(1, dtype=torch.int32, device=dev); t["steer"] = torch.zeros((sc.NQ, 2), dtype=torch.int32, device=dev)
        outs = [t[f] for f in ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum", "result_count", "allowed_cmps", "status")]
        if steer is not None:
            outs.append(t["steer"])
        stream = torch.cuda.Stream(device=dev)
        sp = C.c_void_p(stream.cuda_stream)
        qp = _capi.QueryParams(k=10, beam=beam, cut=1.35, limit=sc.N, degree_limit=32, rerank_factor=100, pad=1.0)
        call = lambda: _capi.check(_dev_search(lib, ix, t, sc.NQ, Q.strides[0], nstarts, G_TABLE, qp, _capi.PANN_PRED_MATCH, G_TABLE, steer,
                                               steer or 0, sp))
        with torch.cuda.stream(stream):                                          # the first call grows the scratch: not timed
            for k_, v in real.items():
                t[k_].copy_(v)
        call()
        stream.synchronize()
        for k_ in real:
            t[k_].copy_(decoy[k_])
        early = stream_order.run_behind_delay(stream, [(t[k_], real[k_]) for k_ in real], outs, [call])
        assert early                                                              # nothing is synchronised
        host = {f: t[f].cpu().numpy() for f in ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum", "result_count",
                                                "allowed_cmps", "status")}
        assert host["status"][0] == 0
        for f in ("ids", "dists") + SEARCH_COUNTERS:
            np.testing.assert_array_equal(host[f].view(np.uint32), want[f].view(np.uint32), err_msg=f"dev {f}")
        if steer is not None:
            counters = t["steer"].cpu().numpy().view(np.uint32)
            np.testing.assert_array_equal(counters[:, 0], want["bridge_rows"]); np.testing.assert_array_equal(counters[:, 1], want["hop2_cmps"])
        # a table index >= G: padding, count 0, the status bit, and every other row as before
        bad = group.copy(); bad[9] = G_TABLE; bad[40] = 0xFFFFFFFF
        t["group"].copy_(up(bad))
        for o in outs:
            stream_order.poison(o)
        torch.cuda.synchronize()
        call()
        stream.synchronize()
        ids, cnt, status = t["ids"].cpu().numpy().view(np.uint32), t["result_count"].cpu().numpy(), t["status"].cpu().numpy().view(np.uint32)
        assert status[0] == _capi.PANN_STATUS_BAD_GROUP
        good = np.ones(sc.NQ, bool); good[[9, 40]] = False
        assert (ids[~good] == 0xFFFFFFFF).all() and (cnt[~good] == 0).all() and np.isinf(t["dists"].cpu().numpy()[~good]).all()
        np.testing.assert_array_equal(ids[good], want["ids"][good]); np.testing.assert_array_equal(cnt[good], want["result_count"][good].view(np.int32))
        np.testing.assert_array_equal(t["dist_cmps"].cpu().numpy()[good].view(np.uint32), want["dist_cmps"][good])
    finally:
        ix.drop_labels()


def test_grouped_search_refusals():
    lib = _capi.load()
    layout, kind = "u8", "match"
    X, Q, _ = sc.layout_data(layout)
    lab, table = _tenant_table(20, kind)
    group = _group()
    starts = _starts(lab, kind, table, 2, G_TABLE)
    ix = _index(layout)
    BAD, UNS = _capi.PANN_ERR_BAD_ARG, _capi.PANN_ERR_UNSUPPORTED
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    qp = _capi.QueryParams(k=10, beam=64, cut=1.35, limit=sc.N, degree_limit=32, rerank_factor=100, pad=1.0)
    POISON = 0xA5A5A5A5

    def refused(out_k=10, beam=64, start_rows=G_TABLE, group=group, starts=starts, npreds=G_TABLE, kind_code=_capi.PANN_PRED_MATCH, steer=0):
        qp.beam = beam
        ids = np.full((sc.NQ, out_k), POISON, np.uint32); rc_ = np.full(sc.NQ, POISON, np.uint32); ac = np.full(sc.NQ, POISON, np.uint32)
        st = np.full((sc.NQ, 2), POISON, np.uint32)
        out = _capi.SearchOut(ids=p(ids), out_k=out_k)
        rc = lib.pann_batch_search_grouped_labeled(ix.handle, p(Q), None, sc.NQ, Q.strides[0], p(starts), 2, start_rows, C.byref(qp), kind_code,
                                                   p(table), npreds, p(group), C.byref(out), p(rc_), p(ac), steer, 8, p(st))
        if rc != 0:
            assert lib.pann_last_error()
            assert (ids == POISON).all() and (rc_ == POISON).all() and (ac == POISON).all() and (st == POISON).all()
        return rc
    assert refused() == BAD                                                       # no labels yet
    ix.set_labels(lab)
    try:
        assert refused() == 0 and refused(steer=1) == 0                           # the valid calls
        assert refused(start_rows=2) == BAD                                       # start_rows not in {1, G}
        assert refused(start_rows=1) == 0
        bad_g = group.copy(); bad_g[33] = G_TABLE
        assert refused(group=bad_g) == BAD and b"out of range" in lib.pann_last_error()       # a host table index >= G
        bad_s = starts.copy(); bad_s[6, 1] = sc.N
        assert refused(starts=bad_s) == BAD                                       # a host start >= n
        assert refused(group=None) == BAD                                         # a NULL index array
        assert refused(npreds=0) == BAD                                           # an empty table
        assert refused(kind_code=5) == BAD                                        # an unknown kind
        assert refused(out_k=65, beam=128) == UNS and refused(out_k=65) == BAD    # what the twin refuses keeps its code
        assert refused(starts=None) == BAD
        with pytest.raises(ValueError):
            ix.batch_search_grouped(Q, where=(kind, table), group_of_query=bad_g, starts=starts)
        with pytest.raises(ValueError):
            ix.batch_search_grouped(Q, where=(kind, table), group_of_query=group, starts=starts[:3])
        out = _capi.SearchOut(ids=None, out_k=10)
        qp.beam = 64                                                              # the device entry checks before it launches anything
        assert lib.pann_batch_search_grouped_labeled_dev(ix.handle, None, None, sc.NQ, 32, None, 1, 1, C.byref(qp), _capi.PANN_PRED_MATCH, None,
                                                         G_TABLE, None, C.byref(out), None, None, 0, 0, None, None) == BAD
    finally:
        ix.drop_labels()


def test_graph_index_entry_medoid(tmp_path):
    from parlayann_amd import io
    from parlayann_amd.graph_index import UInt8EuclidianIndex
    X, Q, _ = sc.layout_data("u8")
    io.write_bin(tmp_path / "b.bin", X)
    io.write_graph(tmp_path / "g.graph", sc.graph("u8", 32))
    lab, preds = sc.labels_of(20, "match", True)                                  # one predicate per query, 20 distinct
    gi = UInt8EuclidianIndex(str(tmp_path / "b.bin"), str(tmp_path / "g.graph"), labels=lab)
    try:
        for steer in (None, 8):
            ids, dists = gi.batch_search(Q, 10, 64, visit_limit=1000, where=("match", preds), steer=steer, entry="medoid")
            table, group = np.unique(preds, axis=0, return_inverse=True)         # the composition, by hand
            starts = gi.index.filter_medoids(where=("match", table), per_filter=1, fill_id=0)["ids"]
            A = label_allow(lab, "match", table)
            assert A[np.arange(len(table)), starts[:, 0]].all()                  # every tenant starts at one of its own points
            want = gi.index.batch_search_grouped(Q, where=("match", table), group_of_query=group.reshape(-1), starts=starts, k=10, beam=64,
                                                 limit=1000, degree_limit=32, out_k=10, steer=steer)
            np.testing.assert_array_equal(ids, want["ids"]); np.testing.assert_array_equal(dists, want["dists"])
            plain = gi.batch_search(Q, 10, 64, visit_limit=1000, where=("match", preds), steer=steer)
            none = gi.batch_search(Q, 10, 64, visit_limit=1000, where=("match", preds), steer=steer, entry=None)
            np.testing.assert_array_equal(plain[0], none[0]); np.testing.assert_array_equal(plain[1], none[1])     # entry=None: the call as it was
        shared = gi.batch_search(Q, 10, 64, visit_limit=1000, where=("match", (0xFFF, 3)), entry="medoid")           # one predicate for the batch
        start = gi.index.filter_medoids(where=("match", (0xFFF, 3)), fill_id=0)["ids"][0]
        want = gi.index.batch_search_labeled(Q, where=("match", (0xFFF, 3)), starts=start, k=10, beam=64, limit=1000, degree_limit=32, out_k=10)
        np.testing.assert_array_equal(shared[0], want["ids"])
        for bad in (dict(entry="nearest", where=("match", preds)), dict(entry="medoid"), dict(entry="medoid", where=("match", preds), exact_below=5)):
            with pytest.raises(ValueError):
                gi.batch_search(Q, 10, 64, **bad)
    finally:
        gi.index.close()
        if gi.q_index is not None:
            gi.q_index.close()
