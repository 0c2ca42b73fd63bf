"""Every id-addressed operation on rows past the 4 GiB / 2^32-element line (DESIGN.md "Rows past 4 GiB", tests/high_rows.py).

Each index is created empty on the device (n just above the line) and gets ONE block of 4096 rows that straddles the line; ids
are the real ones.  The references are the CPU oracle and the numpy references on sparse host arrays of the full shape, and every
comparison is exact: an offset product that loses its upper bits reads a zero vector or an empty row and changes an answer for
the rows >= B0.  tests/test_high_rows_cpu.py proves what the block-local references rest on."""
import numpy as np
import pytest

import delete_ref
import filtered_ref
import high_rows as hr
import masked_ref
import reach_ref
from parlayann_amd import DeviceIndex, bfloat16, quantize
from parlayann_amd import sketch as sk
from parlayann_amd._capi import PannError
from parlayann_amd.index import label_allow

pytestmark = pytest.mark.gpu

M = hr.M
CASES = {"A-f16": ("A", np.float16, "l2"), "A-bf16": ("A", bfloat16, "l2"), "B-u8": ("B", np.uint8, "l2"),
         "B-i8": ("B", np.int8, "mips"), "C-f32": ("C", np.float32, "l2")}
AB = ["A-f16", "A-bf16", "B-u8", "B-i8"]
SEARCH_FIELDS = ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum")


def _empty(n, d, dtype, max_degree, metric):
    try:
        return DeviceIndex.empty(n, d, dtype, max_degree, metric=metric)
    except PannError as e:
        stride, gs = (d * np.dtype(dtype).itemsize + 63) // 64 * 64, (max_degree + 15) // 16 * 16
        pytest.fail(f"no empty index of {n} rows: {n * stride} bytes of points and {n * gs * 4} bytes of graph were asked for ({e})")


class Case:
    """one geometry and element type: the sparse host arrays, the oracle's graph of the block, and the device index holding both"""

    def __init__(self, name, oracle):
        self.name = name
        self.geom, dt, self.metric = CASES[name]
        self.dtype = np.dtype(dt)
        g = hr.GEOMS[self.geom]
        self.n, self.d, self.R = g["n"], g["d"], g["max_deg"]
        self.lo, self.b0, self.ids = hr.lo(self.geom), hr.b0(self.geom), hr.block_ids(self.geom)
        self.alpha = hr.ALPHA[self.metric]
        self.Xb = hr.block(self.geom, self.dtype, self.metric)
        self.X = hr.sparse_points(self.geom, self.dtype, self.metric)
        self.G, self.start = hr.block_graph(oracle, self.geom, self.dtype, self.metric)
        self.Gl = hr.block_rows(self.G, self.geom)
        self.Q = hr.queries(self.geom, self.dtype, self.metric)
        self.allow_block = hr.block_allow(self.n, self.ids)
        self.ix = _empty(self.n, self.d, self.dtype, self.R, self.metric)
        self.ix.upload_points(self.lo, self.Xb)
        self.restore_graph(clear=False)

    def restore_graph(self, clear=True):
        if clear:
            self.ix.clear_graph()
        self.ix.update_rows(self.ids, self.G[self.lo:self.lo + M])

    def read_rows(self):
        """the block's graph rows off the device, block-local ids: the whole graph (up to 17 GB) is never downloaded"""
        s = self.ix.subset(allow=self.allow_block, maps=False)
        try:
            assert s.n == M
            return s.get_graph()
        finally:
            s.close()

    def dists(self, Q, ids):
        """float32 (nq, len(ids)): exact distances of query rows to block ids"""
        return hr.dist_matrix(Q, self.Xb[np.asarray(ids, np.int64) - self.lo], self.metric).astype(np.float32)

    def close(self):
        self.ix.close()
        for k in [k for k in hr._cache if k[0] in ("sparse", "graph") and k[1] == self.geom and k[2] == hr.type_name(self.dtype)]:
            del hr._cache[k]                       # the virtual allocations of this case go with its index


@pytest.fixture(scope="module")
def hx(request, oracle):
    """the case named by the parameter: module scoped, so pytest runs the tests of one case together and one index is alive at a time"""
    c = Case(request.param, oracle)
    yield c
    c.close()


def on(*names):
    return pytest.mark.parametrize("hx", list(names), indirect=True)


def _same(got, exp, fields, what=""):
    for f in fields:
        np.testing.assert_array_equal(got[f], exp[f], err_msg=f"{what} {f}")


def _above_and_below(c, ids):
    """the ids of a case really lie on both sides of the line"""
    ids = np.asarray(ids, np.int64)
    assert (ids < c.b0).any() and (ids >= c.b0).any()


# ---- a: points round trip ----

@on(*CASES)
def test_points_round_trip(hx):
    c = hx
    got = c.ix.points(first_row=c.lo, nrows=M)
    assert got.tobytes() == c.Xb.tobytes()
    np.testing.assert_array_equal(c.ix.points(c.b0 - 1, 2).view(np.uint8), np.ascontiguousarray(c.Xb[M // 2 - 1:M // 2 + 1]).view(np.uint8))
    assert not c.ix.points(0, 64).view(np.uint8).any() and not c.ix.points(c.n - 64, 64).view(np.uint8).any()
    assert not c.ix.points(c.lo - 64, 64).view(np.uint8).any()


# ---- b: graph rows ----

@on("A-f16", "B-u8", "C-f32")
def test_graph_read_back_and_degrees(hx):
    c = hx
    np.testing.assert_array_equal(c.read_rows(), c.Gl)
    if c.geom != "C":             # B too (2 x 268 MB cross the bus): at 2^26 rows one wave per row is more than 2^32 work-items
        out_deg, in_deg = c.ix.degrees()
        eo, ei = reach_ref.degrees_ref(c.Gl)
        np.testing.assert_array_equal(out_deg[c.lo:c.lo + M], eo)
        np.testing.assert_array_equal(in_deg[c.lo:c.lo + M], ei)
        assert not out_deg[:c.lo].any() and not out_deg[c.lo + M:].any() and not in_deg[:c.lo].any() and not in_deg[c.lo + M:].any()


@on("A-f16", "B-u8", "B-i8")
def test_sort_neighbors(hx):
    """every row sorted by (distance to its owner, id), vamana/index.h:180-185: one wave per row over ALL n rows"""
    c = hx
    D = hr.dist_matrix(c.Xb, c.Xb, c.metric)
    exp = c.Gl.copy()
    for i in range(M):
        nb = c.Gl[i, 1:1 + c.Gl[i, 0]]
        exp[i, 1:1 + len(nb)] = nb[np.lexsort((nb, D[i, nb]))]
    assert (exp[:M // 2] != c.Gl[:M // 2]).any() and (exp[M // 2:] != c.Gl[M // 2:]).any()      # the build leaves rows unsorted
    try:
        c.ix.vamana_sort_neighbors()
        np.testing.assert_array_equal(c.read_rows(), exp)
    finally:
        c.restore_graph()


# ---- c: beam search ----

@on(*AB)
def test_batch_search(hx, oracle):
    c = hx
    kw = dict(metric=c.metric)
    st = (c.start,)
    o = oracle.batch_search(c.X, c.G, queries=c.Q, k=10, beam=64, starts=st, **kw)
    _above_and_below(c, o["ids"])
    _same(c.ix.batch_search(c.Q, k=10, beam=64, starts=st), o, SEARCH_FIELDS, "beam 64")
    Qbig = hr.queries(c.geom, c.dtype, c.metric, nq=2112)        # more than 2048 queries at beam 65..128: the persistent kernel
    _same(c.ix.batch_search(Qbig, k=10, beam=100, starts=st), oracle.batch_search(c.X, c.G, queries=Qbig, k=10, beam=100, starts=st, **kw),
          SEARCH_FIELDS, "beam 100, 2112 queries")
    many = (c.start, c.lo + 5, c.b0, c.b0 - 1, c.lo + M - 1)
    _same(c.ix.batch_search(c.Q, k=10, beam=64, starts=many), oracle.batch_search(c.X, c.G, queries=c.Q, k=10, beam=64, starts=many, **kw),
          SEARCH_FIELDS, "five starts")
    per = c.ids[np.random.default_rng(3).integers(0, M, (len(c.Q), 3))]
    g = c.ix.batch_search(c.Q, k=10, beam=32, starts=per)
    for i in range(len(c.Q)):                                    # the oracle takes one start set per call
        oi = oracle.batch_search(c.X, c.G, queries=c.Q[i:i + 1], k=10, beam=32, starts=per[i], **kw)
        for f in SEARCH_FIELDS:
            np.testing.assert_array_equal(g[f][i], oi[f][0], err_msg=f"per-query starts, query {i}, {f}")
    qid = c.ids[::9]                                             # builder mode: the query is a base point and skips itself
    for beam in (64, 100):
        _same(c.ix.batch_search(query_ids=qid, k=10, beam=beam, starts=st),
              oracle.batch_search(c.X, c.G, query_ids=qid, k=10, beam=beam, starts=st, **kw), SEARCH_FIELDS, f"builder mode, beam {beam}")


# ---- d: Vamana insertion into the empty device graph ----

@pytest.mark.parametrize("L", [64, 100])
@on("A-f16", "B-u8")
def test_insert_batches(hx, oracle, L):
    """L = 100 at n > 4095 * 4096: the 12-bit filter codes cannot exist and the searches fall back to the id table.  L = 64 ends
    with a second-pass batch of the whole block, large enough to be launched in locality-cell order."""
    c = hx
    assert c.n > 4095 * 4096 and c.n * hr.row_stride(c.geom, c.dtype) >= 1 << 30 and c.n >= 256 * 1024
    start, bs = hr.batches(oracle, c.geom)
    if L == 64:
        bs = bs + [np.concatenate(bs)]
    Go = hr.sparse_graph(c.geom)
    c.ix.clear_graph()
    try:
        for i, b in enumerate(bs):
            so = oracle.vamana_insert_batch(c.X, Go, b, c.R, L, c.alpha, start=start, metric=c.metric)
            sg = c.ix.vamana_insert_batch(b, c.R, L, c.alpha, start=start)
            np.testing.assert_array_equal(c.read_rows(), hr.block_rows(Go, c.geom), err_msg=f"after batch {i} of {len(b)}")
            assert (int(so[0]), int(so[1]), int(so[2])) == (sg.search_dist_cmps, sg.prune_dist_cmps, sg.visited_total), f"batch {i}"
    finally:
        c.restore_graph()


# ---- e: robustPrune and deletion ----

@on(*AB)
def test_robust_prune_batch(hx, oracle):
    c = hx
    rng = np.random.default_rng(0)
    owners = c.ids[rng.integers(0, M, 200)]
    owners[:2] = (c.b0 - 1, c.b0)
    cands, dists = [], []
    for i, p in enumerate(owners):
        cc = c.ids[rng.choice(M, int(rng.integers(0, 200)), replace=False)]
        if i % 7 == 0 and len(cc) > 3:
            cc = np.concatenate([cc, cc[:3], [p]]).astype(np.uint32)         # duplicates and the owner itself
        cands.append(cc)
        dists.append(c.dists(c.Xb[int(p) - c.lo][None, :], cc)[0])
    off = np.concatenate([[0], np.cumsum([len(x) for x in cands])]).astype(np.uint64)
    cid, cd = np.concatenate(cands).astype(np.uint32), np.concatenate(dists).astype(np.float32)
    _above_and_below(c, cid)
    for alpha, R, add, with_d in ((c.alpha, c.R, True, True), (1.0, c.R, True, False), (c.alpha, 8, False, True), (1.35, c.R, False, False)):
        ro, dco = oracle.robust_prune_batch(c.X, c.G, owners, cid, cd if with_d else None, off, alpha, R, add=add, metric=c.metric)
        rg, dcg = c.ix.robust_prune_batch(owners, cid, off, alpha, R, cand_dists=cd if with_d else None, add_out_nbrs=add)
        np.testing.assert_array_equal(rg, ro)
        np.testing.assert_array_equal(dcg, dco)


@on("A-f16", "B-u8")
def test_delete_batch(hx, oracle):
    """tests/delete_ref.py: the candidate lists come from the graph alone, so they are read off the block-local rows and shifted;
    the prune is the oracle's, on the real ids and the sparse arrays"""
    c = hx
    dl = delete_ref.seeded_ids(M, 0.05, 77, keep=(c.start - c.lo,))
    dl[:2] = (M // 2 - 1, M // 2 + 1)                                          # one deleted row on each side of the line
    dl = np.unique(dl)
    inD, owners, cand, off = delete_ref.candidates(c.Gl, dl)
    rows, dc = oracle.robust_prune_batch(c.X, c.G, owners + np.uint32(c.lo), cand + np.uint32(c.lo), None, off, c.alpha, c.R, add=False,
                                         metric=c.metric)
    exp = c.Gl.copy()
    live = np.arange(c.R)[None, :] < rows[:, :1]
    exp[owners] = np.concatenate([rows[:, :1], np.where(live, rows[:, 1:] - np.uint32(c.lo), 0)], axis=1)
    exp[inD] = 0
    try:
        st = c.ix.vamana_delete_batch(dl + np.uint32(c.lo), c.R, c.alpha)
        np.testing.assert_array_equal(c.read_rows(), exp)
        want = dict(deleted=len(dl), affected=len(owners), candidates=int(off[-1]), prune_dist_cmps=int(dc.sum(dtype=np.uint64)))
        assert {k: st[k] for k in want} == want
    finally:
        c.restore_graph()


# ---- f: distances, rerank, leaf kNN, pivot split ----

@on(*CASES)
def test_distances_rerank_leaves_and_pivots(hx, oracle):
    c = hx
    rng = np.random.default_rng(5)
    a, b = c.ids[rng.integers(0, M, 500)], c.ids[rng.integers(0, M, 500)]
    a[:3], b[:3] = (c.b0 - 1, c.b0, c.lo), (c.b0, c.b0 - 1, c.lo + M - 1)
    D = hr.dist_matrix(c.Xb, c.Xb, c.metric)
    pd = c.ix.pair_distances(a, b)
    np.testing.assert_array_equal(pd, D[a.astype(np.int64) - c.lo, b.astype(np.int64) - c.lo].astype(np.float32))
    for i in range(12):                                                      # and the oracle itself on a sample, sparse rows
        assert pd[i] == np.float32(oracle.distance(c.X[a[i]], c.X[b[i]], c.metric))
    ids = c.ids[rng.permutation(M)[:300]]
    QD = hr.dist_matrix(c.Q, c.Xb, c.metric).astype(np.float32)
    np.testing.assert_array_equal(c.ix.query_distances(c.Q, ids), QD[:, ids.astype(np.int64) - c.lo])
    # rerank: exact distances of each query's candidates, sorted by (dist, id)
    cand = np.stack([c.ids[rng.choice(M, 60, replace=False)] for _ in range(len(c.Q))]).astype(np.uint32)
    cnt = rng.integers(12, 61, len(c.Q)).astype(np.uint32)
    gi, gd = c.ix.rerank(c.Q, cand, cnt, 10, resort=True)
    for i in range(len(c.Q)):
        cc = cand[i, :cnt[i]]
        dd = QD[i, cc.astype(np.int64) - c.lo]
        order = np.lexsort((cc, dd))[:10]
        np.testing.assert_array_equal(gi[i], cc[order], err_msg=f"rerank row {i}")
        np.testing.assert_array_equal(gd[i], dd[order])
    # leaves whose members straddle B0
    half = {1000: 500, 65: 32, 64: 32, 11: 5, 2: 1}
    leaves = [np.arange(c.b0 - h, c.b0 - h + s, dtype=np.uint32) for s, h in half.items()]
    leaves[0] = c.ids[np.sort(rng.choice(M, 1000, replace=False))]
    for leaf in leaves:
        _above_and_below(c, leaf)
    off = np.concatenate([[0], np.cumsum([len(x) for x in leaves])]).astype(np.uint64)
    gi, gd = c.ix.leaf_knn_batch(np.concatenate(leaves), off, 10)
    for j, leaf in enumerate(leaves):
        oi, od = oracle.leaf_knn(c.X, leaf, 10, c.metric)
        np.testing.assert_array_equal(gi[int(off[j]):int(off[j + 1])], oi, err_msg=f"leaf of {len(leaf)}")
        np.testing.assert_array_equal(gd[int(off[j]):int(off[j + 1])], od)
    # pivot split: side 0 when d(id, a) <= d(id, b)
    sizes = [700, 64, 1, 130]
    sid = np.concatenate([c.ids[rng.choice(M, s, replace=False)] for s in sizes]).astype(np.uint32)
    soff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    pa = np.array([c.lo + 7, c.b0 - 1, c.b0 + 9, c.b0 + 70], np.uint32)
    pb = np.array([c.b0 + 70, c.b0, c.lo + 1, c.lo + 7], np.uint32)         # the second pair is the duplicate across the line; the last
                                                                            # is the first one swapped, so both sides occur
    seg = np.repeat(np.arange(len(sizes)), sizes)
    L = sid.astype(np.int64) - c.lo
    exp = np.where(D[L, pa[seg].astype(np.int64) - c.lo] <= D[L, pb[seg].astype(np.int64) - c.lo], 0, 1).astype(np.uint8)
    side = c.ix.pivot_split(sid, soff, pa, pb)
    np.testing.assert_array_equal(side, exp)
    assert (side[700:764] == 0).all() and 0 < exp.sum() < len(exp)


# ---- g: brute force over the whole table ----

@on(*CASES)
def test_bruteforce_knn_and_range(hx):
    """valid by the dominance condition: no zero row can enter a result"""
    c = hx
    for k in (10, 100):
        ei, ed, _ = hr.knn_ref(c.Q, c.Xb, c.lo, k, c.metric)
        gi, gd = c.ix.bruteforce_knn(c.Q, k)
        np.testing.assert_array_equal(gi, ei, err_msg=f"k = {k}")
        np.testing.assert_array_equal(gd, ed)
        _above_and_below(c, ei)
    for qt in hr.RADIUS_QUANTILES:
        r = hr.radius(c.geom, c.dtype, c.metric, qt)
        eo, ei = hr.range_ref(c.Q, c.Xb, c.lo, r, c.metric)
        go, gi = c.ix.bruteforce_range(c.Q, r)
        np.testing.assert_array_equal(go, eo)
        np.testing.assert_array_equal(gi, ei)
        assert len(ei) > len(c.Q)
        _above_and_below(c, ei)


# ---- h: allow bitmaps ----

def _half(c, seed=11):
    keep = np.random.default_rng(seed).random(M) < 0.5
    keep[M // 2 - 1], keep[M // 2] = True, False                   # of the duplicated pair across the line only the lower row
    return keep


MASKED_FIELDS = ("ids", "dists", "result_count", "allowed_cmps", "frontier_size", "visited_count", "dist_cmps", "degree_sum")


@on("A-f16")
def test_masked_knn_and_masked_search(hx):
    c = hx
    keep = _half(c)
    allow = hr.block_allow(c.n, c.ids[keep])
    Q = c.Q[:8]
    ei, ed, ec = hr.knn_ref(Q, c.Xb, c.lo, 10, c.metric, allowed=keep)
    gi, gd, gc = c.ix.bruteforce_knn_masked(Q, 10, allow)
    np.testing.assert_array_equal(gi, ei); np.testing.assert_array_equal(gd, ed); np.testing.assert_array_equal(gc, ec)
    ref = masked_ref.masked_batch_search(c.X, c.G, allow, queries=Q, k=10, beam=64, starts=(c.start,), metric=c.metric)
    _same(c.ix.batch_search_masked(Q, allow, k=10, beam=64, starts=(c.start,)), ref, MASKED_FIELDS, "masked search")
    assert (ref["result_count"] == 10).all()


# ---- i: labels ----

@on("B-u8")
def test_labels(hx):
    c = hx
    lab = np.random.default_rng(8).integers(1, 8, M).astype(np.uint32)          # never 0: a zero row's label matches nothing below
    lab[M // 2 - 1], lab[M // 2] = 5, 6
    Q = c.Q[:8]
    try:
        c.ix.set_labels(lab, first_row=c.lo)
        np.testing.assert_array_equal(c.ix.labels(c.lo, M), lab)
        assert not c.ix.labels(0, 64).any() and not c.ix.labels(c.n - 64, 64).any()
        for where in (("match", (7, 5)), ("any", (2, 0)), ("range", (1, 3))):
            keep = label_allow(lab, *where)
            assert 0 < keep.sum() < M and c.ix.label_count(where) == int(keep.sum())
            ei, ed, ec = hr.knn_ref(Q, c.Xb, c.lo, 10, c.metric, allowed=keep)
            gi, gd, gc = c.ix.bruteforce_knn_labeled(Q, 10, where)
            np.testing.assert_array_equal(gi, ei, err_msg=str(where)); np.testing.assert_array_equal(gd, ed); np.testing.assert_array_equal(gc, ec)
        table = np.array([(7, 5), (7, 6), (7, 1)], np.uint32)
        group = np.arange(len(c.Q)) % 3
        gi, gd, gc = c.ix.bruteforce_knn_grouped(c.Q, 10, where=("match", table), group_of_query=group)
        for gno in range(3):
            keep = label_allow(lab, "match", tuple(int(v) for v in table[gno]))
            ei, ed, ec = hr.knn_ref(c.Q[group == gno], c.Xb, c.lo, 10, c.metric, allowed=keep)
            np.testing.assert_array_equal(gi[group == gno], ei); np.testing.assert_array_equal(gd[group == gno], ed)
            np.testing.assert_array_equal(gc[group == gno], ec)
        where = ("match", (7, 5))
        allow = hr.block_allow(c.n, c.ids[label_allow(lab, *where)])
        ref = masked_ref.masked_batch_search(c.X, c.G, allow, queries=Q, k=10, beam=64, starts=(c.start,), metric=c.metric)
        _same(c.ix.batch_search_labeled(Q, where, k=10, beam=64, starts=(c.start,)), ref, MASKED_FIELDS, "labeled search")
    finally:
        c.ix.drop_labels()


# ---- j: range search ----

@on(*AB)
def test_range_search_and_range_query(hx, oracle):
    c = hx
    cap = 256
    shared = np.array([c.start, c.b0 - 1, c.b0, c.lo + 3, c.lo + M - 2], np.uint32)
    per = oracle.batch_search(c.X, c.G, queries=c.Q, k=10, beam=32, starts=(c.start,), metric=c.metric)["ids"]
    qid = c.ids[::67]
    trunc = []
    for qt in hr.RADIUS_QUANTILES:
        r = hr.radius(c.geom, c.dtype, c.metric, qt)
        for starts in (shared, per):
            o = oracle.range_search(c.X, c.G, starts, r, cap, queries=c.Q, metric=c.metric)
            g = c.ix.range_search(starts, r, cap, queries=c.Q)
            _same(g, o, ("counts", "truncated", "ids"), f"range_search at {r}")
            ok = o["truncated"] == 0
            np.testing.assert_array_equal(g["dist_cmps"][ok], o["dist_cmps"][ok])
            trunc.append(o["truncated"])
        assert o["counts"].sum() > len(c.Q)
        for kw_o, kw_g in ((dict(queries=c.Q), dict(queries=c.Q)), (dict(query_ids=qid), dict(query_ids=qid))):
            so = oracle.batch_search(c.X, c.G, k=16, beam=16, cut=0.0, starts=(c.start,), metric=c.metric, **kw_o)
            o = oracle.range_search(c.X, c.G, so["ids"], r, cap, metric=c.metric, **kw_o)
            g = c.ix.range_query(radius=r, beam=16, max_results=cap, starts=(c.start,), **kw_g)
            _same(g, o, ("counts", "truncated", "ids"), f"range_query at {r}")
            np.testing.assert_array_equal(g["search_cmps"], so["dist_cmps"]); np.testing.assert_array_equal(g["visited"], so["visited_count"])
            ok = o["truncated"] == 0
            np.testing.assert_array_equal(g["range_cmps"][ok], o["dist_cmps"][ok])
    assert not np.concatenate(trunc).all()


# ---- k: reachability ----

@on("B-u8")
def test_reachability(hx):
    """the walk reads graph rows only, so the block-local graph with ids shifted by lo is the exact reference"""
    c = hx
    for rounds in (0, 2):
        ref = reach_ref.reach_ref(c.Gl, (c.start - c.lo,), max_rounds=rounds)
        got = c.ix.reachability(starts=(c.start,), consider=c.allow_block, max_rounds=rounds, levels=False)
        for f in reach_ref.STAT_KEYS:
            assert got[f] == ref[f], (rounds, f, got[f], ref[f])
        np.testing.assert_array_equal(got["unreached_ids"], ref["unreached_ids"] + np.uint32(c.lo))
        np.testing.assert_array_equal(got["reached"], hr.block_allow(c.n, c.ids[reach_ref.unpack(ref["reached"], M)]))
    assert ref["truncated"] and ref["unreached_count"] > 0


# ---- l: quantised copy, fused rerank, sketch pre-filter ----

@on("C-f32")
def test_quantised_copy_rerank_and_filtered_search(hx, oracle):
    c = hx
    slope, offset = 0.5, 0                                                    # halves, so the quantiser rounds; a zero row stays zero
    qp = quantize.device_params("euclid_u8", c.d, slope=slope, offset=offset)
    quant, _ = c.ix.quantized("euclid_u8", params=qp)
    try:
        Xqb = oracle.euclid_u8_translate(c.Xb, slope, offset)
        np.testing.assert_array_equal(Xqb, (hr.as_int(c.Xb) + 1) // 2)                     # std::round: halves go up
        assert not oracle.euclid_u8_translate(np.zeros((1, c.d), np.float32), slope, offset).any()
        np.testing.assert_array_equal(quant.points(c.lo, M), Xqb)
        assert not quant.points(0, 64).any() and not quant.points(c.n - 64, 64).any() and not quant.points(c.lo - 64, 64).any()
        Xq = np.zeros((c.n, c.d), np.uint8)
        Xq[c.lo:c.lo + M] = Xqb
        Qq = oracle.euclid_u8_translate(c.Q, slope, offset)
        # the oracle composition of tests/test_search_rerank_gpu.py::test_exact_order_equals_the_oracle_composition
        k, beam = 10, 64
        got = c.ix.search_rerank(quant, qp, c.Q, k=k, beam=beam, starts=(c.start,))
        o = oracle.batch_search(Xq, c.G, queries=Qq, k=k, beam=beam, cut=1.35, out_k=beam, starts=(c.start,))
        QD = hr.dist_matrix(c.Q, c.Xb, c.metric).astype(np.float32)
        exp_ids, exp_d = [], []
        for i in range(len(c.Q)):
            cc = o["ids"][i, :min(o["frontier_size"][i], k * 100)]
            dd = QD[i, cc.astype(np.int64) - c.lo]
            order = np.lexsort((cc, dd))[:k]
            exp_ids.append(cc[order]); exp_d.append(dd[order])
        np.testing.assert_array_equal(got["ids"], np.array(exp_ids))
        np.testing.assert_array_equal(got["dists"], np.array(exp_d, np.float32))
        _same(got, o, ("frontier_size", "visited_count", "dist_cmps"), "fused rerank")
        _above_and_below(c, got["ids"])
        # the bit-sketch pre-filter on the quantised handle
        sp = sk.make_params("euclid_bit", c.d, median=190)
        sk.attach_sketch(quant, c.ix, sp)
        S = np.zeros((c.n, sk.row_bytes(sp.kind, c.d)), np.uint8)
        S[c.lo:c.lo + M] = sk.sketch_rows_numpy(c.Xb, sp)
        np.testing.assert_array_equal(sk.download_sketch(quant, c.lo, M), S[c.lo:c.lo + M])
        nq = 8
        sq = sk.sketch_rows(c.Q[:nq], sp)
        np.testing.assert_array_equal(sq, sk.sketch_rows_numpy(c.Q[:nq], sp))
        ref = filtered_ref.filtered_batch_search(Xq, c.G, queries=Qq[:nq], k=k, beam=beam, starts=(c.start,), use_filtering=True, sketches=S,
                                                 sketch_queries=sq, sketch_params=sp)
        g = quant.batch_search_filtered(Qq[:nq], sq, k=k, beam=beam, starts=(c.start,))
        _same(g, ref, SEARCH_FIELDS + ("pruned_cmps",), "filtered search")
        assert (ref["sketch_dropped"] > 0).any()
    finally:
        quant.close()
