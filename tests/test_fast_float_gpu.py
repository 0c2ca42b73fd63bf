"""GPU parity of the FAST float paths (default mode, never exact_float_order) on signed, fractional and real-valued data.

A. Grid data (tests/float_cases.py: coordinates m / 8, both signs, planted zero / duplicate / negated / orthogonal rows, MIPS
   queries whose top-k holds negative, zero and positive distances): every sum is exact in f32 in any order and any algebraic
   form, so search, prune, builds, leaf kNN, brute force, plain distances, range search and the top-k merge must equal the
   oracle BIT FOR BIT -- the v_fma_mix / v_pk_fma gather accumulators, the butterfly combine, the matrix-core kernels with
   their norm form, negated keys and register lists included.  Distances are compared as floats (-0.0 == +0.0, as the
   reference compares them); the order among zero distances is asserted through the ids.
B. The same on data scaled by 2^s (f16: subnormals at s = -14, a maximum of 51 200 at s = +12; bf16 / f32: s = -40, +40):
   ids and counters as unscaled, distances times 4^s exactly -- operands are widened exactly or this fails.
C. Real-valued data (DEEP-, T2I-shaped, SIFT-shaped plus a fraction): float64 reference on the stored values, the DERIVED
   bounds of float_cases.tolerances per kernel form, completeness over all points, and L2 distances >= 0 (duplicated rows
   included).  Largest observed |err| / tol and relative error per (form, type, data set) are printed; DESIGN.md quotes them.
"""
import ctypes as C

import numpy as np
import pytest

import float_cases as fc
from parlayann_amd import DeviceIndex, bfloat16

pytestmark = pytest.mark.gpu

TYPES = pytest.mark.parametrize("dtype", fc.FLOAT_TYPES, ids=fc.type_name)
METRICS = pytest.mark.parametrize("metric", ["l2", "mips"])
SCALES = {np.dtype(np.float16): (-14, 12), np.dtype(np.float32): (-40, 40), bfloat16: (-40, 40)}
SCALED = pytest.mark.parametrize("dtype,si", [(t, i) for t in fc.FLOAT_TYPES for i in (0, 1)],
                                 ids=lambda v: fc.type_name(v) if not isinstance(v, int) else ("down", "up")[v])
COUNTERS = ("frontier_size", "visited_count", "dist_cmps", "degree_sum")


def _planted_ids(c):
    return np.concatenate([v.ravel() for v in c.planted.values() if isinstance(v, np.ndarray)]).astype(np.uint32)


def _alpha(metric):
    return 1.2 if metric == "l2" else 1.0


def _norm(G):
    G = G.copy()
    cols = np.arange(G.shape[1] - 1)[None, :]
    G[:, 1:][cols >= G[:, :1]] = 0
    return G


_graphs = {}


def _grid(oracle, n, d, dtype, metric, nq=200, s=0, seed=11):
    """grid case + the oracle's Vamana graph of the UNSCALED table (a graph is topology: the scaled copies search the same one)"""
    c = fc.grid_like(n, d, seed, dtype, metric, nq=nq, s=s)
    key = (n, d, fc.type_name(dtype), metric, seed)
    if key not in _graphs:
        base = c if s == 0 else fc.grid_like(n, d, seed, dtype, metric, nq=nq)
        _graphs[key] = oracle.vamana_build(base.X, 32, 64, _alpha(metric), seed=7, metric=metric)[0]
    return c, _graphs[key]


def _same_search(o, g, visited=False):
    for f in COUNTERS:
        np.testing.assert_array_equal(o[f], g[f], err_msg=f)
    np.testing.assert_array_equal(o["ids"], g["ids"])
    np.testing.assert_array_equal(o["dists"], g["dists"])
    if visited:
        for i in range(len(o["ids"])):
            nv = o["visited_count"][i]
            np.testing.assert_array_equal(o["visit_order_ids"][i, :nv], g["visited_ids"][i, :nv])
            order = np.lexsort((g["visited_ids"][i, :nv], g["visited_dists"][i, :nv] + np.float32(0.0)))
            np.testing.assert_array_equal(o["visited_ids"][i, :nv], g["visited_ids"][i, :nv][order])
            np.testing.assert_array_equal(o["visited_dists"][i, :nv], g["visited_dists"][i, :nv][order])


# ======================================================================================================================
# A. bit-exact on grid data
# ======================================================================================================================
@TYPES
@METRICS
@pytest.mark.parametrize("d", [32, 96, 128, 200])
def test_grid_search_every_frontier_kernel(oracle, dtype, metric, d):
    """beams 1 / 16 / 64 (register b64), 100 / 128 (register b128), 300 (LDS frontier); d = 32: 64-byte f16 / bf16 rows take
    the LDS-query variants"""
    n = 5000
    c, G = _grid(oracle, n, d, dtype, metric)
    X, Q = c.X, c.Q
    ix = DeviceIndex(X, G, metric=metric)
    for beam in (1, 16, 64, 100, 128, 300):
        k = min(10, beam)
        o = oracle.batch_search(X, G, queries=Q, k=k, beam=beam, cut=1.35, metric=metric, out_k=beam, visited_cap=n)
        g = ix.batch_search(Q, k=k, beam=beam, cut=1.35, out_k=beam, visited_cap=n)
        assert o["rc"] == 0
        _same_search(o, g, visited=True)
    if metric == "mips":       # the planted queries see distances of both signs and zeros in one result row
        r = ix.batch_search(Q[3:5], k=10, beam=300, out_k=300)["dists"]
        assert (r < 0).any() and (r == 0).any() and (r > 0).any()
    if d in (32, 128):
        # the builder's mode: base-point queries, k = 0, cut 0, visited lists
        qid = np.concatenate([np.random.default_rng(5).integers(0, n, 300), _planted_ids(c)])
        qid = qid.astype(np.uint32)
        for L in (64, 128):
            o = oracle.batch_search(X, G, query_ids=qid, k=0, beam=L, cut=0.0, metric=metric, out_k=L, visited_cap=n)
            g = ix.batch_search(query_ids=qid, k=0, beam=L, cut=0.0, out_k=L, visited_cap=n)
            _same_search(o, g, visited=True)
        # one start set per query
        rng = np.random.default_rng(3)
        for nst, beam in ((1, 64), (3, 100)):
            starts = np.stack([rng.choice(n, nst, replace=False) for _ in range(len(Q))]).astype(np.uint32)
            g = ix.batch_search(Q, k=10, beam=beam, starts=starts)
            for i in (0, 3, 4, 7, 100, len(Q) - 1):
                o = oracle.batch_search(X, G, queries=Q[i:i + 1], k=10, beam=beam, starts=starts[i], metric=metric)
                np.testing.assert_array_equal(o["ids"][0], g["ids"][i])
                np.testing.assert_array_equal(o["dists"][0], g["dists"][i])
                for f in COUNTERS:
                    assert o[f][0] == g[f][i], f
    ix.close()


@TYPES
@METRICS
@pytest.mark.parametrize("k,cut,limit,dl", [(0, 0.0, None, None), (10, 0.0, None, None), (10, 1.35, 20, None),
                                            (10, 1.35, 1000, 16), (10, 1.1, 100, None), (5, 2.0, None, 8),
                                            (10, 1.35, 0, None), (10, 1.35, 127, None), (10, 1.35, 128, None)])
def test_grid_search_params(oracle, dtype, metric, k, cut, limit, dl):
    """cut-prune, visit limit and degree limit compare non-integer distances of both signs"""
    c, G = _grid(oracle, 5000, 128, dtype, metric)
    ix = DeviceIndex(c.X, G, metric=metric)
    o = oracle.batch_search(c.X, G, queries=c.Q, k=k, beam=64, cut=cut, limit=limit, degree_limit=dl, out_k=64,
                            visited_cap=2048, metric=metric)
    g = ix.batch_search(c.Q, k=k, beam=64, cut=cut, limit=limit, degree_limit=dl, out_k=64, visited_cap=2048)
    assert o["rc"] == 0
    _same_search(o, g, visited=True)
    ix.close()


@TYPES
@METRICS
def test_grid_robust_prune(oracle, dtype, metric):
    n = 4000
    c = fc.grid_like(n, 96, 21, dtype, metric)
    X = c.X
    G, _ = oracle.vamana_build(X, R=24, L=48, alpha=_alpha(metric), seed=3, metric=metric, max_degree=32)
    rng = np.random.default_rng(0)
    owners = np.concatenate([rng.integers(0, n, 250), _planted_ids(c)]).astype(np.uint32)
    cands = []
    for i, p in enumerate(owners):
        cc = rng.choice(n, int(rng.integers(0, 200)), replace=False).astype(np.uint32)
        if i % 7 == 0 and len(cc) > 3:
            cc = np.concatenate([cc, cc[:3], [p]]).astype(np.uint32)              # duplicates and the owner itself
        if i % 5 == 0:
            cc = np.concatenate([cc, c.planted["dup"].ravel(), c.planted["zero"], c.planted["neg"]]).astype(np.uint32)
        cands.append(cc)
    off = np.concatenate([[0], np.cumsum([len(cc) for cc in cands])]).astype(np.uint64)
    cid = np.concatenate(cands).astype(np.uint32)
    own = np.repeat(owners, np.diff(off).astype(np.int64))
    cd = fc.ref_pairs(X[cid], X[own], metric).astype(np.float32)                  # exact on the grid (test_float_cases_cpu.py)
    ix = DeviceIndex(X, G, metric=metric)
    for alpha, R, add, with_d in ((1.2, 24, True, True), (1.0, 32, True, False), (1.2, 8, False, False), (1.0, 32, False, True)):
        ro, dco = oracle.robust_prune_batch(X, G, owners, cid, cd if with_d else None, off, alpha, R, add=add, metric=metric)
        rg, dcg = ix.robust_prune_batch(owners, cid, off, alpha, R, cand_dists=cd if with_d else None, add_out_nbrs=add)
        np.testing.assert_array_equal(ro, rg, err_msg=f"alpha {alpha} R {R}")
        np.testing.assert_array_equal(dco, dcg)
    ix.close()


@TYPES
@METRICS
@pytest.mark.parametrize("L", [64, 100])
def test_grid_vamana_build_identical_graph(oracle, dtype, metric, L):
    """L = 100: the builder's searches take the 91..128 filter-code path"""
    X = fc.grid_like(4000, 128, 31, dtype, metric).X
    Go, so = oracle.vamana_build(X, 32, L, _alpha(metric), num_passes=1, seed=11, metric=metric)
    ix = DeviceIndex(X, max_degree=32, metric=metric)
    st = ix.vamana_build(32, L, _alpha(metric), num_passes=1, seed=11)
    np.testing.assert_array_equal(_norm(Go), _norm(ix.get_graph()))
    assert int(so[0]) == st.search_dist_cmps and int(so[1]) == st.prune_dist_cmps
    ix.close()


@TYPES
@METRICS
def test_grid_hcnng_build_identical_graph(oracle, dtype, metric):
    """the leaves go through the matrix-core leaf kNN for f16 / bf16"""
    X = fc.grid_like(4000, 128, 41, dtype, metric).X
    Go = oracle.hcnng_build(X, 4, 300, 3, seed=9, metric=metric)
    ix = DeviceIndex(X, max_degree=Go.shape[1] - 1, metric=metric)
    ix.hcnng_build(4, 300, 3, seed=9)
    np.testing.assert_array_equal(_norm(Go), _norm(ix.get_graph()))
    ix.close()


def _leaves(c, n, rng):
    sizes = [1000, 300, 64, 65, 37, 2, 1, 11]
    leaves = [rng.choice(n, s, replace=False).astype(np.uint32) for s in sizes]
    special = np.concatenate([c.planted["dup"].ravel(), c.planted["zero"], c.planted["neg"], c.planted["orth"]])
    for li in (0, 1):                                                  # equal rows, the zero row, a row and its negation in one leaf
        rest = leaves[li][~np.isin(leaves[li], special)]
        leaves[li] = np.concatenate([special, rest])[: sizes[li]].astype(np.uint32)
    leaves[5] = c.planted["dup"][0].astype(np.uint32)                  # a leaf of two equal rows
    return sizes, leaves


def _leaf_check(oracle, ix, X, sizes, leaves, metric):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    gi, gd = ix.leaf_knn_batch(np.concatenate(leaves), off, 10)
    for li, ids in enumerate(leaves):
        oi, od = oracle.leaf_knn(X, ids, 10, metric=metric)
        np.testing.assert_array_equal(oi, gi[off[li]:off[li + 1]], err_msg=f"leaf {li} size {len(ids)}")
        np.testing.assert_array_equal(od, gd[off[li]:off[li + 1]], err_msg=f"leaf {li} size {len(ids)}")
    return gi, gd


@TYPES
@METRICS
@pytest.mark.parametrize("d", [40, 96, 128, 200])
def test_grid_leaf_knn(oracle, dtype, metric, d):
    n = 5000
    c = fc.grid_like(n, d, 51, dtype, metric)
    sizes, leaves = _leaves(c, n, np.random.default_rng(3))
    ix = DeviceIndex(c.X, max_degree=8, metric=metric)
    _leaf_check(oracle, ix, c.X, sizes, leaves, metric)
    ix.close()


BF_CASES = [(1, 0, 130), (10, 1, 64), (16, 2, 65), (17, 3, 130), (64, 5, 1), (100, 0, 130), (113, 2, 65), (128, 1, 64),
            (100, 5, 130), (10, 3, 1), (128, 0, 65)]


def _bf_check(oracle, ix, X, Q, k, pieces, metric, tag=""):
    ix.set_option("gt_pieces", pieces)
    gi, gd = ix.bruteforce_knn(Q, k)
    oi, od = oracle.bruteforce_knn(X, Q, k, metric=metric)
    np.testing.assert_array_equal(oi, gi, err_msg=f"{tag} k={k} pieces={pieces} nq={len(Q)}")
    np.testing.assert_array_equal(od, gd, err_msg=f"{tag} k={k} pieces={pieces} nq={len(Q)}")
    return gi, gd


@TYPES
@METRICS
def test_grid_bruteforce(oracle, dtype, metric):
    """lane lists (k <= 16), register lists of 2..8 registers (k = 17..128), every piece count, partial query tiles"""
    c = fc.grid_like(9000, 128, 61, dtype, metric, nq=130)
    ix = DeviceIndex(c.X, max_degree=8, metric=metric)
    for k, pieces, nq in BF_CASES:
        gi, gd = _bf_check(oracle, ix, c.X, c.Q[:nq], k, pieces, metric)
        if nq >= 8 and k >= 100:
            if metric == "mips":
                assert (gd[3] < 0).any() and (gd[3] == 0).any() and (gd[3] > 0).any()      # one top-k, three signs
            else:
                assert gd[1, 0] == 0 and gd[1, 1] == 0 and gi[1, 0] < gi[1, 1]              # the query equal to two rows
    ix.close()


@TYPES
@METRICS
def test_grid_bruteforce_fewer_points_than_k_and_long_rows(oracle, dtype, metric):
    c = fc.grid_like(70, 128, 62, dtype, metric, nq=20)                # n < k: unused slots are SENTINEL / +inf
    ix = DeviceIndex(c.X, max_degree=8, metric=metric)
    for k, pieces in ((100, 0), (128, 2), (10, 1), (17, 3)):
        _bf_check(oracle, ix, c.X, c.Q, k, pieces, metric, "n=70")
    ix.close()
    c = fc.grid_like(5000, 200, 63, dtype, metric, nq=65)              # two-byte rows of 400 bytes: the fallback above 256 B
    ix = DeviceIndex(c.X, max_degree=8, metric=metric)
    for k, pieces in ((10, 0), (64, 2), (100, 0), (113, 5)):
        _bf_check(oracle, ix, c.X, c.Q, k, pieces, metric, "d=200")
    ix.close()
    c = fc.grid_like(3000, 96, 64, dtype, metric, nq=64)
    ix = DeviceIndex(c.X, max_degree=8, metric=metric)
    for k, pieces in ((10, 0), (37, 3), (100, 1)):
        _bf_check(oracle, ix, c.X, c.Q, k, pieces, metric, "d=96")
    ix.close()


@pytest.mark.parametrize("dtype,metric,k,pieces", [(np.float16, "mips", 100, 5), (bfloat16, "l2", 17, 3), (np.float32, "mips", 10, 4),
                                                   (bfloat16, "mips", 16, 6), (np.float16, "l2", 100, 0)],
                         ids=lambda v: fc.type_name(v) if isinstance(v, (type, np.dtype)) else str(v))
def test_grid_bruteforce_many_workgroups_per_cu(oracle, dtype, metric, k, pieces):
    """4 000 queries x 60 000 points: several workgroups per CU, the pieces of a row race to publish bounds of both signs"""
    c = fc.grid_like(60000, 64, 71, dtype, metric, nq=4000)
    ix = DeviceIndex(c.X, max_degree=8, metric=metric)
    _bf_check(oracle, ix, c.X, c.Q, k, pieces, metric)
    ix.close()


@TYPES
@METRICS
@pytest.mark.parametrize("d", [32, 96, 200])
def test_grid_plain_distances(oracle, dtype, metric, d):
    n = 3000
    c = fc.grid_like(n, d, 81, dtype, metric, nq=24)
    X, Q, p = c.X, c.Q, c.planted
    ix = DeviceIndex(X, max_degree=8, metric=metric)
    rng = np.random.default_rng(0)
    a = rng.integers(0, n, 500).astype(np.uint32); b = rng.integers(0, n, 500).astype(np.uint32)
    a[:6] = [p["dup"][0][0], p["dup"][1][0], p["neg"][0], p["zero"][0], 7, p["orth"][0]]
    b[:6] = [p["dup"][0][1], p["dup"][1][1], p["neg"][1], 9, 7, p["zero"][0]]
    np.testing.assert_array_equal(ix.pair_distances(a, b), fc.ref_pairs(X[a], X[b], metric).astype(np.float32))
    for i in range(0, 40):                                             # and the oracle itself on a sample
        assert ix.pair_distances(a[i:i + 1], b[i:i + 1])[0] == np.float32(oracle.distance(X[a[i]], X[b[i]], metric))
    ids = np.concatenate([rng.integers(0, n, 150), _planted_ids(c)]).astype(np.uint32)
    ref = fc.ref_matrix(Q, X, metric)
    np.testing.assert_array_equal(ix.query_distances(Q, ids), ref[:, ids].astype(np.float32))
    # rerank: exact distances of each query's candidates, sorted by (dist, id) or kept in order
    pool = np.setdiff1d(np.arange(n), _planted_ids(c))
    cand = np.stack([rng.choice(pool, 60, replace=False) for _ in range(len(Q))]).astype(np.uint32)
    cand[:, 5] = p["dup"][0][1]; cand[:, 40] = p["dup"][0][0]; cand[:, 7] = p["zero"][0]; cand[:, 9:12] = p["orth"]
    cnt = rng.integers(12, 61, len(Q)).astype(np.uint32)
    gi, gd = ix.rerank(Q, cand, cnt, 8, resort=False)
    np.testing.assert_array_equal(gi, cand[:, :8])
    np.testing.assert_array_equal(gd, np.take_along_axis(ref, cand[:, :8].astype(np.int64), 1).astype(np.float32))
    gi, gd = ix.rerank(Q, cand, cnt, 20, resort=True)
    for i in range(len(Q)):
        cc = cand[i, :cnt[i]]
        dd = ref[i, cc].astype(np.float32) + np.float32(0.0)
        order = np.lexsort((cc, dd))[:20]
        np.testing.assert_array_equal(gi[i, :len(order)], cc[order], err_msg=f"rerank row {i}")
        np.testing.assert_array_equal(gd[i, :len(order)], dd[order])
        assert (gi[i, len(order):] == fc.SENTINEL).all() and np.isposinf(gd[i, len(order):]).all()
    # pivot split: side 0 when d(id, a) <= d(id, b) -- equal pivots (every compare is a tie), a pivot and its negation, the zero row
    sizes = [700, 64, 1, 130, 200]
    sid = np.concatenate([rng.choice(n, s, replace=False) for s in sizes]).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    pa = np.array([rng.integers(0, n), p["dup"][0][0], 5, p["neg"][0], p["zero"][0]], np.uint32)
    pb = np.array([rng.integers(0, n), p["dup"][0][1], 6, p["neg"][1], p["orth"][0]], np.uint32)
    side = ix.pivot_split(sid, off, pa, pb)
    seg = np.repeat(np.arange(len(sizes)), sizes)
    da = fc.ref_pairs(X[sid], X[pa[seg]], metric); db = fc.ref_pairs(X[sid], X[pb[seg]], metric)
    np.testing.assert_array_equal(side, np.where(da <= db, 0, 1).astype(np.uint8))
    assert (side[700:764] == 0).all()
    ix.close()


@TYPES
@METRICS
def test_grid_range_search_radius_equal_to_a_distance(oracle, dtype, metric):
    """radius_2 EQUAL to a distance that occurs, and the float just below it: `<=` on an exact non-integer threshold decides"""
    n = 5000
    c, G = _grid(oracle, n, 128, dtype, metric)
    X, Q = c.X, c.Q
    ix = DeviceIndex(X, G, metric=metric)
    starts = ix.batch_search(Q, k=10, beam=32)["ids"]
    ref = fc.ref_matrix(Q, X, metric).astype(np.float32)
    radii = []
    for rank in (10, 40):
        kth = np.sort(np.partition(ref, rank - 1, axis=1)[:, rank - 1])
        kth = kth[len(kth) // 2:]
        r = np.float32(kth[kth != np.rint(kth)][0])                     # a typical rank-th distance that is no integer
        assert (ref == r).any()                                         # and occurs
        radii += [r, np.nextafter(r, np.float32(-np.inf))]
    if metric == "mips":
        radii += [np.float32(0.0), np.float32(-0.0)]                    # a threshold at the sign change, either zero
    counts = []
    for r2 in radii:
        o = oracle.range_search(X, G, starts, float(r2), 2048, queries=Q, metric=metric)
        g = ix.range_search(starts, float(r2), 2048, queries=Q)
        for f in ("counts", "truncated", "ids"):
            np.testing.assert_array_equal(o[f], g[f], err_msg=f"{f} at radius {r2!r}")
        ok = o["truncated"] == 0
        np.testing.assert_array_equal(o["dist_cmps"][ok], g["dist_cmps"][ok])
        counts.append(int(o["counts"].sum()))
    assert counts[0] > counts[1] and counts[2] >= counts[3]             # a boundary point is in at r and out just below
    ix.close()


def test_merge_topk_mixed_signs_zeros_and_ties(oracle):
    import torch
    from parlayann_amd import _capi, distributed as D
    lib = _capi.load()
    rng = np.random.default_rng(6)
    dev = torch.device("cuda", 0)
    for W, nq, k in ((2, 300, 10), (8, 500, 100), (3, 7, 1), (5, 64, 17)):
        ids = rng.permutation(1 << 20)[: W * nq * k].reshape(W, nq, k).astype(np.uint32)
        d = np.sort(rng.integers(-12, 13, (W, nq, k)).astype(np.float32) / np.float32(4.0), axis=2)     # many ties, both signs
        d[(d == 0) & (rng.random(d.shape) < 0.5)] = np.float32(-0.0)                                       # both zeros
        assert d.size < 1000 or (np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all())
        ids[0, ::5, k - 1] = fc.SENTINEL; d[0, ::5, k - 1] = np.inf                                        # short lists
        if k > 4:
            ids[1, ::3, k - 3:] = fc.SENTINEL; d[1, ::3, k - 3:] = np.inf
        ti = torch.from_numpy(ids.view(np.int32)).to(dev); td = torch.from_numpy(d).to(dev)
        oi = torch.empty((nq, k), dtype=torch.int32, device=dev); od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _capi.check(lib.pann_merge_topk_dev(ti.data_ptr(), td.data_ptr(), W, nq, k, k, None, k, oi.data_ptr(), od.data_ptr(), st))
        torch.cuda.synchronize()
        ei, ed = D.merge_topk(ids, d, k)
        np.testing.assert_array_equal(oi.cpu().numpy().view(np.uint32), ei)
        np.testing.assert_array_equal(od.cpu().numpy(), ed)
        # independent of merge_topk's own key mapping: plain (float, id) lexicographic order
        allid = np.transpose(ids, (1, 0, 2)).reshape(nq, W * k); alld = np.transpose(d, (1, 0, 2)).reshape(nq, W * k)
        for i in range(0, nq, 7):
            use = allid[i] != fc.SENTINEL
            order = np.lexsort((allid[i][use], alld[i][use] + np.float32(0.0)))[:k]
            np.testing.assert_array_equal(ei[i, :len(order)], allid[i][use][order])


# ======================================================================================================================
# B. exponent sweep: the same results on data scaled by 2^s
# ======================================================================================================================
def _scaled_pair(n, d, seed, dtype, metric, si, nq):
    s = SCALES[np.dtype(dtype)][si]
    return fc.grid_like(n, d, seed, dtype, metric, nq=nq), fc.grid_like(n, d, seed, dtype, metric, nq=nq, s=s), 4.0 ** s


@SCALED
@METRICS
def test_scaled_search(oracle, dtype, si, metric):
    """The device equals the oracle at the scaled data at every s.  Ids and counters equal the unscaled run only while the
    distances stay below 2^31: the reference admits a candidate to a frontier that is not yet full only below
    (float)INT_MAX (beamSearch.h:150-152), so at s = +12 / +40 the oracle's own result is a different one (still matched
    bit for bit); the metamorphic relation is asserted at the down scale and at s = +6."""
    s_far = SCALES[np.dtype(dtype)][si]
    c0, G = _grid(oracle, 5000, 128, dtype, metric)
    i0 = DeviceIndex(c0.X, G, metric=metric)
    for s in ((s_far,) if si == 0 else (s_far, 6)):
        c1, _ = _grid(oracle, 5000, 128, dtype, metric, s=s)
        i1 = DeviceIndex(c1.X, G, metric=metric)
        for beam in (64, 100):
            b = i1.batch_search(c1.Q, k=10, beam=beam, out_k=beam)
            o = oracle.batch_search(c1.X, G, queries=c1.Q, k=10, beam=beam, out_k=beam, metric=metric)
            _same_search(o, b)
            if s != s_far or si == 0:
                a = i0.batch_search(c0.Q, k=10, beam=beam, out_k=beam)
                assert np.abs(a["dists"][np.isfinite(a["dists"])]).max() * 4.0 ** s < 2.0 ** 31
                for f in COUNTERS + ("ids",):
                    np.testing.assert_array_equal(a[f], b[f], err_msg=f)
                np.testing.assert_array_equal(a["dists"].astype(np.float64) * 4.0 ** s, b["dists"].astype(np.float64))
        i1.close()
    i0.close()


@SCALED
@METRICS
def test_scaled_dense_and_pairs(oracle, dtype, si, metric):
    """brute force k = 10 / 100, leaf kNN, pair distances: f16 subnormal operands and operands near 65504 reach the matrix
    cores and v_fma_mix widened exactly"""
    n = 6000
    c0, c1, f = _scaled_pair(n, 128, 91, dtype, metric, si, 130)
    i0 = DeviceIndex(c0.X, max_degree=8, metric=metric); i1 = DeviceIndex(c1.X, max_degree=8, metric=metric)
    for k in (10, 100):
        ai, ad = i0.bruteforce_knn(c0.Q, k)
        bi, bd = _bf_check(oracle, i1, c1.X, c1.Q, k, 0, metric, "scaled")
        np.testing.assert_array_equal(ai, bi)
        np.testing.assert_array_equal(ad.astype(np.float64) * f, bd.astype(np.float64))
    sizes, leaves = _leaves(c0, n, np.random.default_rng(4))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ai, ad = i0.leaf_knn_batch(np.concatenate(leaves), off, 10)
    bi, bd = _leaf_check(oracle, i1, c1.X, sizes, leaves, metric)
    np.testing.assert_array_equal(ai, bi)
    np.testing.assert_array_equal(ad.astype(np.float64) * f, bd.astype(np.float64))
    rng = np.random.default_rng(1)
    a = rng.integers(0, n, 600).astype(np.uint32); b = rng.integers(0, n, 600).astype(np.uint32)
    pa, pb = i0.pair_distances(a, b), i1.pair_distances(a, b)
    np.testing.assert_array_equal(pb, fc.ref_pairs(c1.X[a], c1.X[b], metric).astype(np.float32))
    np.testing.assert_array_equal(pa.astype(np.float64) * f, pb.astype(np.float64))
    i0.close(); i1.close()


# ======================================================================================================================
# C. real-valued data: derived bounds
# ======================================================================================================================
REPORT = {}


def _stat(form, dtype, name):
    return REPORT.setdefault((form, fc.type_name(dtype), name), fc.Stats())


@TYPES
@pytest.mark.parametrize("name,metric", [("deep", "l2"), ("deep", "mips"), ("t2i", "mips"), ("t2i", "l2"), ("offset", "l2"),
                                         ("offset", "mips")])
def test_real_valued_within_derived_bounds(oracle, dtype, name, metric):
    n, nq = 6000, 64
    X, Q = fc.real_set(name, n, nq, dtype)
    l2 = metric == "l2"
    ix = DeviceIndex(X, max_degree=8, metric=metric)
    ref = fc.ref_matrix(Q, X, metric)
    gform, dform = fc.gather_form(metric), fc.dense_form(dtype, metric)
    gtol = fc.tolerances(Q, X, metric, gform, ref=ref if l2 else None)
    dtol = gtol if dform == gform else fc.tolerances(Q, X, metric, dform)
    gs, ds = _stat(gform, dtype, name), _stat(dform, dtype, name)
    rng = np.random.default_rng(0)
    # gather kernels
    a = rng.integers(0, n, 500).astype(np.uint32); b = rng.integers(0, n, 500).astype(np.uint32)
    a[:3] = [n // 5, 1, 9]; b[:3] = [n // 2, n - 1, 9]                  # the duplicated rows, a row with itself
    fc.check_dists(ix.pair_distances(a, b), fc.ref_pairs(X[a], X[b], metric), fc.tolerances_pairs(X[a], X[b], metric, gform), l2,
                   stats=gs, what="pair_distances")
    ids = np.concatenate([rng.integers(0, n, 200), [n // 5, n // 2]]).astype(np.uint32)
    fc.check_dists(ix.query_distances(Q, ids), ref[:, ids], gtol[:, ids], l2, stats=gs, what="query_distances")
    pool = np.setdiff1d(np.arange(n), [n // 2, n // 5])
    cand = np.stack([rng.choice(pool, 80, replace=False) for _ in range(nq)]).astype(np.uint32)
    cand[:, 3] = n // 2; cand[:, 50] = n // 5
    ri, rd = ix.rerank(Q, cand, None, 10, resort=True)
    masked = np.full_like(ref, np.inf)
    np.put_along_axis(masked, cand.astype(np.int64), np.take_along_axis(ref, cand.astype(np.int64), 1), 1)
    fc.check_topk(ri, rd, masked, gtol, l2, stats=gs, what="rerank")
    # dense kernels
    for k in (10, 100):
        bi, bd = ix.bruteforce_knn(Q, k)
        fc.check_topk(bi, bd, ref, dtol, l2, stats=ds, what=f"bruteforce k={k}")
    leaf = np.unique(np.concatenate([rng.choice(n, 700, replace=False), [n // 5, n // 2, 1, n - 1]])).astype(np.uint32)
    li, ld = ix.leaf_knn(leaf, 10)
    lref = fc.ref_matrix(X[leaf], X[leaf], metric)
    ltol = fc.tolerances(X[leaf], X[leaf], metric, dform, ref=lref if dform == "diff" else None)
    local = np.searchsorted(leaf, li)                                  # leaf is sorted: global id order == local order
    assert (leaf[local] == li).all()
    fc.check_topk(local, ld, lref, ltol, l2, exclude=np.arange(len(leaf)), stats=ds, what="leaf_knn")
    ix.close()
    print(f"\n[fast-float] {name:6s} {fc.type_name(dtype):8s} {metric:4s} gather({gform}): {gs}; dense({dform}): {ds}")


@TYPES
@pytest.mark.parametrize("name,metric", [("deep", "l2"), ("t2i", "mips"), ("offset", "l2")])
def test_real_valued_beam_search_distances(oracle, dtype, name, metric):
    """every returned distance is within the derived bound of the float64 distance of ITS id, rows are sorted (the statistical
    comparison with the oracle's ids stays in test_build_gpu.py / test_bf16_gpu.py)"""
    n, nq = 6000, 200
    X, Q = fc.real_set(name, n, nq, dtype)
    G, _ = oracle.vamana_build(X, 32, 64, _alpha(metric), seed=5, metric=metric)
    ix = DeviceIndex(X, G, metric=metric)
    ref = fc.ref_matrix(Q, X, metric)
    tol = fc.tolerances(Q, X, metric, fc.gather_form(metric), ref=ref if metric == "l2" else None)
    st = _stat(fc.gather_form(metric), dtype, name)
    for beam in (64, 100, 300):
        r = ix.batch_search(Q, k=10, beam=beam, out_k=beam)
        for i in range(nq):
            m = int(r["frontier_size"][i])
            ids, dd = r["ids"][i, :m].astype(np.int64), r["dists"][i, :m].astype(np.float64)
            assert (ids < n).all() and len(np.unique(ids)) == m
            fc.check_dists(dd, ref[i, ids], tol[i, ids], metric == "l2", stats=st, what=f"beam {beam} query {i}")
            dif = np.diff(dd)
            assert (dif >= 0).all() and (np.diff(ids)[dif == 0] > 0).all(), f"beam {beam} query {i}: row not sorted by (dist, id)"
    ix.close()
    print(f"\n[fast-float] {name:6s} {fc.type_name(dtype):8s} {metric:4s} beam search: {st}")


def test_real_valued_report():
    """the largest figures seen above, per (kernel form, type, data set); reports against the float64 reference, the asserted
    bounds are the derived ones"""
    print("\n[fast-float] form  type     set     max|err|/tol  max rel err")
    for (form, t, name), st in sorted(REPORT.items()):
        print(f"[fast-float] {form:5s} {t:8s} {name:7s} {st.err_over_tol:12.3g} {st.rel:12.3g}")
        assert st.err_over_tol <= 1.0
