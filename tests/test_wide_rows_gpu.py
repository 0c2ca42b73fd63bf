"""Adjacency rows wider than one 64-lane wavefront (gstride > 64) in every kernel that walks a row: the multi-pass loops of
the search kernels (register-frontier beam 64, two-entries-per-lane beam 128 with the filter in LDS and in HBM, the generic
kernel with the filter in LDS and in HBM, its sketch-filtered variant), the BFS range search, robustPrune, the builders'
reverse-edge append, re-prune, row scatter and neighbour sort, and the HCNNG edge append.

Every comparison is bit for bit against the CPU oracle (tests/oracle_api.py) on integer-valued data, where any summation order
is exact.  The cases are those of tests/wide_cases.py; tests/test_wide_cases_cpu.py shows on the CPU that each of them really
walks rows wider than a wave."""
import numpy as np
import pytest

import filtered_ref
import wide_cases as wc
from parlayann_amd import DeviceIndex, PannError, _capi, quantize
from parlayann_amd import sketch as sk
from test_build_gpu import _norm
from test_search_gpu import _compare

pytestmark = pytest.mark.gpu
PAD = 0xFFFFFFFF
LAYOUTS = list(wc.LAYOUTS)
# b64 (16, 64), b128 with the table in LDS (100, 128), the generic kernel with the table in HBM (300)
BEAMS = (16, 64, 100, 128, 300)
# every layout at 65 and 129; 80 (a multiple of 16) and 200 (four passes) on the uint8 layout
LAYOUT_WIDTHS = [(lay, w) for lay in LAYOUTS for w in (65, 129)] + [("u8", 80), ("u8", 200)]
LW_IDS = [f"{a}-{b}" for a, b in LAYOUT_WIDTHS]


def _index(layout, width):
    X, Q, G, metric = wc.case(layout, width)
    return X, Q, G, metric, DeviceIndex(X, G, metric=metric)


# ---- 3. search kernels --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,width", LAYOUT_WIDTHS, ids=LW_IDS)
def test_every_frontier_kernel(oracle, layout, width):
    X, Q, G, metric, ix = _index(layout, width)
    try:
        for beam in BEAMS:
            kw = dict(k=10, beam=beam, cut=1.35, out_k=beam, visited_cap=2048)
            o = oracle.batch_search(X, G, queries=Q, metric=metric, **kw)
            assert o["rc"] == 0
            _compare(o, ix.batch_search(Q, **kw), visited=True)
        # three visits from the full-degree start: the degree_sum no count of single passes explains (test_wide_cases_cpu)
        o = oracle.batch_search(X, G, queries=Q, metric=metric, **wc.SHORT_SEARCH)
        _compare(o, ix.batch_search(Q, **wc.SHORT_SEARCH), visited=True)
    finally:
        ix.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_degree_limit_at_the_pass_boundary(oracle, layout):
    """degree_limit on either side of each pass boundary of a three-pass row, and the limits at which the narrow-row kernels
    switch their two-vertex paths on and off (limit >= 2 * beam, nvis < limit), which the wide path must ignore"""
    X, Q, G, metric, ix = _index(layout, 129)
    try:
        variants = [dict(degree_limit=dl) for dl in (63, 64, 65, 127, 128, 129, 500)]
        variants += [dict(degree_limit=100, limit=lim) for lim in (20, 127, 128)]
        for beam in (64, 100):
            for v in variants:
                kw = dict(k=10, beam=beam, cut=1.35, out_k=beam, visited_cap=2048, **v)
                o = oracle.batch_search(X, G, queries=Q, metric=metric, **kw)
                try:
                    _compare(o, ix.batch_search(Q, **kw), visited=True)
                except AssertionError as e:
                    raise AssertionError(f"beam {beam} {v}: {e}") from None
    finally:
        ix.close()


@pytest.mark.parametrize("layout,width", [(lay, w) for lay in LAYOUTS for w in (65, 129)],
                         ids=[f"{lay}-{w}" for lay in LAYOUTS for w in (65, 129)])
def test_builders_mode_skips_the_own_vertex(oracle, layout, width):
    """query_ids, k = 0, cut 0, visited lists: the builder's searches.  The planted rows hold their own id in a column >= 64,
    and they are among the queries: the own vertex is skipped in the later passes too."""
    X, Q, G, metric, ix = _index(layout, width)
    try:
        planted = wc.planted_rows(G)
        qids = np.concatenate([planted, np.arange(5, len(X), 31, dtype=np.uint32)]).astype(np.uint32)
        for beam in (64, 128, 200):
            kw = dict(query_ids=qids, k=0, beam=beam, cut=0.0, out_k=beam, visited_cap=2048)
            o = oracle.batch_search(X, G, metric=metric, **kw)
            _compare(o, ix.batch_search(**kw), visited=True)
    finally:
        ix.close()


@pytest.mark.parametrize("beam", [90, 100, 128])
@pytest.mark.parametrize("layout,width", [(lay, w) for lay in ("u8", "f32") for w in (65, 129)],
                         ids=[f"{lay}-{w}" for lay in ("u8", "f32") for w in (65, 129)])
def test_large_batches_beam_65_to_128(oracle, layout, width, beam):
    """more than 2048 queries: at beams 100 (second frontier slot partly filled) and 128 the two-entries-per-lane kernel keeps
    its filter table split between HBM and LDS (persistent blocks); at beam 90 the table is 8 KB and stays in LDS.  Results and
    counters do not depend on where the table lives."""
    X, _, G, metric, ix = _index(layout, width)
    try:
        nq = 2100
        dtype, d, _ = wc.LAYOUTS[layout]
        Q = wc.rows_of(nq, d, dtype, 777)
        kw = dict(k=10, beam=beam, cut=1.35, out_k=beam)
        _compare(oracle.batch_search(X, G, queries=Q, metric=metric, **kw), ix.batch_search(Q, **kw))
        qid = (np.arange(nq, dtype=np.uint32) * 7) % len(X)
        qid[:wc.N_PLANTED] = wc.planted_rows(G)[:wc.N_PLANTED]
        kw = dict(query_ids=qid, k=0, beam=beam, cut=0.0, out_k=beam, visited_cap=4 * beam)
        _compare(oracle.batch_search(X, G, metric=metric, **kw), ix.batch_search(**kw), visited=True)
    finally:
        ix.close()


FIELDS = ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_per_query_starts(oracle, layout):
    X, Q, G, metric, ix = _index(layout, 129)
    try:
        rng = np.random.default_rng(3)
        starts = np.stack([rng.choice(len(X), 3, replace=False) for _ in range(len(Q))]).astype(np.uint32)
        starts[::2, 1] = 0                                     # half of the queries also start at the full-degree vertex
        for beam in (64, 100):
            kw = dict(k=10, beam=beam, cut=1.35, out_k=beam)
            g = ix.batch_search(Q, starts=starts, **kw)
            for i in range(len(Q)):
                o = oracle.batch_search(X, G, queries=Q[i:i + 1], starts=starts[i], metric=metric, **kw)
                for f in FIELDS:
                    assert np.array_equal(o[f][0].view(np.uint32), g[f][i].view(np.uint32)), (beam, i, f)
    finally:
        ix.close()


_narrow = {}


def _narrow_graph(oracle, layout):
    if layout not in _narrow:
        X, Q, metric = wc.layout_data(layout)
        _narrow[layout] = oracle.vamana_build(X, 32, 64, 1.2 if metric == "l2" else 1.0, seed=7, metric=metric)[0]
    return _narrow[layout]


@pytest.mark.parametrize("graph", ["narrow", "wide129"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_many_starts_take_the_generic_kernel_with_its_table_in_lds(oracle, layout, graph):
    """65 .. 128 start points: the two-entries-per-lane kernel takes at most 64, so the generic kernel runs with its filter
    table in LDS -- on rows of one pass (max_deg 32) and of three"""
    X, Q, metric = wc.layout_data(layout)
    G = _narrow_graph(oracle, layout) if graph == "narrow" else wc.case(layout, 129)[2]
    ix = DeviceIndex(X, G, metric=metric)
    try:
        rng = np.random.default_rng(11)
        for nst, beam in ((70, 100), (70, 128), (65, 65)):
            starts = rng.choice(np.arange(1, len(X)), nst - 1, replace=False).astype(np.uint32)
            starts = np.concatenate([starts[:nst // 2], [0], starts[nst // 2:]]).astype(np.uint32)
            assert len(np.unique(starts)) == nst
            kw = dict(k=10, beam=beam, cut=1.35, out_k=beam, visited_cap=2048, starts=starts)
            o = oracle.batch_search(X, G, queries=Q, metric=metric, **kw)
            assert o["rc"] == 0
            _compare(o, ix.batch_search(Q, **kw), visited=True)
    finally:
        ix.close()


@pytest.mark.parametrize("beam", [64, 200])
@pytest.mark.parametrize("layout,kind", [("i8", "mips_bit"), ("u8", "euclid_bit")])
def test_sketch_filtered_search(layout, kind, beam):
    """pann_batch_search_filtered on three-pass rows against the Python checker, pruned_cmps included.  The sketches are made
    from the float copy of the (integer-valued) points."""
    X, Q, G, metric = wc.case(layout, 129)
    nq = 24                                                    # the checker is plain Python
    Xf, Qf = X.astype(np.float32), Q[:nq].astype(np.float32)
    p = sk.sketch_params_numpy(Xf, kind)
    S, SQ = sk.sketch_rows_numpy(Xf, p), sk.sketch_rows_numpy(Qf, p)
    qp = dict(k=10, beam=beam, cut=1.35)
    ix, src = DeviceIndex(X, G, metric=metric), DeviceIndex(Xf, max_degree=4, metric=metric)
    try:
        pd = sk.sketch_params(src, kind)
        assert (pd.kind, pd.dims, pd.median) == (p.kind, p.dims, p.median) and np.float32(pd.cut) == np.float32(p.cut)
        sk.attach_sketch(ix, src, pd)
        sq = sk.sketch_rows(Qf, pd)
        np.testing.assert_array_equal(sq, SQ)
        qids = np.concatenate([wc.planted_rows(G)[:8], (17 + 331 * np.arange(16)) % len(X)]).astype(np.uint32)
        for form in ("ext", "ids"):
            a = dict(queries=Q[:nq], sketch_queries=SQ) if form == "ext" else dict(query_ids=qids)
            ref = filtered_ref.filtered_batch_search(X, G, metric=metric, out_k=beam, visited_cap=2048, use_filtering=True,
                                                     sketches=S, sketch_params=p, **a, **qp)
            assert (ref["sketch_dropped"] > 0).any() and (ref["pruned_cmps"] > ref["dist_cmps"]).any()     # it really filters
            assert (ref["degree_sum"] > 0).all()
            if form == "ext":
                g = ix.batch_search_filtered(Q[:nq], sq, out_k=beam, visited_cap=2048, **qp)
            else:
                g = ix.batch_search_filtered(query_ids=qids, out_k=beam, visited_cap=2048, **qp)
            for f in FIELDS + ("pruned_cmps",):
                assert np.array_equal(g[f], ref[f]), (form, f, g[f], ref[f])
            for i in range(len(ref["visited_count"])):
                v = int(ref["visited_count"][i])
                assert np.array_equal(g["visited_ids"][i, :v], ref["visited_ids"][i, :v]), (form, i)
                assert np.array_equal(g["visited_dists"][i, :v], ref["visited_dists"][i, :v]), (form, i)
    finally:
        ix.close(); src.close()


def test_fused_rerank_equals_the_composition():
    """search_rerank with a float32 handle and its EUCLID_U8 copy carrying a three-pass graph (copy_graph) equals
    quantize_rows -> batch_search -> rerank"""
    X, Q, G, metric = wc.case("f32", 129)
    k, rf = 10, 100
    full = DeviceIndex(X, G)
    quant, qparams = full.quantized("euclid_u8", copy_graph=True)
    try:
        np.testing.assert_array_equal(quant.get_graph(), _norm(G))
        for beam in (64, 100):
            # the composition, as test_search_rerank_gpu.Case.compose builds it
            qq = quantize.device_quantize_rows(Q, qparams, normalize_first=False)
            r = quant.batch_search(qq, k=k, beam=beam, out_k=beam)
            counts = np.minimum(r["frontier_size"], k * rf).astype(np.uint32)
            assert int(counts.max()) == beam
            ids, dists = full.rerank(Q, r["ids"], counts, k, resort=True)
            exp = {"ids": ids, "dists": dists, "frontier_size": r["frontier_size"], "visited_count": r["visited_count"],
                   "dist_cmps": r["dist_cmps"]}
            got = full.search_rerank(quant, qparams, Q, k=k, beam=beam, rerank_factor=rf)
            for f, e in exp.items():
                assert got[f].dtype == e.dtype and np.array_equal(got[f].view(np.uint32), e.view(np.uint32)), (beam, f)
            assert int(got["status"][0]) == 0
    finally:
        full.close(); quant.close()


def test_four_bit_rows(oracle):
    """the uint8 layout's three-pass graph set on a PANN_U4 handle, against the oracle on the unpacked nibbles"""
    from test_quant4_gpu import _same_search
    X, Q, G, metric = wc.case("u8", 129)
    V, Vq = (X >> 4).astype(np.uint8), (Q >> 4).astype(np.uint8)
    ix4 = DeviceIndex.from_packed(quantize.pack_nibbles(V), V.shape[1], "u4", max_degree=129)
    try:
        ix4.set_graph(G)
        Pq = quantize.pack_nibbles(Vq)
        qids = wc.planted_rows(G)
        for beam in (64, 100):
            kw = dict(k=10, beam=beam, cut=1.35, out_k=beam, visited_cap=2048)
            o = oracle.batch_search(V, G, queries=Vq, **kw)
            assert (o["degree_sum"] > 64 * 2).all()
            _same_search(o, ix4.batch_search(Pq, **kw), 1.0)
            _same_search(oracle.batch_search(V, G, query_ids=qids, **kw), ix4.batch_search(query_ids=qids, **kw), 1.0)
    finally:
        ix4.close()


# ---- 4. range search and graph plumbing ---------------------------------------------------------------------------------------

def _check_range(o, g, what, cmps=True):
    np.testing.assert_array_equal(o["counts"], g["counts"], err_msg=what)
    np.testing.assert_array_equal(o["truncated"], g["truncated"], err_msg=what)
    np.testing.assert_array_equal(o["ids"], g["ids"], err_msg=what)
    if cmps:
        ok = o["truncated"] == 0                # a truncated query stops early; where exactly is not part of the contract
        np.testing.assert_array_equal(o["dist_cmps"][ok], g["dist_cmps"][ok], err_msg=what)


@pytest.mark.parametrize("layout,width", [(lay, w) for lay in ("u8", "f16") for w in (65, 129, 200)],
                         ids=[f"{lay}-{w}" for lay in ("u8", "f16") for w in (65, 129, 200)])
def test_range_search(oracle, layout, width):
    X, Q, G, metric, ix = _index(layout, width)
    try:
        so = oracle.batch_search(X, G, queries=Q, k=10, beam=32, metric=metric)
        seeds = ix.batch_search(Q, k=10, beam=32)["ids"]
        np.testing.assert_array_equal(seeds, so["ids"])
        shared = np.concatenate([[0], seeds[0], seeds[1][:3]]).astype(np.uint32)          # one start list for every query
        for rank in (10, 60):
            r2 = wc.range_radius(oracle, X, Q, rank, metric)
            for starts, name in ((seeds, "per-query"), (shared, "shared")):
                o = oracle.range_search(X, G, starts, r2, 2048, queries=Q, metric=metric)
                assert o["counts"].max() > 5 and not o["truncated"].any()
                _check_range(o, ix.range_search(starts, r2, 2048, queries=Q), f"rank {rank} {name}")
        assert (o["dist_cmps"] > 64).any()
        r2 = wc.range_radius(oracle, X, Q, 300, metric)          # truncation at 50 results
        o = oracle.range_search(X, G, seeds, r2, 50, queries=Q, metric=metric)
        assert o["truncated"].any() and (o["counts"][o["truncated"] != 0] == 50).all()
        _check_range(o, ix.range_search(seeds, r2, 50, queries=Q), "truncated")
        # base-point queries: the own vertex is skipped, the planted rows name it in their later passes
        qid = np.concatenate([wc.planted_rows(G), np.arange(3, 300, 7, dtype=np.uint32)]).astype(np.uint32)
        st = np.zeros((len(qid), 2), np.uint32); st[:, 1] = G[qid, 1]
        o = oracle.range_search(X, G, st, r2, 2048, query_ids=qid, metric=metric)
        _check_range(o, ix.range_search(st, r2, 2048, query_ids=qid), "base-point")
    finally:
        ix.close()


@pytest.mark.parametrize("layout", ["u8", "f16"])
def test_range_query(oracle, layout):
    X, Q, G, metric, ix = _index(layout, 129)
    try:
        r = float(np.median(oracle.bruteforce_knn(X, Q, 40, metric)[1][:, -1]))
        qid = np.concatenate([wc.planted_rows(G), (np.arange(60, dtype=np.uint32) * 7) % len(X)]).astype(np.uint32)
        for beam in (48, 128):
            for cap in (2048, 50):
                for kw in (dict(queries=Q), dict(query_ids=qid)):
                    what = f"beam {beam} cap {cap} {'external' if 'queries' in kw else 'base-point'}"
                    g = ix.range_query(radius=r, beam=beam, max_results=cap, **kw)
                    so = oracle.batch_search(X, G, k=beam, beam=beam, cut=0.0, metric=metric, **kw)
                    o = oracle.range_search(X, G, so["ids"], r, cap, metric=metric, **kw)
                    _check_range(o, g, what)
                    np.testing.assert_array_equal(g["search_cmps"], so["dist_cmps"], err_msg=what)
                    np.testing.assert_array_equal(g["visited"], so["visited_count"], err_msg=what)
    finally:
        ix.close()


def test_graph_plumbing_on_a_width_200_slab(oracle):
    X, Q, G, metric = wc.case("u8", 200)
    n = len(X)
    ix = DeviceIndex(X, max_degree=200)
    try:
        ix.set_graph(G)
        np.testing.assert_array_equal(ix.get_graph(), _norm(G))
        # update_rows with rows of degree 0, 64, 65 and 200, then search parity
        rng = np.random.default_rng(5)
        ids = np.array([0, 7, 1500, n - 1], np.uint32)
        rows = np.zeros((4, 201), np.uint32)
        for r, dv in enumerate((200, 0, 64, 65)):
            rows[r, 0] = dv
            rows[r, 1:1 + dv] = rng.choice(n, dv, replace=False)
        ix.update_rows(ids, rows)
        G2 = G.copy(); G2[ids] = rows
        np.testing.assert_array_equal(ix.get_graph(), _norm(G2))
        for beam in (64, 100):
            kw = dict(k=10, beam=beam, cut=1.35, out_k=beam, visited_cap=2048)
            _compare(oracle.batch_search(X, G2, queries=Q, **kw), ix.batch_search(Q, **kw), visited=True)
        # an id >= n in column 150 of one row: refused, that row left empty, the others intact
        bad = G.copy(); bad[0, 0] = 200; bad[0, 150] = n
        with pytest.raises(PannError) as e:
            ix.set_graph(bad)
        assert e.value.code == _capi.PANN_ERR_BAD_ARG
        exp = _norm(G); exp[0] = 0
        np.testing.assert_array_equal(ix.get_graph(), exp)
        ix.clear_graph()
        assert not ix.get_graph().any()
    finally:
        ix.close()


# ---- 5. builders --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,max_deg", [(65, 65), (96, 96), (200, 129)])
@pytest.mark.parametrize("layout", ["u8", "i8"])
def test_robust_prune_batch(oracle, layout, R, max_deg):
    """owners that already hold rows of degree 0, 64, 65 and max_deg (add_out_nbrs joins them to the candidates), candidate
    lists of 300 to 1500 ids with duplicates and the owner itself, with and without the caller's distances"""
    X, Q, metric = wc.layout_data(layout)
    n = len(X)
    G = wc.wide_graph(X, max_deg, 300 + max_deg, metric)
    deg = G[:, 0]
    rng = np.random.default_rng(R)
    owners = np.concatenate([rng.choice(np.flatnonzero(deg == dv), 6, replace=False) for dv in (0, 64, 65, max_deg)])
    owners = np.concatenate([owners, wc.planted_rows(G)[:4]]).astype(np.uint32)
    cands = []
    for i, p in enumerate(owners):
        c = rng.choice(n, int(rng.integers(300, 1501)), replace=False).astype(np.uint32)
        if i % 3 == 0:
            c = np.concatenate([c, c[:3], [p]]).astype(np.uint32)
        cands.append(c)
    off = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.uint64)
    cid = np.concatenate(cands).astype(np.uint32)
    cd = np.concatenate([[oracle.distance(X[j], X[p], metric) for j in c] for c, p in zip(cands, owners)]).astype(np.float32)
    alpha = 1.2 if metric == "l2" else 1.0
    ix = DeviceIndex(X, G, metric=metric)
    try:
        for add in (True, False):
            for with_d in (True, False):
                ro, dco = oracle.robust_prune_batch(X, G, owners, cid, cd if with_d else None, off, alpha, R, add=add, metric=metric)
                rg, dcg = ix.robust_prune_batch(owners, cid, off, alpha, R, cand_dists=cd if with_d else None, add_out_nbrs=add)
                np.testing.assert_array_equal(ro, rg, err_msg=f"add {add} dists {with_d}")
                np.testing.assert_array_equal(dco, dcg, err_msg=f"add {add} dists {with_d}")
        if metric == "l2":
            assert (ro[:, 0] > 64).any()                        # alpha 1.2 keeps rows wider than a wave
    finally:
        ix.close()


def _stats_equal(so, sg):
    assert (int(so[0]), int(so[1]), int(so[2])) == (sg.search_dist_cmps, sg.prune_dist_cmps, sg.visited_total)


def test_insert_batch_into_a_wide_graph(oracle):
    """500 ids into the oracle-built R = 96 graph: the reverse-edge append onto rows that end below, at and above R, and the
    re-prune of those that overflow"""
    X, G, batch, R, L, alpha = wc.insert_case(oracle)        # test_wide_cases_cpu: rows end at 95, at 96 and overflow
    Go = G.copy()
    so = oracle.vamana_insert_batch(X, Go, batch, R, L, 1.2)
    assert not np.array_equal(Go, G)
    ix = DeviceIndex(X, G)
    try:
        sg = ix.vamana_insert_batch(batch, R, L, 1.2)
        np.testing.assert_array_equal(_norm(Go), _norm(ix.get_graph()))
        _stats_equal(so, sg)
    finally:
        ix.close()


@pytest.mark.parametrize("name", list(wc.VAMANA_BUILDS))
def test_vamana_build(oracle, name):
    """graph and counters of a build whose rows outgrow a wave; with L = 128 the builder prepares filter codes that searches on
    wide rows cannot use, so nothing may change.  Then the neighbour sort on its own."""
    dtype, R, L, alpha, passes, seed = wc.VAMANA_BUILDS[name]
    X, Gs, ss = wc.vamana_oracle_build(name, sort_neighbors=True)
    _, Gu, su = wc.vamana_oracle_build(name, sort_neighbors=False)
    ix = DeviceIndex(X, max_degree=R)
    try:
        sg = ix.vamana_build(R, L, alpha, num_passes=passes, seed=seed, sort_neighbors=True)
        np.testing.assert_array_equal(_norm(Gs), _norm(ix.get_graph()))
        _stats_equal(ss, sg)
        ix.clear_graph()
        sg = ix.vamana_build(R, L, alpha, num_passes=passes, seed=seed, sort_neighbors=False)
        np.testing.assert_array_equal(_norm(Gu), _norm(ix.get_graph()))
        _stats_equal(su, sg)
        ix.vamana_sort_neighbors()
        np.testing.assert_array_equal(_norm(Gs), _norm(ix.get_graph()))
    finally:
        ix.close()


def test_single_batch_build_from_random_rows_wider_than_a_wave(oracle):
    X = wc.build_points(np.uint8)
    Go, so = oracle.vamana_build(X, 96, 128, 1.2, num_passes=1, seed=7, single_batch=70)
    ix = DeviceIndex(X, max_degree=96)
    try:
        sg = ix.vamana_build(96, 128, 1.2, num_passes=1, seed=7, single_batch=70)
        np.testing.assert_array_equal(_norm(Go), _norm(ix.get_graph()))
        _stats_equal(so, sg)
    finally:
        ix.close()


@pytest.mark.parametrize("dtype", [np.uint8, np.float16], ids=["u8", "f16"])
@pytest.mark.parametrize("name,width", [("30x100x3", 90), ("24x60x4", 96)])
def test_hcnng_build(oracle, name, width, dtype):
    X, Go = wc.hcnng_oracle_build(name, dtype)
    c, s, m, seed = wc.HCNNG_BUILDS[name]
    ix = DeviceIndex(X, max_degree=width)
    try:
        ix.hcnng_build(c, s, m, seed=seed)
        np.testing.assert_array_equal(ix.get_graph(), Go)
    finally:
        ix.close()


def test_hcnng_build_appends_to_a_graph_it_finds(oracle):
    """a second forest onto a handle that holds the first (max_degree 180): rows grow from below a wave to above two"""
    X, G1 = wc.hcnng_oracle_build("30x100x3", np.uint8)
    c2, s2, m2, seed2 = wc.HCNNG_BUILDS["24x60x4"]
    Go = np.zeros((len(X), 181), np.uint32)
    Go[:, :91] = G1
    ix = DeviceIndex(X, Go.copy())
    try:
        wc.hcnng_oracle_append(X, Go, c2, s2, m2, seed2 + 1)
        assert Go[:, 0].max() > 128
        ix.hcnng_build(c2, s2, m2, seed=seed2 + 1)
        np.testing.assert_array_equal(ix.get_graph(), _norm(Go))
    finally:
        ix.close()
