"""The wide-row cases of tests/wide_cases.py really are wide: asserted on the CPU oracle alone, so that no test of
tests/test_wide_rows_gpu.py can pass without a kernel having walked rows longer than one 64-lane wavefront."""
import numpy as np
import pytest

import wide_cases as wc

PAIRS = [(lay, w) for lay in wc.LAYOUTS for w in wc.WIDTHS]


def test_degree_choices_put_three_of_seven_above_a_wave():
    for w in wc.WIDTHS:
        ch = wc.degree_choices(w)
        assert len(ch) == 7 and max(ch) == w and sum(c > wc.WAVE for c in ch) == 3 and wc.WAVE in ch and 0 in ch
    assert wc.degree_choices(129) == [0, 1, 63, 64, 65, 128, 129]


@pytest.mark.parametrize("layout,width", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_generated_graph_is_wide(oracle, layout, width):
    X, Q, G, metric = wc.case(layout, width)
    n = len(X)
    deg = G[:, 0].astype(np.int64)
    assert G.shape == (n, width + 1) and deg.max() == width and deg[0] == width
    assert set(np.unique(deg)) == set(wc.degree_choices(width))
    assert (deg > wc.WAVE).mean() >= 0.30                      # the draw gives 3/7
    assert (deg == wc.WAVE).mean() >= 0.10                     # 1/7: rows that end exactly at the pass boundary
    cols = np.arange(width)[None, :]
    assert (G[:, 1:][cols < deg[:, None]] < n).all()
    # the planted rows: full degree, own id and a duplicate in slab columns >= 64 (wide_graph says which pass each lands in)
    planted = wc.planted_rows(G)
    assert len(planted) >= wc.N_PLANTED and 0 in planted
    dups = 0
    for v in planted:
        row = G[v, 1:1 + deg[v]]
        tail = G[v, wc.WAVE:1 + deg[v]]
        assert v in tail
        dups += any((row == a).sum() > 1 for a in tail)
    assert dups >= wc.N_PLANTED
    if width >= 80:                                            # both planted ids beyond the first pass: a duplicate across passes
        for v in planted[:wc.N_PLANTED]:
            late = G[v, wc.WAVE + 1:1 + deg[v]]
            assert v in late and np.isin(late, G[v, 1:wc.WAVE + 1]).any(), v
    # every query walks wide rows, at the narrowest beam of the device tests
    o = oracle.batch_search(X, G, queries=Q, k=10, beam=16, cut=1.35, metric=metric, out_k=16, visited_cap=2048)
    for i in range(len(Q)):
        vis = o["visit_order_ids"][i, :o["visited_count"][i]]
        assert (deg[vis] > wc.WAVE).sum() >= 2, i
    # a degree_sum that no count of single passes explains.  At width 65 a row is at most one neighbour wider than a wave, so
    # this needs a search of few visits (the rows of degree 0 and 1 pull the sum down): the limit-3 search of the device test
    s = oracle.batch_search(X, G, queries=Q, metric=metric, **wc.SHORT_SEARCH)
    both = [r["degree_sum"].astype(np.int64) > wc.WAVE * r["visited_count"].astype(np.int64) for r in (o, s)]
    assert both[1].any() and (width == 65 or both[0].any())
    # and in the builder's mode the planted rows are visited by their own queries (start 0 is planted itself)
    b = oracle.batch_search(X, G, query_ids=planted, k=0, beam=64, cut=0.0, metric=metric, out_k=64, visited_cap=2048)
    assert all(0 in b["visit_order_ids"][i, :b["visited_count"][i]] for i in range(len(planted)))


@pytest.mark.parametrize("name,expect_max", [("u8_R96", 96), ("f16_R130", 130)])
def test_vamana_build_inputs_are_wide(name, expect_max):
    X, G, st = wc.vamana_oracle_build(name)
    assert wc.wide_count(G) >= 100 and G[:, 0].max() == expect_max
    if name == "f16_R130":
        assert (G[:, 0] > 128).sum() >= 1                      # rows of three passes
    Xu, Gu, _ = wc.vamana_oracle_build(name, sort_neighbors=False)
    assert np.array_equal(G[:, 0], Gu[:, 0]) and not np.array_equal(G, Gu)      # the final sort really moves neighbours


@pytest.mark.parametrize("name,width", [("30x100x3", 90), ("24x60x4", 96)])
@pytest.mark.parametrize("dtype", [np.uint8, np.float16])
def test_hcnng_build_inputs_are_wide(oracle, name, width, dtype):
    X, G = wc.hcnng_oracle_build(name, dtype)
    assert G.shape[1] == width + 1 and wc.wide_count(G) >= 100


def test_hcnng_oracle_appends_to_an_initial_graph(oracle):
    """the oracle's entry point takes an initial graph: a build onto an empty slab equals the wrapper's, and a second build
    appends to the rows of the first"""
    X, G1 = wc.hcnng_oracle_build("30x100x3", np.uint8)
    c, s, m, seed = wc.HCNNG_BUILDS["30x100x3"]
    np.testing.assert_array_equal(wc.hcnng_oracle_append(X, np.zeros_like(G1), c, s, m, seed), G1)
    G2 = np.zeros((len(X), 181), np.uint32)
    G2[:, :91] = G1
    c2, s2, m2, seed2 = wc.HCNNG_BUILDS["24x60x4"]
    wc.hcnng_oracle_append(X, G2, c2, s2, m2, seed2 + 1)
    assert (G2[:, 0] >= G1[:, 0]).all() and (G2[:, 0] > G1[:, 0]).any() and G2[:, 0].max() > 128
    for v in range(0, len(X), 97):
        assert np.array_equal(G2[v, 1:1 + G1[v, 0]], G1[v, 1:1 + G1[v, 0]])


def test_single_batch_build_input_is_wide(oracle):
    X = wc.build_points(np.uint8)
    G, st = oracle.vamana_build(X, 96, 128, 1.2, num_passes=1, seed=7, single_batch=70)
    assert wc.wide_count(G) >= 100


def test_insert_batch_overflows_rows_of_the_wide_graph(oracle):
    """the batch of test_insert_batch_into_a_wide_graph: with c reverse edges onto a row of degree deg, the row is appended to
    when c + deg <= R and re-pruned otherwise.  Rows must end below R, exactly at R - 1 and R, and overflow."""
    X, G, batch, R, L, alpha = wc.insert_case(oracle)
    rows = oracle.vamana_phase_a(X, G, batch, R, L, alpha)
    live = rows != 0xFFFFFFFF
    deg = G[:, 0].astype(np.int64)
    deg[batch] = live.sum(1)                                   # a batch point's row is replaced before the reverse edges arrive
    c = np.bincount(rows[live], minlength=len(X))
    sums = (c + deg)[c > 0]
    assert (sums > R).sum() >= 10                              # re-pruned
    assert (sums == R).any() and (sums == R - 1).any()         # appended to, ending at 96 and at 95
    assert ((sums > wc.WAVE) & (sums <= R)).sum() >= 100       # appends that write beyond the first pass of the row
    assert (live.sum(1) > wc.WAVE).any()                       # new rows of the batch points wider than a wave (row scatter)


@pytest.mark.parametrize("layout,width", [(lay, w) for lay in ("u8", "f16") for w in (65, 129, 200)])
def test_range_bfs_expands_wide_rows(oracle, layout, width):
    """the BFS expands every vertex it reports (no query of this case is truncated): most queries expand rows wider than a wave"""
    X, Q, G, metric = wc.case(layout, width)
    deg = G[:, 0]
    seeds = oracle.batch_search(X, G, queries=Q, k=10, beam=32, metric=metric)["ids"]
    r = oracle.range_search(X, G, seeds, wc.range_radius(oracle, X, Q, 10, metric), 2048, queries=Q, metric=metric)
    assert not r["truncated"].any()
    wide = np.array([(deg[r["ids"][i, :r["counts"][i]]] > wc.WAVE).sum() for i in range(len(Q))])
    assert (wide >= 1).mean() >= 0.7 and wide.sum() >= 10 * len(Q)
