"""CPU-only: the restatement of the masked fused search (tests/masked_rerank_cases.py) meets every regime a device case of
tests/test_masked_rerank_gpu.py is there for, so that no device test passes vacuously.  Nothing here runs on a GPU: the rule
(DESIGN.md "Masked search on the fused path") is restated with the oracle's quantiser, its Vamana graph and its distances, and
the walk of tests/masked_ref.py."""
import numpy as np
import pytest

import masked_rerank_cases as rc
import masked_ref

SENT = rc.SENT


def test_the_data_is_what_the_cases_say():
    assert rc.N % 32 == 25 and rc.WORDS * 32 - rc.N == 7
    p = rc.pack(rc.mask("zeros", "l2_64"))
    assert p.shape == (rc.WORDS,) and (p[:-1] == 0).all() and p[-1] == 0xFE000000     # only the 7 stray bits are set
    assert rc.pack(rc.mask("rows_differ", "l2_64")).shape == (rc.NQ, rc.WORDS)
    for name in rc.RESTATED:
        slope, offset, Xq, Qq = rc.quantised(name)
        X, Q = rc.data(name)
        assert slope != 1.0 and Xq.dtype == np.uint8 and not np.array_equal(Xq.astype(np.float32), X)   # not a cast
        assert Xq.min() == 0 and Xq.max() == 255
    assert [rc.pool(*s) for s in rc.SWEEP] == [16, 64, 6, 64, 64]
    # row bytes per route: 64 (b64), 96 on a 128-byte stride (generic at beam <= 64), four-bit 64 (b64)
    assert [rc.DATASETS[n][0] * rc.DATASETS[n][2] // 8 for n in ("l2_64", "l2_96", "l2_128_u4")] == [64, 96, 64]


@pytest.mark.parametrize("name", rc.RESTATED)
def test_the_walk_does_not_see_the_mask(name, oracle):
    _, _, Xq, Qq = rc.quantised(name)
    o = oracle.batch_search(Xq, rc.graph(name), queries=Qq, k=10, beam=64, cut=1.35, out_k=64)
    for mkind in ("ones", "rand50", "zeros", "far_only"):
        r = rc.restate(name, 64, 10, 100, mkind)
        for f in ("frontier_size", "visited_count", "dist_cmps"):
            np.testing.assert_array_equal(r[f], o[f], err_msg=f"{mkind} {f}")


@pytest.mark.parametrize("name", rc.RESTATED)
def test_a_five_percent_mask_at_beam_16_leaves_short_and_full_rows(name):
    full = rc.restate(name, 16, 10, 100, "rand5")
    assert (full["result_count"] >= 10).all()                        # without a visit limit no list is shorter than k (SHORT_LIMIT)
    r = rc.restate(name, 16, 10, 100, "rand5", limit=rc.SHORT_LIMIT)
    assert (r["result_count"] < 10).any() and (r["result_count"] >= 10).any()
    short = r["result_count"] < 10
    pad = np.arange(10)[None, :] >= r["result_count"][:, None]
    assert (r["rr_ids"][pad] == SENT).all() and np.isposinf(r["rr_dists"][pad]).all() and pad[short].any()
    assert (r["rr_ids"][~pad] != SENT).all()


@pytest.mark.parametrize("name", rc.RESTATED)
def test_an_all_zero_mask_leaves_every_row_empty(name):
    r = rc.restate(name, 64, 10, 100, "zeros")
    assert (r["result_count"] == 0).all() and (r["allowed_cmps"] == 0).all()
    assert (r["rr_ids"] == SENT).all() and np.isposinf(r["rr_dists"]).all()


@pytest.mark.parametrize("name", rc.RESTATED)
def test_a_pool_of_six_is_cut_from_more_allowed_points(name):
    r = rc.restate(name, 64, 2, 3, "rand50")
    assert rc.pool(64, 2, 3) == 6 and (r["result_count"] == 6).all() and (r["allowed_cmps"] > 6).all()


@pytest.mark.parametrize("name", rc.RESTATED)
def test_the_rerank_changes_the_order_of_the_list(name):
    r = rc.restate(name, 64, 10, 100, "rand50")
    assert (r["result_count"] == 64).all()
    differs = [not np.array_equal(r["rr_ids"][i], r["ids"][i, :10]) for i in range(rc.NQ)]
    assert any(differs)                                              # the exact order is not the quantised order
    for i in range(rc.NQ):                                           # and every reranked id comes from the list
        assert np.isin(r["rr_ids"][i], r["ids"][i]).all()


@pytest.mark.parametrize("name", rc.RESTATED)
def test_masking_is_not_post_filtering_the_plain_result(name):
    """the caller's alternative without the feature: the plain fused call, disallowed ids dropped afterwards"""
    m = rc.mask("rand50", name)
    ids, _, _ = rc.plain_rerank(name, 64, 10, 100)
    r = rc.restate(name, 64, 10, 100, "rand50")
    assert (r["rr_ids"] != SENT).all()                               # the masked rows are full
    for i in range(rc.NQ):
        kept = [a for a in ids[i] if a != SENT and m[a]]
        assert 0 < len(kept) < 10 and list(r["rr_ids"][i, :len(kept)]) == kept       # the post-filter leaves a short prefix of them
    # under far_only even the whole frontier (k = beam = 64: every entry reranked) holds no allowed point at all
    mf = rc.mask("far_only", name)
    wide, _, _ = rc.plain_rerank(name, 64, 64, 100)
    rf = rc.restate(name, 64, 10, 100, "far_only")
    for i in range(rc.NQ):
        assert not [a for a in wide[i] if a != SENT and mf[i][a]] and (rf["rr_ids"][i] != SENT).all()


@pytest.mark.parametrize("name", rc.RESTATED)
def test_far_only_results_come_from_beyond_the_cutoff(name):
    r = rc.restate(name, 64, 10, 100, "far_only")
    assert (r["from_beyond_cutoff"] > 0).any()
    nn = rc.knn_exact(name, 200)
    for i in range(rc.NQ):
        real = r["rr_ids"][i][r["rr_ids"][i] != SENT]
        assert len(real) and not np.isin(real, nn[i]).any()


def test_the_line_walk_overflows_a_small_dropped_list(oracle):
    X, G, Q, allow, Xq, Qq = rc.line_case()
    for beam in (16, 100):
        r = masked_ref.masked_batch_search(Xq, G, allow, queries=Qq, k=1, beam=beam, cut=1.0, out_k=rc.pool(beam, 1, 100))
        assert r["visited_count"].max() > 600                        # far more than the 256 entries a fresh handle has room for
        assert (r["result_count"] > 0).all()
