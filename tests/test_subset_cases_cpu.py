"""CPU-only: the numpy restatement of the subset rule (tests/subset_ref.py) agrees with a plain per-row loop, and the case tables of
tests/subset_cases.py reach the regimes they are there for -- so that no device test of tests/test_subset_gpu.py passes vacuously."""
import numpy as np
import pytest

import subset_cases as sc
import subset_ref as sr


def _inputs(layout, n, with_sketch=False):
    X, G, L = sc.case(layout, n)
    sk = np.random.default_rng(9).integers(0, 256, (n, 16), dtype=np.uint8) if with_sketch else None
    return sc.points_bytes(X), G, L, sk


@pytest.mark.parametrize("mask", sc.mask_names(sc.N_SMALL))
def test_vectorised_reference_equals_the_loop_small(mask):
    P, G, L, sk = _inputs("u8", sc.N_SMALL, with_sketch=True)
    a = sc.masks(sc.N_SMALL)[mask]
    n_out = 5 if mask == "none" else (0 if mask != "1pct" else 9)
    assert sr.same(sr.subset_ref(P, G, L, sk, a, n_out), sr.subset_ref_loop(P, G, L, sk, a, n_out)) is None
    assert sr.same(sr.subset_ref(P, G, None, None, a, n_out, copy_graph=False),
                   sr.subset_ref_loop(P, G, None, None, a, n_out, copy_graph=False)) is None


@pytest.mark.parametrize("layout", ["u4", "u8_w65"])
def test_vectorised_reference_equals_the_loop_big(layout):
    n = sc.N_BIG
    P, G, L, sk = _inputs(layout, n)
    for mask in ("50pct", "dead_bits", "block_edges"):
        a = sc.masks(n)[mask]
        assert sr.same(sr.subset_ref(P, G, L, sk, a), sr.subset_ref_loop(P, G, L, sk, a)) is None, mask
    assert sr.same(sr.subset_ref(P, G, L, sk, None, n + 3), sr.subset_ref_loop(P, G, L, sk, None, n + 3)) is None


def test_masks_are_what_their_names_say():
    for n in (sc.N_BIG, sc.N_BLOCK, sc.N_SMALL):
        m = sc.masks(n)
        K = {k: sr.kept_ids(v, n) for k, v in m.items()}
        assert all(len(v) == (n + 31) // 32 for v in m.values())
        assert len(K["all"]) == n and len(K["none"]) == 0
        assert list(K["only_first"]) == [0] and list(K["only_last"]) == [n - 1]
        assert 0.4 * n < len(K["50pct"]) < 0.6 * n
        assert 1 <= len(K["1pct"]) <= 1 + 0.03 * n                                    # the draw, and the one forced bit
        if n & 31:
            assert not np.array_equal(m["dead_bits"], m["50pct"]) and np.array_equal(K["dead_bits"], K["50pct"])
            assert int(m["dead_bits"][-1]) >> (n & 31) == (1 << (32 - (n & 31))) - 1
        else:
            assert "dead_bits" not in m
    assert list(sr.kept_ids(sc.masks(sc.N_BIG)["block_edges"], sc.N_BIG)) == [8191, 8192]
    assert (sc.N_BIG + 31) // 32 == 626 and sc.N_BIG & 31 == 11 and sc.N_BLOCK // 32 == 256


@pytest.mark.parametrize("layout", list(sc.LAYOUTS))
def test_graphs_are_well_formed_and_reach_their_regimes_under_50pct(layout):
    n = sc.N_BIG
    G = sc.graph(layout, n)
    max_deg = sc.LAYOUTS[layout][3]
    deg = G[:, 0].astype(np.int64)
    cols = np.arange(max_deg)[None, :]
    live = cols < deg[:, None]
    assert set(np.unique(deg)) == set(sc.degree_choices(max_deg))
    assert (G[:, 1:][~live] == 0).all() and (G[:, 1:][live] < n).all()
    assert not (live & (G[:, 1:] == np.arange(n)[:, None])).any()                     # never the row's own id
    srt = np.sort(np.where(live, G[:, 1:].astype(np.int64), -1 - cols), axis=1)
    assert (np.diff(srt, axis=1) != 0).all()                                         # distinct
    keep = sc.bool_masks(n)["50pct"]
    nb_kept = live & keep[G[:, 1:]]
    lost = (live & ~nb_kept).sum(axis=1)
    rows = np.flatnonzero(keep)
    assert ((deg[rows] > 0) & (lost[rows] == deg[rows])).any()                       # a kept row loses every neighbour
    assert ((deg[rows] > 0) & (lost[rows] == 0)).any()                               # ... one loses none
    assert (live & ~keep[G[:, 1:]])[rows].any()                                      # a dropped id is the neighbour of a kept row
    if layout in sc.WIDE:
        assert sc.graph(layout, n).shape[1] - 1 > sc.WAVE
        first, later = slice(0, sc.WAVE), slice(sc.WAVE, None)
        late_loss = nb_kept[:, first].all(axis=1) & (live & ~nb_kept)[:, later].any(axis=1)
        late_keep = ~nb_kept[:, first].any(axis=1) & nb_kept[:, later].any(axis=1)
        assert late_loss[rows].sum() >= sc.N_PLANTED and late_keep[rows].sum() >= sc.N_PLANTED
        p = sc.planted(layout, n)
        assert late_loss[p["late_loss"]].all() and late_keep[p["late_keep"]].all() and keep[p["late_loss"]].all()
        # what the reference makes of them: 64 neighbours survive the first pass and none a later one / none and max_deg - 64
        ref = sr.subset_ref(sc.points_bytes(sc.points(layout, n)), G, None, None, sc.masks(n)["50pct"])
        assert (ref["graph"][ref["old_to_new"][p["late_loss"]], 0] == sc.WAVE).all()
        assert (ref["graph"][ref["old_to_new"][p["late_keep"]], 0] == max_deg - sc.WAVE).all()


def test_u4_rows_keep_the_high_nibble_of_the_last_byte_zero():
    X = sc.points("u4", sc.N_BIG)
    assert X.shape == (sc.N_BIG, 13) and X.dtype == np.uint8 and (X[:, -1] >> 4 == 0).all() and (X[:, :-1] >> 4 != 0).any()
