"""The reference side of tests/test_two_phase_build_gpu.py, asserted on the CPU oracle alone: the oracle-side drivers of
tests/two_phase_cases.py reproduce the oracle's single-process builds for every case and every W, and every case really contains
what it is there for (uneven splits, batches smaller than W, padded and full rows, rows wider than a wave, idle ranks) -- so that
no device test passes vacuously.  The last tests perturb the expected values the way a wrong kernel would and show that the
comparisons of the device test tell the difference."""
import numpy as np
import pytest

import two_phase_cases as tp
from parlayann_amd import from_bf16


@pytest.mark.parametrize("name,W", tp.VAMANA_PAIRS, ids=[f"{a}-W{b}" for a, b in tp.VAMANA_PAIRS])
def test_two_phase_build_equals_single_process_build(oracle, name, W):
    X, metric, R, max_deg, L, alpha, passes, _ = tp.vamana_case(name)
    ms, row_lens, one_id_slice = [], [], False
    for ids, rows, G in tp.oracle_two_phase_build(oracle, X, R, L, alpha, passes, tp.SEED, W, metric, max_degree=max_deg):
        if ids is None:
            break
        assert rows.shape == (len(ids), R) and rows.dtype == np.uint32
        live = rows != tp.SENTINEL
        assert (live[:, :-1] >= live[:, 1:]).all()                    # the padding follows the picks, never between them
        ms.append(len(ids))
        row_lens.append(live.sum(1))
        one_id_slice |= len(ids) > 1 and any(s1 - s0 == 1 for s0, s1 in tp.slices(len(ids), W))
    np.testing.assert_array_equal(G, tp.vamana_oracle_build(oracle, name)[0])
    ms, row_lens = np.array(ms), np.concatenate(row_lens)
    assert (ms == 1).any()                                            # a batch of one id
    if W > 1:                                                         # (W = 1 splits nothing: both are impossible)
        assert (ms % W != 0).any() and (ms < W).any()
    if W in (2, 7):
        assert one_id_slice                                           # a slice of one id in a batch of several
    assert (row_lens < R).any()                                       # padded rows
    if name == "u8_R96":    # padded rows wider than a wave, none full (at most 76 picks): test_full_rows_wider_than_a_wave has those
        assert (G[:, 0] > tp.WAVE).sum() >= 100 and (row_lens > tp.WAVE).sum() >= 10 and row_lens.max() < R
    else:
        assert (row_lens == R).any()                                  # full rows


def test_full_rows_wider_than_a_wave(oracle):
    """the batch that gives the R = 96 case its full rows: some rows of 96 picks, many wider than a wave, all different (the
    launch-order test runs on a batch like this one: a row at another slot of its slice is seen)"""
    X, metric, G, ids, rows, R, L, alpha = tp.full_wide_batch(oracle)
    lens = (rows != tp.SENTINEL).sum(1)
    assert R == 96 and (lens == R).sum() >= 3 and (lens > tp.WAVE).sum() >= 50 and (lens < R).any()
    assert len(np.unique(rows, axis=0)) == len(ids) == tp.FULL_WIDE_M
    assert min(s1 - s0 for s0, s1 in tp.slices(len(ids), 3)) >= 64         # long enough for the locality order to engage


def test_case_table_is_what_the_device_test_says_it_is():
    assert [c[:3] + c[3:7] for c in tp.VAMANA_CASES.values()] == [
        (np.uint8, "l2", 32, 16, 16, 48, 2), (np.float16, "l2", 64, 32, 32, 100, 1), (np.float16, "l2", 64, 32, 32, 128, 1),
        (np.int8, "mips", 100, 24, 24, 70, 1), (tp.bfloat16, "l2", 128, 32, 32, 64, 1), (np.float32, "l2", 24, 16, 16, 200, 1),
        (np.uint8, "l2", 32, 96, 129, 100, 1)]
    assert [c[7] for c in tp.VAMANA_CASES.values()] == [(1, 2, 3, 7)] * 2 + [(3,)] * 5
    assert tp.N == 3000 and tp.slices(7, 3) == [(0, 3), (3, 6), (6, 7)] and tp.slices(2, 3) == [(0, 1), (1, 2), (2, 2)]
    for name in tp.VAMANA_CASES:                                      # integer-valued rows in every type
        X = tp.vamana_case(name)[0]
        f = from_bf16(X) if X.dtype == tp.bfloat16 else X.astype(np.float32)
        assert len(X) == tp.N and (f == np.round(f)).all() and np.abs(f).max() <= 255


def test_start_other_than_zero_changes_the_rows(oracle):
    """the start vertex reaches phase A: the first batches of a build from vertex 5 differ from those of a build from vertex 0"""
    X, metric, R, max_deg, L, alpha, passes, _ = tp.vamana_case("i8_L70")
    a = tp.oracle_two_phase_build(oracle, X, R, L, alpha, passes, tp.SEED, 3, metric, max_degree=max_deg)
    b = tp.oracle_two_phase_build(oracle, X, R, L, alpha, passes, tp.SEED, 3, metric, max_degree=max_deg, start=5)
    (_, ra, _), (_, rb, _) = next(a), next(b)
    assert ra[0, 0] == 0 and rb[0, 0] == 5


@pytest.mark.parametrize("name,W,forest", tp.HCNNG_TRIPLES, ids=[f"{a}-W{b}-{f[0]}x{f[1]}" for a, b, f in tp.HCNNG_TRIPLES])
def test_slabs_interleaved_in_tree_order_equal_the_forest(oracle, name, W, forest):
    T, cs = forest
    X, metric = tp.hcnng_points(name)
    want = oracle.hcnng_build(X, T, cs, tp.MST_DEG, seed=tp.HCNNG_SEED, metric=metric)
    stride = tp.slab_stride(T, W, tp.MST_DEG)
    slabs = tp.oracle_tree_slabs(oracle, X, T, cs, tp.MST_DEG, tp.HCNNG_SEED, W, metric)
    assert slabs.shape == (W, len(X), stride)
    np.testing.assert_array_equal(tp.interleave(slabs, T, tp.MST_DEG, T * tp.MST_DEG), want)
    wider = tp.oracle_tree_slabs(oracle, X, T, cs, tp.MST_DEG, tp.HCNNG_SEED, W, metric, stride=stride + 5)
    assert (wider[:, :, stride:] == tp.SENTINEL).all() and np.array_equal(wider[:, :, :stride], slabs)
    owned = [len(range(r, T, W)) for r in range(W)]
    for r in range(W):                                                # owned columns hold edges, all other columns are empty
        assert (slabs[r, :, owned[r] * tp.MST_DEG:] == tp.SENTINEL).all()
        assert all((slabs[r, :, j * tp.MST_DEG] != tp.SENTINEL).sum() > len(X) // 2 for j in range(owned[r]))
    if T % W:
        assert min(owned) < (T + W - 1) // W                          # a rank with fewer trees than the slab has room for
    if W > T:
        assert 0 in owned                                             # a rank without any tree
    if 1 < W < T:       # slab order is another graph: an assembly that walks the slabs one after the other is noticed
        assert not np.array_equal(tp.interleave(slabs, T, tp.MST_DEG, T * tp.MST_DEG, order="slab"), want)


def test_every_hcnng_type_has_an_idle_rank_case():
    for name, (_, _, Ws) in tp.HCNNG_CASES.items():
        assert any(T % W for W in Ws for T, _ in tp.HCNNG_FORESTS), name
    assert 7 in tp.HCNNG_CASES["u8"][2]


def test_append_onto_a_first_forest_and_the_bound_at_max_deg(oracle):
    """the expectations of the device's append tests: the oracle's initial-graph entry equals the interleave of the slabs after
    the current neighbours, with room for both forests and with rows that fill up (nothing beyond max_deg, order kept)"""
    X, metric = tp.hcnng_points("u8")
    (T1, cs1), (T2, cs2) = tp.HCNNG_FORESTS[1], tp.HCNNG_FORESTS[0]
    first = oracle.hcnng_build(X, T1, cs1, tp.MST_DEG, seed=tp.HCNNG_SEED)
    slabs = tp.oracle_tree_slabs(oracle, X, T2, cs2, tp.MST_DEG, tp.HCNNG_SEED + 100, 2)
    for max_deg in ((T1 + T2) * tp.MST_DEG, T1 * tp.MST_DEG + 2):
        G = np.zeros((len(X), max_deg + 1), np.uint32)
        G[:, :first.shape[1]] = first
        want = tp.wide_cases.hcnng_oracle_append(X, G.copy(), T2, cs2, tp.MST_DEG, tp.HCNNG_SEED + 100, oracle=oracle)
        np.testing.assert_array_equal(tp.interleave(slabs, T2, tp.MST_DEG, max_deg, initial=G), want)
        assert (want[:, 0] > first[:, 0]).any()
        assert all(np.array_equal(want[v, 1:1 + first[v, 0]], first[v, 1:1 + first[v, 0]]) for v in range(0, len(X), 97))
        if max_deg < (T1 + T2) * tp.MST_DEG:
            cut = first[:, 0].astype(np.int64) + (slabs != tp.SENTINEL).sum((0, 2)) > max_deg
            assert cut.sum() >= 100 and (want[cut, 0] == max_deg).all()      # rows that would overflow stop exactly at max_deg


def test_poison_is_told_from_padding():
    """the device test prefills every output with POISON and compares all words: padding or slab columns left unwritten differ
    from the 0xFFFFFFFF the oracle side holds there"""
    assert tp.SENTINEL == 0xFFFFFFFF and np.int32(-1).astype(np.uint32) == tp.SENTINEL
