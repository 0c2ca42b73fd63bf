"""The reference side of tests/test_hcnng_leaves_gpu.py, on the CPU alone: the Python restatement of the HCNNG build
(tests/hcnng_ref.py) equals the oracle's on every case of tests/hcnng_cases.py, every case really contains the leaves and the
halvings it is there for -- worked out from the restated trees, which are the only place that knows WHY a cluster was halved --
and the restatement tells the reference's rules from their textbook neighbours."""
import numpy as np
import pytest

import hcnng_cases as hc
import hcnng_ref
import wide_cases

_built = {}


def _ref_build(oracle, name):
    if name not in _built:
        X, metric, T, cs, mst_deg, seed = hc.case(name)
        _built[name] = hcnng_ref.build(X, T, cs, mst_deg, seed, metric, oracle)
    return _built[name]


@pytest.mark.parametrize("name", hc.NAMES)
def test_restatement_equals_oracle(oracle, name):
    np.testing.assert_array_equal(_ref_build(oracle, name), hc.oracle_graph(name, oracle))


@pytest.mark.parametrize("name", hc.NAMES)
def test_case_contains_what_it_is_there_for(name):
    X, metric, T, cs, mst_deg, seed = hc.case(name)
    got = hc.trees(name)
    assert len(got) == T
    for t, (leaves, why) in enumerate(got):
        sizes = [len(l) for l in leaves]
        print(f"{name} tree {t}: {len(sizes)} leaves, sizes {sizes if len(sizes) <= 8 else sorted(set(sizes))}, {why}")
        assert np.array_equal(np.sort(np.concatenate(leaves)), np.arange(len(X)))          # a partition of the ids
        assert max(sizes) <= cs and min(sizes) >= 1
        assert why["same"] + why["first_empty"] + why["second_empty"] <= why["splits"] == len(leaves) - 1
    if hc.CONDITIONS[name] is not None:
        assert hc.CONDITIONS[name](name)


def test_case_table_is_what_the_device_test_says_it_is():
    assert hc.LDS_CAP == 4096 and hcnng_ref.M == 10
    assert [hc.case(k)[0].shape for k in hc.NAMES] == [(10000, 16)] * 3 + [(5000, 16), (3000, 16), (1000, 16), (3000, 8), (3000, 8)] + \
        [(777, 16)] * 2 + [(300, 16), (1, 16), (2, 16), (3, 16)]
    assert [hc.case(k)[0].dtype for k in hc.STRADDLES] == [np.uint8, np.float16, np.int8]
    u8, f16, i8 = (hc.case(k)[0] for k in hc.STRADDLES)
    assert np.array_equal(u8, f16) and np.array_equal(u8.astype(np.int64) - 128, i8)
    assert len(np.unique(hc.case("dup5")[0], axis=0)) == 5
    ray = hc.case("ray_mips")[0]
    assert ray[:, 0].min() >= 1 and not ray[:, 1:].any()
    assert [hc.case(k)[4] for k in ("tiny2", "tiny11")] == [1, 12]                           # mst_deg 1; a bound never reached
    # MIPS on a ray: the distance to a pivot is -c * c_pivot with c > 0, so every member lands on the side of the larger pivot
    # and EVERY split is halved -- an empty first side is the normal outcome there, not a corner
    for _, why in hc.trees("ray_mips"):
        assert why["first_empty"] + why["second_empty"] + why["same"] == why["splits"]
    # ... which is why ray_mips cannot see a builder WITHOUT the empty-first-side guard: the cluster is split again whole until
    # the other side comes out empty, and is halved at the same place; the seeds differ, but no split of this case looks at one.
    # cone_mips is there for that (its condition): rows in a narrow cone, where two pivots of like length split for real
    X, metric, T, cs, _, seed = hc.case("ray_mips")
    for t, (leaves, _) in enumerate(hc.trees("ray_mips")):
        other = hcnng_ref.tree(X, cs, seed, t, metric, first_empty_guard=False)[0]
        assert len(other) == len(leaves) and all(np.array_equal(a, b) for a, b in zip(leaves, other))
    cone = hc.case("cone_mips")[0]
    assert cone.dtype == np.int8 and cone.min() >= 1


def test_all_same_distances_are_zero(oracle):
    X, metric, *_ = hc.case("all_same")
    leaf = hc.trees("all_same")[0][0][0]
    ids, d = oracle.leaf_knn(X, leaf, hcnng_ref.M, metric)
    assert not d.any()
    rest = [np.delete(leaf, i)[:hcnng_ref.M] for i in range(len(leaf))]                      # ties by id: the lowest other ids
    np.testing.assert_array_equal(ids, np.sort(np.stack(rest), axis=1))


def test_tiny_leaves_leave_empty_knn_slots(oracle):
    X, metric, *_ = hc.case("tiny11")
    leaf = next(l for l in hc.trees("tiny11")[0][0] if 2 <= len(l) <= 10)
    ids, d = oracle.leaf_knn(X, leaf, hcnng_ref.M, metric)
    assert (ids[:, len(leaf) - 1:] == hcnng_ref.SENTINEL).all() and (ids[:, :len(leaf) - 1] != hcnng_ref.SENTINEL).all()
    # mst_deg = 12 is never reached in a leaf of at most 11 members; mst_deg = 1 is reached by every matched member
    assert hc.oracle_graph("tiny11", oracle)[:, 0].max() <= 3 * 10
    g2 = hc.oracle_graph("tiny2", oracle)
    assert g2[:, 0].max() == 3 and g2[:, 0].min() < 3                                        # 1-member leaves add nothing


def test_build_onto_an_initial_graph_equals_oracle_append(oracle):
    """dup5 twice with max_degree = 14 < 2 * 9: the second pass is cut at the row end"""
    X, metric, T, cs, mst_deg, seed = hc.case("dup5")
    max_deg = 14
    first = hcnng_ref.build(X, T, cs, mst_deg, seed, metric, oracle, graph=np.zeros((len(X), max_deg + 1), np.uint32))
    np.testing.assert_array_equal(first[:, :T * mst_deg + 1], hc.oracle_graph("dup5", oracle))
    got = hcnng_ref.build(X, T, cs, mst_deg, seed, metric, oracle, graph=first)
    want = wide_cases.hcnng_oracle_append(X, first.copy(), T, cs, mst_deg, seed, metric=metric, oracle=oracle)
    np.testing.assert_array_equal(got, want)
    # (rows of degree 0 stay: in a leaf of identical points the members with the lowest ids take every edge)
    assert (got[:, 0] == max_deg).sum() >= 100 and got[:, 0].max() == max_deg and (first[:, 0] == T * mst_deg).sum() >= 100


SMALL = tuple(k for k in hc.NAMES if len(hc.case(k)[0]) <= 3000)


def test_rank_rule_and_stop_test_cannot_show_in_the_graph(oracle):
    """Union by rank[x] where a textbook has rank[root], and the stop test after every N-th edge, are restated because the
    device restates them -- but neither can change a graph (hcnng_ref.leaf_mst says why), so no case can be asked to tell them
    apart; asserted here so that nobody looks for the case.  What they CAN do on the device is fire wrongly (a stop before the
    sets are one, a find that loses a member): that changes the edges taken, and every case sees it."""
    for name in SMALL:
        X, metric, T, cs, mst_deg, seed = hc.case(name)
        for kw in (dict(rank_of="root"), dict(stop_every_n=False)):
            np.testing.assert_array_equal(hcnng_ref.build(X, T, cs, mst_deg, seed, metric, oracle, **kw), _ref_build(oracle, name))


def test_the_restatement_can_fail(oracle, monkeypatch):
    """the comparison with the oracle is not vacuous: a degree bound off by one (deg <= mst_deg where the reference has <)
    changes the graph of one_leaf, dup5, all_same, ray_mips and cone_mips -- the cases whose leaves reach the bound -- and of neither
    tiny2 (leaves of at most 2 members: one edge at most) nor tiny11 (mst_deg = 12 is never reached), which is what those two
    are in the table for.  A stop test that fires one edge early (before the last union) changes tiny11 and tiny2."""
    kruskal = hcnng_ref.leaf_mst
    monkeypatch.setattr(hcnng_ref, "leaf_mst", lambda lo, hi, N, mst_deg, *a: kruskal(lo, hi, N, mst_deg + 1, *a))
    changed = {}
    for name in SMALL:
        X, metric, T, cs, mst_deg, seed = hc.case(name)
        changed[name] = not np.array_equal(hcnng_ref.build(X, T, cs, mst_deg, seed, metric, oracle), _ref_build(oracle, name))
    assert [k for k in SMALL if changed[k]] == ["dup5", "all_same", "ray_mips", "cone_mips", "one_leaf"], changed
    monkeypatch.setattr(hcnng_ref, "leaf_mst", lambda lo, hi, N, mst_deg, *a: kruskal(lo, hi, N, mst_deg, *a)[:-1])
    for name in ("tiny2", "tiny11"):
        X, metric, T, cs, mst_deg, seed = hc.case(name)
        assert not np.array_equal(hcnng_ref.build(X, T, cs, mst_deg, seed, metric, oracle), _ref_build(oracle, name))
