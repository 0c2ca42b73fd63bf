"""HCNNG builds on the device at the leaves the other suites never produce (tests/hcnng_cases.py): leaves above 4096 members --
leaf_mst_kernel's HBM mode, alone and side by side with LDS-mode leaves in one launch; the leaf kNN kernels on thousands of
members -- halved clusters (identical pivots, an empty side under MIPS), leaves of identical points, leaves of 1 .. 11 members,
builds without a split level, and the refusals at the parameter edges.  Whole graphs against the oracle, then phase by phase
(leaf kNN over the restated leaves, one tree at a time) so that a mismatch names a tree and, with the leaf list, a leaf.
tests/test_hcnng_cases_cpu.py shows on the CPU that every case contains what it is there for.  Integer-valued data: every
comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import hcnng_cases as hc
import hcnng_ref
import two_phase_cases as tp
import wide_cases
from parlayann_amd import DeviceIndex, _capi

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
BAD_ARG = _capi.PANN_ERR_BAD_ARG


def _device_graph(name, max_degree=None, options=()):
    X, metric, T, cs, mst_deg, seed = hc.case(name)
    ix = DeviceIndex(X, max_degree=T * mst_deg if max_degree is None else max_degree, metric=metric)
    try:
        for k, v in options:
            ix.set_option(k, v)
        ix.hcnng_build(T, cs, mst_deg, seed=seed)
        return ix.get_graph()
    finally:
        ix.close()


# ---- 1. whole graphs --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", hc.NAMES)
def test_graph_equals_oracle(oracle, name):
    want = hc.oracle_graph(name, oracle)
    got = _device_graph(name)
    np.testing.assert_array_equal(got[:, 0], want[:, 0], err_msg="degrees")
    np.testing.assert_array_equal(hc.norm(got), hc.norm(want))
    if name == "n1":
        assert got.shape == (1, 7) and not got.any()


# ---- 2. phase by phase at large leaves ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", hc.STRADDLES)
def test_leaf_knn_of_the_restated_leaves(oracle, name):
    """the kNN kernels (lane-owns-row for one-byte types, dense tiles for float16) on leaves of thousands of members"""
    X, metric, T, cs, mst_deg, seed = hc.case(name)
    leaves = hc.trees(name)[0][0]
    assert max(len(l) for l in leaves) > hc.LDS_CAP
    ids = np.concatenate(leaves)
    off = np.concatenate([[0], np.cumsum([len(l) for l in leaves])]).astype(np.uint64)
    ix = DeviceIndex(X, max_degree=mst_deg, metric=metric)
    try:
        gi, gd = ix.leaf_knn_batch(ids, off, hcnng_ref.M)
    finally:
        ix.close()
    for l, leaf in enumerate(leaves):
        oi, od = oracle.leaf_knn(X, leaf, hcnng_ref.M, metric)
        rows = slice(int(off[l]), int(off[l + 1]))
        np.testing.assert_array_equal(gi[rows], oi, err_msg=f"ids of leaf {l} ({len(leaf)} members)")
        np.testing.assert_array_equal(gd[rows].view(np.uint32), od.view(np.uint32), err_msg=f"distances of leaf {l} ({len(leaf)} members)")


@pytest.mark.parametrize("name", hc.STRADDLES)
def test_one_tree_at_a_time(oracle, name):
    X, metric, T, cs, mst_deg, seed = hc.case(name)
    for t in range(T):
        ix = DeviceIndex(X, max_degree=mst_deg, metric=metric)
        try:
            ix.hcnng_build(1, cs, mst_deg, seed=seed + t)
            got = ix.get_graph()
        finally:
            ix.close()
        want = tp.oracle_tree(oracle, X, t, cs, mst_deg, seed, metric)
        np.testing.assert_array_equal(hc.norm(got), hc.norm(want), err_msg=f"tree {t}, leaves {hc.leaf_sizes(name)[t]}")


# ---- 3. HBM mode onto occupied rows ------------------------------------------------------------------------------------------

def test_second_forest_onto_occupied_rows(oracle):
    """(3, 6000, 3) with seed 5, then again with seed 6 onto the same handle at max_degree = 14: the HBM-mode leaves of the second
    forest read the rows' live degrees and cut the rows at 14"""
    X, metric, T, cs, mst_deg, seed = hc.case("straddle")
    max_deg = 14
    ix = DeviceIndex(X, max_degree=max_deg, metric=metric)
    try:
        ix.hcnng_build(T, cs, mst_deg, seed=seed)
        first = ix.get_graph()
        np.testing.assert_array_equal(hc.norm(first)[:, :T * mst_deg + 1], hc.norm(hc.oracle_graph("straddle", oracle)))
        assert not first[:, T * mst_deg + 1:].any()
        ix.hcnng_build(T, cs, mst_deg, seed=seed + 1)
        got = ix.get_graph()
    finally:
        ix.close()
    want = wide_cases.hcnng_oracle_append(X, hc.norm(first), T, cs, mst_deg, seed + 1, metric=metric, oracle=oracle)
    np.testing.assert_array_equal(hc.norm(got), hc.norm(want))
    assert got[:, 0].max() == max_deg and (got[:, 0] == max_deg).sum() >= 100 and (got[:, 0] > first[:, 0]).any()


# ---- 4. slab mode ----------------------------------------------------------------------------------------------------------

def _to_host(t):
    return t.cpu().numpy().view(np.uint32)


def test_tree_slabs_and_assembly_at_large_leaves(oracle):
    """W = 2: rank 0 owns trees 0 and 2, rank 1 tree 1.  In slab mode deg is pre-filled with (tg + j) * mst_deg and the HBM
    path adds to it"""
    X, metric, T, cs, mst_deg, seed = hc.case("straddle")
    W = 2
    stride = tp.slab_stride(T, W, mst_deg)
    ix = DeviceIndex(X, max_degree=T * mst_deg, metric=metric)
    try:
        slabs = torch.full((W, ix.n, stride), POISON, dtype=torch.int32, device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        for r in range(W):
            _capi.check(ix._lib.pann_hcnng_build_trees_dev(ix.handle, r, W, len(range(r, T, W)), cs, mst_deg, seed,
                                                           C.c_void_p(slabs[r].data_ptr()), stride, None))
        want = tp.oracle_tree_slabs(oracle, X, T, cs, mst_deg, seed, W, metric)
        np.testing.assert_array_equal(_to_host(slabs), want)
        assert not ix.get_graph().any()
        _capi.check(ix._lib.pann_hcnng_assemble_dev(ix.handle, C.c_void_p(slabs.data_ptr()), W, stride, T, mst_deg))
        np.testing.assert_array_equal(ix.get_graph(), hc.oracle_graph("straddle", oracle))
    finally:
        ix.close()


# ---- 5. forest grouping ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", [1, 3])
def test_forest_group_at_large_leaves(oracle, group):
    """group = 3: leaves above and below the cap from different trees share the level launches"""
    got = _device_graph("straddle", options=(("forest_group", group),))
    np.testing.assert_array_equal(hc.norm(got), hc.norm(hc.oracle_graph("straddle", oracle)))


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["straddle", "all_same"])
def test_two_runs_give_the_same_graph(name):
    a, b = _device_graph(name), _device_graph(name)
    np.testing.assert_array_equal(hc.norm(a), hc.norm(b))
    assert a[:, 0].any()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------

def test_refusals_at_the_parameter_edges(oracle):
    X, metric, T, cs, mst_deg, seed = hc.case("one_leaf")
    lib = _capi.load()
    ix = DeviceIndex(X, max_degree=T * mst_deg, metric=metric)
    try:
        ix.hcnng_build(T, cs, mst_deg, seed=seed)
        G = ix.get_graph()
        np.testing.assert_array_equal(hc.norm(G), hc.norm(hc.oracle_graph("one_leaf", oracle)))
        for what, args in (("cluster_size 1", (T, 1, mst_deg)), ("cluster_size 65536", (T, 65536, mst_deg)),
                           ("mst_deg 256", (1, cs, 256)), ("num_clusters * mst_deg > max_degree", (T + 1, cs, mst_deg))):
            assert lib.pann_index_set_option(ix.handle, b"no-such-option", 0) == 1          # last error := another text
            with pytest.raises(_capi.PannError) as e:
                ix.hcnng_build(*args, seed=seed)
            assert e.value.code == BAD_ARG and "no-such-option" not in str(e.value), what
            np.testing.assert_array_equal(ix.get_graph(), G, err_msg=what)
    finally:
        ix.close()
    # mst_deg 256 is refused for itself, not for the row length: a handle with room for it
    ix = DeviceIndex(X, max_degree=256, metric=metric)
    try:
        with pytest.raises(_capi.PannError) as e:
            ix.hcnng_build(1, cs, 256, seed=seed)
        assert e.value.code == BAD_ARG and "mst_deg" in str(e.value)
        assert not ix.get_graph().any()
    finally:
        ix.close()


def test_largest_accepted_parameters(oracle):
    """cluster_size 65535 and mst_deg 255 on one_leaf, max_degree sized to fit: a single leaf whose degree bound never binds"""
    X, metric, T, _, _, seed = hc.case("one_leaf")
    ix = DeviceIndex(X, max_degree=T * 255, metric=metric)
    try:
        ix.hcnng_build(T, 65535, 255, seed=seed)
        got = ix.get_graph()
    finally:
        ix.close()
    want = oracle.hcnng_build(X, T, 65535, 255, seed=seed, metric=metric)
    np.testing.assert_array_equal(hc.norm(got), hc.norm(want))
    assert 0 < got[:, 0].max() < T * 255
