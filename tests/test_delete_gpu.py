"""pann_vamana_delete_batch on the device against the CPU restatement (tests/delete_ref.py), bit for bit: the whole graph, the
per-owner distance comparisons and the call's counters.  tests/test_delete_cpu.py asserts that every shared case exercises the
regime it is there for.  Float types use integer-valued data (any summation order is exact)."""
import numpy as np
import pytest

import delete_ref as dr
from parlayann_amd import DeviceIndex, PannError, datasets

pytestmark = pytest.mark.gpu

PP0 = 3        # what per_point_dist_cmps holds before a call: the call adds to it


def _delete_and_check(oracle, ix, X, D, R, alpha, metric, dev=False):
    """one call on the handle == the restatement on the handle's graph; returns (expected graph, info)"""
    exp, info = dr.delete_ref(oracle, X, ix.get_graph(), D, alpha, R, metric)
    pp = np.full(len(X), PP0, np.uint32)
    if dev:
        import torch
        t = torch.from_numpy(np.ascontiguousarray(D, np.uint32).view(np.int32)).cuda()
        torch.cuda.synchronize()
        st = ix.vamana_delete_batch_dev(t.data_ptr(), len(D), R, alpha, point_stats=pp)
    else:
        st = ix.vamana_delete_batch(D, R, alpha, point_stats=pp)
    np.testing.assert_array_equal(ix.get_graph(), exp)
    want = np.full(len(X), PP0, np.uint32)
    want[info["owners"]] += info["dist_cmps"]
    np.testing.assert_array_equal(pp, want)
    for key, v in dr.expected_stats(info).items():
        assert st[key] == v, (key, st[key], v)
    assert st["t_expand_s"] > 0 and st["t_prune_s"] >= 0
    return exp, info


@pytest.fixture(scope="module")
def base(oracle):
    """the 600 x 24 uint8 case with the oracle's graph (the device's build is the same graph: test_build_gpu.py)"""
    return dr.layout_case("u8_24", oracle)


@pytest.mark.parametrize("name", list(dr.LAYOUTS))
def test_layouts_and_types(oracle, name):
    n, d, dtype, metric, R, L = dr.LAYOUTS[name]
    X = dr.layout_points(name)
    D = dr.layout_case(name, oracle)[2]
    ix = DeviceIndex(X, max_degree=R, metric=metric)
    ix.vamana_build(R, L, dr.LAYOUT_ALPHA, num_passes=1, seed=dr.LAYOUT_BUILD_SEED)
    G = ix.get_graph()
    _, info = _delete_and_check(oracle, ix, X, D, R, dr.LAYOUT_ALPHA, metric)
    reg = dr.regime(G, info)
    assert reg["two_deleted"] >= 1 and reg["back_edge"] >= 1, reg
    ix.close()


@pytest.mark.parametrize("max_deg", dr.WIDE_WIDTHS)
def test_rows_wider_than_a_wavefront(oracle, max_deg):
    X, G, D, R, alpha, metric = dr.wide_case(max_deg)
    ix = DeviceIndex(X, G, metric=metric)
    _, info = _delete_and_check(oracle, ix, X, D, R, alpha, metric)
    reg = dr.regime(G, info)
    assert reg["widest_affected"] > 64 and reg["widest_deleted"] > 64, reg
    ix.close()


def test_long_candidate_lists(oracle):
    X, G, D, R, alpha, metric = dr.long_case()
    ix = DeviceIndex(X, G, metric=metric)
    _, info = _delete_and_check(oracle, ix, X, D, R, alpha, metric)
    reg = dr.regime(G, info)
    assert reg["longest"] > dr.LONG and reg["shortest"] < dr.LONG, reg      # the LDS and the HBM list path in one call
    ix.close()


def test_owner_ranges_give_the_same_graph(oracle, base):
    """the prune of a call whose keys would not fit the key index runs in ranges of owners against the same snapshot"""
    X, G, D, R, alpha, metric = base
    ix = DeviceIndex(X, G, metric=metric)
    ix.set_option("delete_range_keys", 700)
    assert ix.get_option("delete_range_keys") == 700
    _, info = _delete_and_check(oracle, ix, X, D, R, alpha, metric)
    assert info["offsets"][-1] > 10 * 700
    ix.close()


def test_edges(oracle, base):
    X, G, D, R, alpha, metric = base
    n = len(X)
    ix = DeviceIndex(X, G, metric=metric)
    # m = 0
    st = ix.vamana_delete_batch(np.zeros(0, np.uint32), R, alpha)
    np.testing.assert_array_equal(ix.get_graph(), dr.normalized(G))
    assert st["deleted"] == 0 and st["affected"] == 0 and st["candidates"] == 0
    # one id a hundred times
    _, info = _delete_and_check(oracle, ix, X, np.full(100, 42, np.uint32), R, alpha, metric)
    assert info["inD"].sum() == 1 and len(info["owners"]) >= 1
    # ... and once more: an isolated vertex, nothing to do
    before = ix.get_graph()
    _, info = _delete_and_check(oracle, ix, X, np.array([42], np.uint32), R, alpha, metric)
    assert len(info["owners"]) == 0
    np.testing.assert_array_equal(ix.get_graph(), before)
    # every in-neighbour of a vertex, not the vertex
    ix.set_graph(G)
    Din = dr.in_neighbours(G, 11)
    got, info = _delete_and_check(oracle, ix, X, Din, R, alpha, metric)
    assert len(Din) >= 1 and not info["inD"][11] and not got[Din].any()
    # a vertex whose neighbours and their neighbours are all deleted keeps an empty row
    ix.set_graph(G)
    got, info = _delete_and_check(oracle, ix, X, dr.empty_row_case(G, 7), R, alpha, metric)
    assert 7 in info["owners"] and got[7, 0] == 0 and dr.regime(G, info)["empty_list"] >= 1
    # R below the handle's max_deg
    ix.set_graph(G)
    got, info = _delete_and_check(oracle, ix, X, D, R // 2, alpha, metric)
    assert got[info["owners"], 0].max() == R // 2 and got[:, 0].max() > R // 2      # only the re-pruned rows are cut to R
    # two successive calls
    ix.set_graph(G)
    _delete_and_check(oracle, ix, X, D[::2], R, alpha, metric)
    _delete_and_check(oracle, ix, X, D[1::2], R, alpha, metric)
    # shuffled and repeated ids: the same graph as the sorted set
    ix.set_graph(G)
    want, _ = dr.delete_ref(oracle, X, G, D, alpha, R, metric)
    ix.vamana_delete_batch(np.random.default_rng(2).permutation(np.concatenate([D, D[:50]])), R, alpha)
    np.testing.assert_array_equal(ix.get_graph(), want)
    # everything
    ix.set_graph(G)
    _, info = _delete_and_check(oracle, ix, X, np.arange(n, dtype=np.uint32), R, alpha, metric)
    assert len(info["owners"]) == 0 and not ix.get_graph().any()
    ix.close()


def test_device_ids_on_the_callers_stream(oracle, base):
    import torch
    X, G, D, R, alpha, metric = base
    ix = DeviceIndex(X, G, metric=metric)
    s = torch.cuda.Stream()
    ix.set_stream(s.cuda_stream)
    exp, _ = _delete_and_check(oracle, ix, X, D, R, alpha, metric, dev=True)
    ix.set_stream(0, private=True)
    np.testing.assert_array_equal(exp, dr.delete_ref(oracle, X, G, D, alpha, R, metric)[0])
    ix.close()


def test_errors_leave_the_graph_unchanged(base):
    import torch
    X, G, D, R, alpha, metric = base
    n = len(X)
    ix = DeviceIndex(X, G, metric=metric)
    bad = np.concatenate([D[:20], [n]]).astype(np.uint32)
    d_bad = torch.from_numpy(bad.view(np.int32)).cuda()
    d_ok = torch.from_numpy(D.view(np.int32)).cuda()
    torch.cuda.synchronize()
    calls = [lambda: ix.vamana_delete_batch(bad, R, alpha), lambda: ix.vamana_delete_batch(D, 0, alpha),
             lambda: ix.vamana_delete_batch(D, R + 1, alpha),
             lambda: ix.vamana_delete_batch_dev(d_bad.data_ptr(), len(bad), R, alpha),
             lambda: ix.vamana_delete_batch_dev(d_ok.data_ptr(), len(D), 0, alpha),
             lambda: ix.vamana_delete_batch_dev(d_ok.data_ptr(), len(D), R + 1, alpha)]
    for call in calls:
        with pytest.raises(PannError) as e:
            call()
        assert e.value.code == 1                           # PANN_ERR_BAD_ARG
        np.testing.assert_array_equal(ix.get_graph(), dr.normalized(G))
    ix.close()
    packed = np.random.default_rng(3).integers(0, 256, (64, 8), dtype=np.uint8)
    i4 = DeviceIndex.from_packed(packed, 16, "u4", max_degree=8)
    with pytest.raises(PannError) as e:
        i4.vamana_delete_batch(np.array([1], np.uint32), 8, 1.2)
    assert e.value.code == 4                               # PANN_ERR_UNSUPPORTED
    i4.close()


def test_searches_afterwards(oracle, base):
    """the filter codes of the beam-91..128 searches stay in step with the rows a delete writes"""
    X, G, _, R, alpha, metric = base
    n = len(X)
    D = dr.seeded_ids(n, 0.30, 61, keep=(0,))
    ix = DeviceIndex(X, G, metric=metric)
    ix.vamana_insert_batch(np.arange(50, 90, dtype=np.uint32), R, 128, alpha)       # a Vamana call at L = 128 builds the codes
    assert ix.get_option("filter_codes") == 1
    exp, info = _delete_and_check(oracle, ix, X, D, R, alpha, metric)
    assert ix.get_option("filter_codes") == 1             # maintained, not dropped
    live = np.flatnonzero(~info["inD"]).astype(np.uint32)[:150]
    g = ix.batch_search(query_ids=live, k=10, beam=128)
    o = oracle.batch_search(X, exp, query_ids=live, k=10, beam=128)
    for f in ("ids", "dists", "visited_count", "dist_cmps"):
        np.testing.assert_array_equal(g[f], o[f], err_msg=f)
    Q = datasets.sift_like(100, X.shape[1], seed=99, dtype=np.uint8)
    ids = ix.batch_search(Q, k=10, beam=64)["ids"]
    assert (ids < n).all() and not info["inD"][ids].any()
    ix.close()


def test_freed_slots_are_reused(oracle, base):
    """the dynamic loop: delete, upload new vectors into the freed slots, insert them"""
    X, G, _, R, alpha, metric = base
    n, L = len(X), dr.LAYOUTS["u8_24"][5]
    D = dr.seeded_ids(n, 0.10, 62, keep=(0,))
    ix = DeviceIndex(X, G, metric=metric)
    exp, _ = _delete_and_check(oracle, ix, X, D, R, alpha, metric)
    Xn = X.copy()
    Xn[D] = datasets.sift_like(len(D), X.shape[1], seed=63, dtype=np.uint8)
    for v in D:
        ix.upload_points(int(v), Xn[v:v + 1])
    np.testing.assert_array_equal(ix.points(), Xn)
    ix.vamana_insert_batch(D, R, L, alpha, start=0)
    want = np.ascontiguousarray(exp)
    oracle.vamana_insert_batch(Xn, want, D, R, L, alpha, start=0)
    np.testing.assert_array_equal(ix.get_graph(), dr.normalized(want))
    assert (ix.get_graph()[D, 0] > 0).all()
    ix.close()
