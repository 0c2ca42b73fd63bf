"""The label-aware Vamana build on the device (DESIGN.md "Label-aware build"): equal labels give the plain build bit for bit, one
batch (host entry, and device entry on a caller's stream) equals the CPU restatement id for id, every edge joins points that share a
label, every label is reached from its start inside the label, refusals leave the graph as it was.  Integer-valued coordinates."""
import numpy as np
import pytest

import labeled_build_ref as lr
from parlayann_amd import DeviceIndex, PannError

pytestmark = pytest.mark.gpu
TYPES = [(np.uint8, "l2"), (np.int8, "mips"), (np.float16, "l2"), (np.float32, "l2"), (np.float32, "mips")]


def _points(n, d, dtype, seed):
    lo, hi = (0, 32) if dtype == np.uint8 else (-16, 16)
    return np.random.default_rng(seed).integers(lo, hi, (n, d)).astype(dtype)


def _preset(n, deg, max_deg, seed, labels):
    """reference-layout rows of `deg` random neighbours that share a label with the row's point"""
    rng = np.random.default_rng(seed)
    G = np.zeros((n, max_deg + 1), np.uint32)
    G[:, 0] = deg
    for v in range(n):
        G[v, 1:1 + deg] = rng.choice(np.setdiff1d(np.flatnonzero(labels & labels[v]), [v]), deg, replace=False)
    return G


def _labels4(n, seed):
    rng = np.random.default_rng(seed)      # 4 labels, 1-3 per point, overlapping
    return np.array([sum(1 << int(b) for b in rng.choice(4, int(rng.integers(1, 4)), replace=False)) for _ in range(n)], np.uint32)


@pytest.mark.parametrize("dtype,metric", TYPES)
def test_equal_labels_give_the_plain_build(dtype, metric):
    n, R, L = 300, 8, 16
    X = _points(n, 24, dtype, 5)
    same, table = np.full(n, 4, np.uint32), np.zeros((32, 1), np.uint32)
    plain, lab = DeviceIndex(X, max_degree=R, metric=metric), DeviceIndex(X, max_degree=R, metric=metric)
    lab.set_labels(same)
    G0 = _preset(n, 3, R, 6, same)
    batch = np.random.default_rng(7).permutation(n)[:90].astype(np.uint32)
    plain.set_graph(G0), lab.set_graph(G0)
    plain.vamana_insert_batch(batch, R, L, 1.2), lab.vamana_insert_batch(batch, R, L, 1.2, label_starts=table)
    np.testing.assert_array_equal(lab.get_graph(), plain.get_graph())
    plain.clear_graph(), lab.clear_graph()
    plain.vamana_build(R, L, 1.2, num_passes=2, seed=3)
    lab.vamana_build(R, L, 1.2, num_passes=2, seed=3, label_starts=table)
    np.testing.assert_array_equal(lab.get_graph(), plain.get_graph())
    plain.close(), lab.close()


@pytest.fixture(scope="module")
def case():
    """n = 200, 4 overlapping labels, a preset graph of label-sharing edges (max degree R = 6), one start per label"""
    n, labels = 200, _labels4(200, 11)
    table = np.zeros((32, 1), np.uint32)
    table[:4, 0] = [np.flatnonzero(labels & (1 << b))[b] for b in range(4)]
    return n, labels, _preset(n, 3, 6, 12, labels), table


_want = {}      # (dtype, metric, m) -> the restatement's graph, worked out once


@pytest.mark.parametrize("m,dev", [(1, False), (63, False), (65, False), (65, True)])
@pytest.mark.parametrize("dtype,metric", TYPES)
def test_one_batch_equals_the_restatement(oracle, case, dtype, metric, m, dev):
    n, labels, G0, table = case
    R, L, alpha = 6, 12, 1.2
    X = _points(n, 17, dtype, 13)                                # d = 17: a row tail
    batch = np.random.default_rng(14).permutation(n)[:m].astype(np.uint32)
    if (dtype, metric, m) not in _want:
        _want[dtype, metric, m], info = lr.insert_batch(oracle, X, G0, labels, batch, table, R, L, alpha, metric)
        assert m == 1 or (info["longest"] > R and info["heavy"]), info      # a candidate list above R and an over-full reverse row
    ix = DeviceIndex(X, G0, metric=metric)
    ix.set_labels(labels)
    if dev:
        import torch
        d_batch, d_table = (torch.from_numpy(x.view(np.int32).copy()).cuda() for x in (batch, table))
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        ix.set_stream(s.cuda_stream)
        ix.vamana_insert_batch_labeled_dev(d_batch.data_ptr(), m, d_table.data_ptr(), 1, R, L, alpha)
        ix.set_stream(0, private=True)
    else:
        ix.vamana_insert_batch(batch, R, L, alpha, label_starts=table)
    np.testing.assert_array_equal(ix.get_graph(), _want[dtype, metric, m])
    ix.close()


@pytest.fixture(scope="module")
def built():
    """A labeled build from the empty graph.  R = 24: a point shares its row among up to three labels, so each label gets the 8 slots of
    the one-label shape above only at three times its R.  (At R = 8, 10 of label 0's points had no in-edge from inside the label.)"""
    n, R, L = 300, 24, 48
    labels = _labels4(n, 22)
    ix = DeviceIndex(_points(n, 24, np.uint8, 21), max_degree=R)
    ix.set_labels(labels)
    table = ix.label_start_table()
    ix.vamana_build(R, L, 1.2, num_passes=2, seed=3, label_starts=table)
    yield ix, labels, table, ix.get_graph()
    ix.close()


@pytest.mark.parametrize("bit", range(4))
def test_edges_share_a_label_and_a_label_is_reached_from_its_start_inside_it(built, bit):
    ix, labels, table, G = built
    assert all(G[u, 0] > 0 and (labels[G[u, 1:1 + G[u, 0]]] & labels[u]).all() for u in range(len(G)))
    allow = (labels & (1 << bit)) != 0
    inside = np.zeros_like(G)                              # only edges between allowed points are read
    for u in np.flatnonzero(allow):
        nb = [v for v in G[u, 1:1 + G[u, 0]] if allow[v]]
        inside[u, 0], inside[u, 1:1 + len(nb)] = len(nb), nb
    assert allow[table[bit, 0]]
    ix.set_graph(inside)
    r = ix.reachability(starts=table[bit], consider=allow)
    ix.set_graph(G)
    assert r["unreached_count"] == 0, (bit, r["unreached_ids"])


def test_refusals_leave_the_graph_untouched(case):
    n, labels, G0, table = case
    R, L, batch = 6, 12, np.arange(20, dtype=np.uint32)
    ix = DeviceIndex(_points(n, 17, np.uint8, 13), G0)
    before = ix.get_graph()
    def refused(h, starts):
        with pytest.raises(PannError):
            h.vamana_insert_batch(batch, R, L, 1.2, label_starts=starts)
        np.testing.assert_array_equal(h.get_graph(), before if h is ix else 0)
    refused(ix, table)                                       # no labels on the handle
    ix.set_labels(np.where(np.arange(n) == 7, 0, labels).astype(np.uint32))
    refused(ix, table)                                       # a batch point with label word 0
    ix.set_labels(labels)
    refused(ix, np.zeros((32, 0), np.uint32))                # nstarts == 0
    bad = table.copy()
    bad[31, 0] = n
    refused(ix, bad)                                         # a start id >= n, in a row no batch point uses
    q = DeviceIndex.from_packed(np.random.default_rng(1).integers(0, 256, (n, 9)).astype(np.uint8), 18, "u4", max_degree=R)
    q.set_labels(labels)
    refused(q, table)                                        # a four-bit handle
    ix.close(), q.close()
