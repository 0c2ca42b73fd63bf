"""The delete consolidation on the CPU restatement (tests/delete_ref.py): the invariants of the rule, the regime every shared case
is there for (so that no device test passes vacuously), and the quality of the consolidated graph against a rebuild.  The device
is proven equal to the restatement bit for bit in tests/test_delete_gpu.py, so quality needs no GPU."""
import numpy as np
import pytest

import delete_ref as dr
from parlayann_amd import datasets

CASES = [("layout", n) for n in dr.LAYOUTS] + [("wide", w) for w in dr.WIDE_WIDTHS] + [("long", None)]


def _case(kind, arg, oracle):
    if kind == "layout":
        return dr.layout_case(arg, oracle)
    return dr.wide_case(arg) if kind == "wide" else dr.long_case()


def _rows(G, v):
    return G[v, 1:1 + G[v, 0]]


def test_no_device_is_a_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from parlayann_amd import _capi
    lib = _capi.load()
    ids = np.zeros(1, np.uint32)
    for fn in (lib.pann_vamana_delete_batch, lib.pann_vamana_delete_batch_dev):
        assert fn(None, ids.ctypes.data, 1, 8, 1.2, None) == 3          # PANN_ERR_NO_DEVICE
        assert b"no HIP device" in lib.pann_last_error()
    assert _capi.DeleteStats.per_point_dist_cmps.offset == 48


@pytest.mark.parametrize("kind,arg", CASES)
def test_invariants_and_regimes(oracle, kind, arg):
    X, G, D, R, alpha, metric = _case(kind, arg, oracle)
    new, info = dr.delete_ref(oracle, X, G, D, alpha, R, metric)
    inD, owners, off, cand = info["inD"], info["owners"], info["offsets"], info["cand"]
    old = dr.normalized(G)
    # no row references D, rows of D are empty, rows outside A u D are untouched
    for v in range(len(G)):
        assert not inD[_rows(new, v)].any()
    assert not new[inD].any()
    rest = np.ones(len(G), bool); rest[inD] = False; rest[owners] = False
    np.testing.assert_array_equal(new[rest], old[rest])
    assert all(inD[_rows(G, p)].any() for p in owners) and not any(inD[_rows(G, p)].any() for p in np.flatnonzero(rest))
    # every new row is a duplicate-free subset of its candidates, within R, without the owner
    for i, p in enumerate(owners):
        row = _rows(new, p)
        assert len(row) <= R and len(set(row)) == len(row) and p not in row
        assert set(row) <= set(cand[off[i]:off[i + 1]])
    # order and multiplicity of the input mean nothing
    rng = np.random.default_rng(1)
    shuffled = rng.permutation(np.concatenate([D, D[:len(D) // 2], D[:3]]))
    np.testing.assert_array_equal(dr.delete_ref(oracle, X, G, shuffled, alpha, R, metric)[0], new)
    # the regime the case is there for
    reg = dr.regime(G, info)
    assert reg["two_deleted"] >= 1 and reg["back_edge"] >= 1, reg             # (a), (b)
    if kind == "wide":
        assert reg["widest_affected"] > 64 and reg["widest_deleted"] > 64, reg       # (e)
        assert G.shape[1] - 1 == arg and (G[:, 0] == arg).all()
    if kind == "long":
        assert reg["longest"] > dr.LONG and reg["shortest"] < dr.LONG, reg       # (d): both list paths of the greedy prune
        assert (np.diff(off.astype(np.int64)) > dr.LONG).sum() >= 100


def test_two_calls_equal_the_rule_applied_twice(oracle):
    X, G, D, R, alpha, metric = dr.layout_case("u8_24", oracle)
    D1, D2 = D[::2], D[1::2]
    g1, _ = dr.delete_ref(oracle, X, G, D1, alpha, R, metric)
    g2, info2 = dr.delete_ref(oracle, X, g1, D2, alpha, R, metric)
    d_all = np.zeros(len(G), bool); d_all[D] = True
    assert not g2[d_all].any() and not any(d_all[_rows(g2, v)].any() for v in range(len(G)))
    # D is per call: the second call sees the first call's rows, not the original ones, and D1 is already isolated in it
    assert not info2["inD"][D1].any()
    both, _ = dr.delete_ref(oracle, X, G, D, alpha, R, metric)
    assert not np.array_equal(both, g2)                    # one call of D1 u D2 is another graph: snapshot semantics
    # deleting what is already isolated changes nothing
    again, info3 = dr.delete_ref(oracle, X, g2, D1, alpha, R, metric)
    np.testing.assert_array_equal(again, g2)
    assert len(info3["owners"]) == 0


def test_edge_cases_cover_their_regime(oracle):
    X, G, _, R, alpha, metric = dr.layout_case("u8_24", oracle)
    p = 7
    D = dr.empty_row_case(G, p)
    new, info = dr.delete_ref(oracle, X, G, D, alpha, R, metric)
    i = int(np.flatnonzero(info["owners"] == p)[0])
    assert info["offsets"][i + 1] == info["offsets"][i] and new[p, 0] == 0         # (c): affected, nothing to choose from
    assert dr.regime(G, info)["empty_list"] >= 1
    assert 0 < len(D) < len(G) - 1
    v = 11
    Din = dr.in_neighbours(G, v)
    assert len(Din) >= 1 and v not in Din
    new, info = dr.delete_ref(oracle, X, G, Din, alpha, R, metric)
    assert not any(v in _rows(new, u) for u in Din)
    # everything deleted: no owner, every row empty
    new, info = dr.delete_ref(oracle, X, G, np.arange(len(G)), alpha, R, metric)
    assert len(info["owners"]) == 0 and not new.any()


# ---- quality -------------------------------------------------------------------------------------------------
QN, QD, QR, QL, QALPHA, QBEAM, QK, QNQ = 2000, 32, 32, 64, 1.2, 32, 10, 200
# Measured with quality() below while this test was written (recall@10: consolidated / rebuild / dropped edges):
#   seed 1  0.9845 / 0.9885 / 0.9720      seed 2  0.9840 / 0.9810 / 0.9760      seed 3  0.9880 / 0.9845 / 0.9760
# The largest gap rebuild - consolidated is 0.0040 (seed 1); 0.01 on top for the granularity of the tie-aware recall at 2 000
# result slots.  The consolidated graph beat the dropped-edges graph for all three seeds, so that is asserted too.
RECALL_MARGIN = 0.0040 + 0.01


def quality(oracle, seed):
    """tie-aware recall@10 at beam 32 from vertex 0 of (consolidated, rebuilt over the survivors, edges into D merely dropped),
    and the ids the consolidated graph returned"""
    X = datasets.sift_like(QN, QD, seed=1000 + seed, dtype=np.uint8)
    Q = datasets.sift_like(QNQ, QD, seed=2000 + seed, dtype=np.uint8)
    G, _ = oracle.vamana_build(X, QR, QL, QALPHA, num_passes=1, seed=seed)
    D = dr.seeded_ids(QN, 0.20, 3000 + seed, keep=(0,))
    inD = np.zeros(QN, bool); inD[D] = True
    live = np.flatnonzero(~inD).astype(np.uint32)
    gt_local, gt_d = oracle.bruteforce_knn(X[live], Q, 50)
    gt = live[gt_local]
    search = lambda pts, graph: oracle.batch_search(pts, graph, queries=Q, k=QK, beam=QBEAM, starts=(0,))["ids"]
    cons, _ = dr.delete_ref(oracle, X, G, D, QALPHA, QR)
    ids_cons = search(X, cons)
    Gr, _ = oracle.vamana_build(X[live], QR, QL, QALPHA, num_passes=1, seed=seed)
    ids_reb = live[search(X[live], Gr)]
    dropped = np.zeros_like(G)
    for v in live:
        row = G[v, 1:1 + G[v, 0]]
        row = row[~inD[row]]
        dropped[v, 0] = len(row); dropped[v, 1:1 + len(row)] = row
    ids_drop = search(X, dropped)
    rec = [oracle.recall(i, gt, gt_d, QK) for i in (ids_cons, ids_reb, ids_drop)]
    return rec, ids_cons, inD


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_consolidated_graph_keeps_the_recall_of_a_rebuild(oracle, seed):
    (cons, reb, drop), ids, inD = quality(oracle, seed)
    print(f"seed {seed}: recall consolidated {cons:.4f} rebuild {reb:.4f} dropped-edges {drop:.4f}")
    assert (ids < QN).all() and not inD[ids].any()         # hard: a deleted id is never returned
    assert cons >= reb - RECALL_MARGIN
    assert cons >= drop
