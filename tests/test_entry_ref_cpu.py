"""CPU-only: the restatement of the entry-point rules (tests/entry_ref.py, DESIGN.md "Entry points") and the case tables of
tests/entry_cases.py are pinned before the device is compared against them:

* the centroid rule against an independent statement (math.fsum / Python integers) and the conversion rule at its edges;
* the tables reach the regimes they are there for: list lengths 0, 1, P - 1, P, P + 1, several pieces, an entry no query would
  name, two equal entries, a tie on the medoid decided by the id, fewer allowed points than per_filter;
* grouped_search_ref places the rows of the per-entry walks by the index array;
* quality on the data of tests/test_steered_ref_cpu.py: on clustered filters the masked walk finds more from the filter's medoid
  than from vertex 0.
"""
import math

import numpy as np
import pytest

import entry_cases as ec
import entry_ref
import grouped_knn_cases as gc
import masked_ref
import steered_ref
from parlayann_amd import bfloat16, datasets, from_bf16, to_bf16


@pytest.mark.parametrize("tname", ["u8", "i8", "f16", "bf16", "f32"])
def test_centroid_rule_against_fsum(tname):
    X, _ = gc.data(tname, 100)
    allow = np.random.default_rng(3).random(len(X)) < 0.3
    got = entry_ref.centroid(X, allow)
    W = entry_ref.widen(X)[allow]
    c = len(W)
    if tname in ("u8", "i8"):
        want = [int(sum(int(v) for v in W[:, j])) / c for j in range(W.shape[1])]
    else:
        want = [math.fsum(W[:, j]) / c for j in range(W.shape[1])]
    assert got.dtype == np.float32 and np.array_equal(got, np.array(want, np.float64).astype(np.float32))
    assert np.array_equal(entry_ref.centroid(X, np.zeros(len(X), bool)), np.zeros(100, np.float32))
    one = np.zeros(len(X), bool); one[77] = True
    assert np.array_equal(entry_ref.centroid(X, one), entry_ref.widen(X)[77].astype(np.float32))
    # real values: exact_sums is exact, so its double is fsum's
    R = np.random.default_rng(5).standard_normal((500, 7)).astype(np.float32)
    sums, e = entry_ref.exact_sums(R)
    assert [float(s * 2.0 ** e) if abs(e) < 900 else None for s in sums] == [math.fsum(R[:, j].astype(np.float64)) for j in range(7)]
    means = entry_ref.exact_mean(R)
    assert all(abs(float(m) - float(R[:, j].astype(np.float64).mean())) < 1e-12 for j, m in enumerate(means))


def test_conversion_rule():
    c = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 254.5, 255.5, 300.0, -129.0, -128.5, 127.5, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], np.float32)
    assert entry_ref.convert(c, np.uint8).tolist() == [0, 2, 2, 0, 0, 254, 255, 255, 0, 0, 128, 1, 1]          # ties to even, clamped
    assert entry_ref.convert(c, np.int8).tolist() == [0, 2, 2, 0, -2, 127, 127, 127, -128, -128, 127, 1, 1]
    h = entry_ref.convert(c, np.float16)
    assert h.dtype == np.float16 and float(h[11]) == 1.0 and float(h[12]) == 1.0 + 2.0 ** -9                   # f16: ties to even
    b = entry_ref.convert(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.0], np.float32), bfloat16)
    assert b.dtype == bfloat16 and from_bf16(b).tolist() == [1.0, 1.0 + 2.0 ** -6, 3.0] and np.array_equal(b, to_bf16([1.0, 1.015625, 3.0]))
    f = entry_ref.convert(c, np.float32)
    assert f.dtype == np.float32 and np.array_equal(f, c)


def test_tables_reach_their_regimes(oracle):
    tname, metric, d = "f16", "l2", 128
    P = ec.P
    counts = ec.allow_rows("pieces", 10).sum(axis=1)
    assert dict(zip(ec.PIECES, counts.tolist())) == ec.PIECE_COUNTS
    assert {0, 1, P - 1, P, P + 1} <= set(counts.tolist()) and 3 * P < ec.PIECE_COUNTS["several"] < 4 * P
    for E in ec.PER_FILTER:
        want = gc.wanted_counts(E)
        got = ec.allow_rows("groups", E).sum(axis=1)
        assert got.tolist() == [want[e] for e in gc.ENTRIES]
        assert gc.GROUP_SIZES["unused"] == 0                                    # the entry no query of the grouped tests names
        r = ec.reference(oracle, tname, metric, d, "groups", E)
        assert r["counts"].tolist() == [min(E, want[e]) for e in gc.ENTRIES]
        i, j = gc.ENTRIES.index("half"), gc.ENTRIES.index("half_again")          # two equal entries: equal rows
        for f in ("ids", "dists", "centroids"):
            assert np.array_equal(r[f][i], r[f][j])
        short = gc.ENTRIES.index("k_minus_1")                                    # c_g < per_filter: padding behind the list
        assert (r["ids"][short, E - 1:] == 0xFFFFFFFF).all() and np.isinf(r["dists"][short, E - 1:]).all()
        assert not r["centroids"][gc.ENTRIES.index("none")].any() and r["counts"][gc.ENTRIES.index("none")] == 0
        found = r["ids"] != 0xFFFFFFFF
        A = ec.allow_rows("groups", E)
        assert A[np.nonzero(found)[0], r["ids"][found]].all()                   # hard: only allowed points
        assert (np.diff(r["dists"][gc.ENTRIES.index("all")][:min(E, 128)]) >= 0).all()
        p = ec.reference(oracle, tname, metric, d, "pieces", E)
        t = ec.PIECES.index("ties")
        m = min(E, 4)
        assert p["ids"][t, :m].tolist() == list(ec.TIE_IDS[:m]) and (p["dists"][t, :m] == p["dists"][t, 0]).all()   # the id decides
        assert p["counts"].tolist() == [min(E, ec.PIECE_COUNTS[e]) for e in ec.PIECES]
        filled = ec.with_fill(p, 0)
        assert (filled["ids"][ec.PIECES.index("empty")] == 0).all() and np.array_equal(filled["ids"][found_rows(p)], p["ids"][found_rows(p)])
    X, _ = gc.data(tname, d)
    assert np.array_equal(p["centroids"][t], entry_ref.widen(X)[ec.TIE_IDS[0]].astype(np.float32))      # the centroid IS the copied row


def found_rows(r):
    return r["ids"] != 0xFFFFFFFF


def test_grouped_search_ref_places_rows(oracle):
    import steered_cases as sc
    X, Q, metric = sc.layout_data("u8")
    G = sc.graph("u8", 32)
    T = 20
    lab, _ = sc.labels_of(T, "match", False)
    table = np.array([[0xFFF, t] for t in (3, 0, 7)], np.uint32)
    group = np.array([0, 2, 2, 0, 1, 0, 2, 2], np.uint32)                       # interleaved
    starts = np.array([[0, 5], [9, 11], [100, 7]], np.uint32)
    kw = dict(k=10, beam=32, metric=metric, out_k=10, visited_cap=512)
    for steer in (None, 8):
        got = entry_ref.grouped_search_ref(X, G, lab, "match", table, group, starts, steer=steer, queries=Q[:8], **kw)
        for q in range(8):
            allow = (lab & 0xFFF) == table[group[q], 1]
            st = tuple(int(s) for s in starts[group[q]])
            one = (masked_ref.masked_batch_search(X, G, allow, queries=Q[q:q + 1], starts=st, **kw) if steer is None else
                   steered_ref.steered_batch_search(X, G, allow, fill=steer, queries=Q[q:q + 1], starts=st, **kw))
            for f in entry_ref.SEARCH_FIELDS + (entry_ref.STEER_FIELDS if steer is not None else ()) + ("visited_ids", "visited_dists"):
                assert np.array_equal(got[f][q], one[f][0]), (steer, q, f)
    shared = entry_ref.grouped_search_ref(X, G, lab, "match", table, group, starts[0], queries=Q[:8], **kw)   # one row of starts
    allow = (lab & 0xFFF) == 7
    one = masked_ref.masked_batch_search(X, G, allow, queries=Q[1:2], starts=(0, 5), **kw)
    assert np.array_equal(shared["ids"][1], one["ids"][0]) and shared["dist_cmps"][1] == one["dist_cmps"][0]


# ---- quality: the data of tests/test_steered_ref_cpu.py, clustered filters ("tenant clusters") ----------------------------------
QN, QD, QR, QL, QALPHA, QBEAM, QK, QNQ, QSEED = 2000, 32, 32, 64, 1.2, 32, 10, 200, 1
CLUSTERS = [(size, anchor) for size in (100, 20) for anchor in (1234, 77, 1999)]


def test_quality_medoid_start_against_vertex_0(oracle):
    """Masked walk, beam 32, k = 10, 200 queries; filter = the `size` points nearest to an anchor point; starts (0,) against the
    filter's medoid.  Tie-aware recall@10 against the exact allowed neighbours, measured while this test was written (the
    table is in DESIGN.md "Entry points"):

        allowed / anchor          100 / 1234  100 / 77  100 / 1999  20 / 1234  20 / 77  20 / 1999
        recall, start 0           0.9475      0.9720    0.9215      0.7305     0.9250   0.5700
        recall, medoid start      0.9575      0.9805    0.9275      0.7645     0.9850   0.7165
        allowed_cmps, start 0     11 911      15 348    9 476       2 331      4 110    1 531
        allowed_cmps, medoid      13 346      16 180    9 526       2 669      5 453    2 120

    The reference meets both conditions on all six, so both are asserted."""
    X = datasets.sift_like(QN, QD, seed=1000 + QSEED, dtype=np.uint8)
    Q = datasets.sift_like(QNQ, QD, seed=2000 + QSEED, dtype=np.uint8)
    G, _ = oracle.vamana_build(X, QR, QL, QALPHA, num_passes=1, seed=QSEED)
    for size, anchor in CLUSTERS:
        near, _ = oracle.bruteforce_knn(X, X[anchor:anchor + 1], size)
        allow = np.zeros(QN, bool)
        allow[near[0]] = True
        live = np.flatnonzero(allow).astype(np.uint32)
        gt_local, gt_d = oracle.bruteforce_knn(X[live], Q, min(50, len(live)))
        gt = live[gt_local]
        medoid = int(entry_ref.filter_medoids(oracle, X, allow[None, :], 1, "l2")["ids"][0, 0])
        assert allow[medoid]
        kw = dict(queries=Q, k=QK, beam=QBEAM)
        r0 = masked_ref.masked_batch_search(X, G, allow, starts=(0,), **kw)
        rm = masked_ref.masked_batch_search(X, G, allow, starts=(medoid,), **kw)
        rec0, recm = oracle.recall(r0["ids"][:, :QK], gt, gt_d, QK), oracle.recall(rm["ids"][:, :QK], gt, gt_d, QK)
        ac0, acm = int(r0["allowed_cmps"].sum()), int(rm["allowed_cmps"].sum())
        print(f"allowed {size} / anchor {anchor}: medoid {medoid}  recall@{QK} start 0 {rec0:.4f} medoid {recm:.4f}  allowed_cmps {ac0} / {acm}  "
              f"mean dist_cmps {r0['dist_cmps'].mean():.1f} / {rm['dist_cmps'].mean():.1f}")
        assert recm >= rec0, (size, anchor, rec0, recm)
        assert acm >= ac0, (size, anchor, ac0, acm)
