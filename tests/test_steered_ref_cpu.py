"""CPU-only: the restatement of the steered masked search (tests/steered_ref.py, DESIGN.md "Steered masked search") is pinned
before the device is compared against it:

* with an all-ones mask there is no bridge, and every field equals tests/masked_ref.py whatever `fill` is;
* the result equals an independent statement of the rule: the sorted set of the allowed ids a hook around the distance call saw;
* every id the hook saw that is not a start point is allowed (the steered walk spends no distance on a point it may not return);
* `pruned` never exceeds fill - 1 + deg_eff entries on any visit (the bound the kernel's candidate buffer is planned with);
* quality on the data of tests/test_delete_cpu.py: recall and allowed comparisons against the masked search, the yardstick.
"""
import numpy as np
import pytest

import filtered_cases as fc
from filtered_cases import random_rows as _data
import masked_ref
import steered_ref
from parlayann_amd import datasets

FIELDS = ("ids", "dists", "frontier_ids", "frontier_dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum",
          "visited_ids", "visited_dists", "result_count", "allowed_cmps", "from_beyond_cutoff", "from_unmerged", "recompared_in_result")
N, NQ, DEG = 1200, 8, 16


PIN = [(dt, m, beam) for dt, m in ((np.uint8, "l2"), (np.int8, "mips"), (np.float32, "l2")) for beam in (8, 64, 200)]
PIN_IDS = [f"{np.dtype(d).name}-{m}-b{b}" for d, m, b in PIN]


def _case(dtype, metric, beam):
    X, Q = _data(dtype, N, 24, 21 + beam), _data(dtype, NQ, 24, 22 + beam)
    G = fc.random_graph(N, DEG, 23 + beam)
    kw = dict(k=min(10, beam), beam=beam, metric=metric, out_k=min(beam, 64), visited_cap=N, queries=Q, starts=(0, 5, 9))
    return X, G, kw


@pytest.mark.parametrize("dtype,metric,beam", PIN, ids=PIN_IDS)
def test_all_ones_mask_equals_the_masked_search(oracle, dtype, metric, beam):
    X, G, kw = _case(dtype, metric, beam)
    ones = np.ones(N, bool)
    want = masked_ref.masked_batch_search(X, G, ones, **kw)
    for fill in (1, DEG // 2, 0):
        got = steered_ref.steered_batch_search(X, G, ones, fill=fill, **kw)
        for f in FIELDS:
            assert np.array_equal(got[f], want[f]), (fill, f)
        assert not got["bridge_rows"].any() and not got["hop2_cmps"].any()


@pytest.mark.parametrize("frac", [0.4, 0.05])
@pytest.mark.parametrize("dtype,metric,beam", PIN, ids=PIN_IDS)
def test_result_rule_hook_and_pruned_bound(oracle, dtype, metric, beam, frac):
    X, G, kw = _case(dtype, metric, beam)
    allow = np.random.default_rng(24 + beam).random(N) < frac
    allow[5] = False                                                      # one start point is disallowed
    starts, ok = set(kw["starts"]), kw["out_k"]
    bridged = 0
    for fill, dl in ((1, None), (DEG // 2, None), (0, None), (DEG + 5, None), (3, 11)):
        log = [[] for _ in range(NQ)]
        g = steered_ref.steered_batch_search(X, G, allow, fill=fill, degree_limit=dl,
                                             on_distance=lambda qi, a, v: log[qi].append((v, a)), **kw)
        deg_eff = DEG if dl is None else dl
        f_eff = steered_ref.effective_fill(fill, deg_eff, DEG)
        assert 1 <= f_eff <= deg_eff
        assert (g["max_pruned"] <= f_eff - 1 + deg_eff).all()             # |pruned| <= fill - 1 + deg_eff on every visit
        for qi in range(NQ):
            assert len(log[qi]) == g["dist_cmps"][qi]
            assert all(allow[a] for _, a in log[qi] if a not in starts)   # only start points get a distance while disallowed
            want = sorted({e for e in log[qi] if allow[e[1]]})[:ok]
            assert g["result_count"][qi] == len(want)
            assert g["ids"][qi, :len(want)].tolist() == [a for _, a in want]
            assert g["dists"][qi, :len(want)].tolist() == [v for v, _ in want]
            assert (g["ids"][qi, len(want):] == 0xFFFFFFFF).all() and np.isinf(g["dists"][qi, len(want):]).all()
            n_start_off = sum(1 for s in starts if not allow[s])
            assert g["dist_cmps"][qi] == g["allowed_cmps"][qi] + n_start_off      # apart from the starts, dist_cmps == allowed_cmps
            assert g["hop2_cmps"][qi] <= g["dist_cmps"][qi] - len(starts)
        bridged += int(g["bridge_rows"].sum())
    assert bridged > 0                                                    # the two-hop pass ran


def test_degree_sum_counts_visited_rows_only(oracle):
    X, G, kw = _case(np.uint8, "l2", 64)
    allow = np.random.default_rng(3).random(N) < 0.05
    g = steered_ref.steered_batch_search(X, G, allow, fill=0, **kw)
    for qi in range(NQ):
        v = int(g["visited_count"][qi])
        assert g["degree_sum"][qi] == int(G[g["visited_ids"][qi, :v], 0].sum())
    assert g["bridge_rows"].sum() > 0


# ---- quality: the data of tests/test_delete_cpu.py (as tests/test_masked_ref_cpu.py builds it) ------------------------------
QN, QD, QR, QL, QALPHA, QBEAM, QK, QNQ, QSEED = 2000, 32, 32, 64, 1.2, 32, 10, 200, 1
FRACTIONS = (0.50, 0.20, 0.05, 0.01)


def test_quality_against_the_masked_search(oracle):
    """Tie-aware recall@10 against the exact allowed neighbours, steered (fill = deg) and masked, beam 32, 200 queries, one seed.
    Measured while this test was written -- the table is in DESIGN.md "Steered masked search":

        allowed   recall steered / masked   mean dist_cmps steered / masked   mean bridge_rows
        50 %      0.9945 / 0.9745           1164.3 / 665.2                    147.2
        20 %      0.9985 / 0.9460            760.0 / 665.2                    509.9
         5 %      0.9995 / 0.8210            146.9 / 665.2                    680.3
         1 %      0.9795 / 0.4865             25.8 / 665.2                    452.2
    """
    X = datasets.sift_like(QN, QD, seed=1000 + QSEED, dtype=np.uint8)
    Q = datasets.sift_like(QNQ, QD, seed=2000 + QSEED, dtype=np.uint8)
    G, _ = oracle.vamana_build(X, QR, QL, QALPHA, num_passes=1, seed=QSEED)
    rows = {}
    for frac in FRACTIONS:
        allow = np.random.default_rng(4000 + int(frac * 1000)).random(QN) < frac
        live = np.flatnonzero(allow).astype(np.uint32)
        gt_local, gt_d = oracle.bruteforce_knn(X[live], Q, min(50, len(live)))
        gt = live[gt_local]
        kq = min(QK, len(live))
        kw = dict(queries=Q, k=QK, beam=QBEAM, starts=(0,))
        s = steered_ref.steered_batch_search(X, G, allow, fill=0, **kw)
        m = masked_ref.masked_batch_search(X, G, allow, **kw)
        for r in (s, m):
            found = r["ids"][r["ids"] != 0xFFFFFFFF]
            assert allow[found].all()
        rows[frac] = (oracle.recall(s["ids"][:, :kq], gt, gt_d, kq), oracle.recall(m["ids"][:, :kq], gt, gt_d, kq),
                      int(s["allowed_cmps"].sum()), int(m["allowed_cmps"].sum()), float(s["dist_cmps"].mean()), float(m["dist_cmps"].mean()),
                      float(s["bridge_rows"].mean()))
        print(f"allowed {frac:.2f}: recall@{kq} steered {rows[frac][0]:.4f} masked {rows[frac][1]:.4f}  allowed_cmps {rows[frac][2]} / "
              f"{rows[frac][3]}  mean dist_cmps {rows[frac][4]:.1f} / {rows[frac][5]:.1f}  mean bridge_rows {rows[frac][6]:.1f}")
    for frac in (0.05, 0.01):
        rs, rm, acs, acm = rows[frac][:4]
        assert rs >= rm, (frac, rs, rm)
        assert acs >= acm, (frac, acs, acm)
