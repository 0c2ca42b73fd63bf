"""The second-sighting rule of the beam-64 search ("Second sightings") on the CPU: tests/seen_ref.py walks as the
reference does except that a neighbour which the lossy filter lets through again, and which the table V still knows, gets no
distance -- its outcome is read off the frontier and the pending candidates.  Every output must equal the C++ oracle's, which
computes every distance, and the rule must actually fire."""
import numpy as np
import pytest

import seen_ref
from parlayann_amd import datasets

N, D, R, L, NQ = 20_000, 32, 32, 64, 200
FIELDS = ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum")
BIG_CUT = 1e30          # "off": a threshold nothing exceeds


@pytest.fixture(scope="module")
def case(oracle):
    X = datasets.sift_like(N, D, seed=71, dtype=np.uint8)
    Q = datasets.sift_like(NQ, D, seed=72, dtype=np.uint8)
    G, _ = oracle.vamana_build(X, R, L, 1.15, num_passes=1, seed=3)
    return X, Q, G


def check(oracle, X, G, v_n=512, min_skipped=1, **kw):
    o = oracle.batch_search(X, G, **kw)
    assert o["rc"] == 0
    g = seen_ref.seen_batch_search(X, G, v_n=v_n, **kw)
    for f in FIELDS:
        assert np.array_equal(g[f], o[f]), f
    print(f"v_n {v_n} {({k: v for k, v in kw.items() if k not in ('queries', 'query_ids', 'starts')})} {len(kw.get('starts', (0,)))} start(s): per query cmps {o['dist_cmps'].mean():.1f} "
          f"repeats {g['repeats'].mean():.1f} lookups {g['lookups'].mean():.1f} skipped {g['skipped'].mean():.1f}")
    assert g["skipped"].sum() >= min_skipped
    return g


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("cut", [1.0, 1.35, BIG_CUT], ids=["cut1.0", "cut1.35", "cutoff"])
def test_model_equals_the_oracle(oracle, case, cut, k):
    X, Q, G = case
    # cut = 1.0 prunes everything beyond entry k, so a frontier never grows past max(k, its start points): it is full, and V
    # is consulted, only when the search starts with `beam` points
    starts = tuple(range(0, 64 * 311, 311)) if cut == 1.0 else (0,)
    check(oracle, X, G, queries=Q, k=k, beam=64, cut=cut, starts=starts, out_k=max(k, 10))


def test_rule_stays_off_when_a_prune_leaves_k_entries_or_fewer(oracle, case):
    """cut = 1.0, eight start points, k = 10: ten entries after every merge -- the prune threshold is then not monotone, the
    model (as the kernel) stops consulting V for good, and the frontier never fills anyway"""
    X, Q, G = case
    g = check(oracle, X, G, queries=Q[:64], k=10, beam=64, cut=1.0, starts=tuple(range(0, 8 * 997, 997)), min_skipped=0)
    assert g["lookups"].sum() == 0 and g["skipped"].sum() == 0 and (g["frontier_size"] <= 11).all()


def test_model_other_paths(oracle, case):
    X, Q, G = case
    qid = np.arange(0, N, N // 64, dtype=np.uint32)[:64]
    check(oracle, X, G, query_ids=qid, k=10, beam=64, cut=1.35, out_k=64)                          # self exclusion
    check(oracle, X, G, queries=Q[:64], k=0, beam=64, cut=0.0, out_k=64)                            # the builder's call: no cut-prune
    check(oracle, X, G, queries=Q[:64], k=10, beam=40, cut=1.35, degree_limit=20, out_k=40)        # beam < 64, degree_limit < R
    check(oracle, X, G, queries=Q[:64], k=10, beam=64, cut=1.35, limit=30, min_skipped=0)           # limit < 2 * beam: no skipped merges
    check(oracle, X, G, queries=Q[:64], k=10, beam=64, cut=1.35, v_n=256)
    check(oracle, X, G, queries=Q[:64], k=10, beam=64, cut=0.0, min_skipped=0)                      # cut = 0: the frontier never grows


def test_victims_catch_more_than_every_compared_id(oracle, case):
    """the measurement behind the insertion policy, at this file's shape"""
    X, Q, G = case
    kw = dict(queries=Q[:64], k=10, beam=64, cut=1.35)
    v = seen_ref.seen_batch_search(X, G, v_n=512, **kw)
    a = seen_ref.seen_batch_search(X, G, v_n=512, insert="all", **kw)
    o = oracle.batch_search(X, G, **kw)
    for f in FIELDS:
        assert np.array_equal(a[f], o[f]), f
    print(f"skipped per query: victims {v['skipped'].mean():.1f}, every compared id {a['skipped'].mean():.1f}, "
          f"repeats {v['repeats'].mean():.1f} of {o['dist_cmps'].mean():.1f} comparisons")
    assert v["skipped"].sum() > a["skipped"].sum() > 0
    assert (v["skipped"] <= v["repeats"]).all()
