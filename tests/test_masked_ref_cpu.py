"""CPU-only checks of the masked search's rule and of its test infrastructure (DESIGN.md "Masked search"):

* tests/masked_ref.py walks exactly as the C++ oracle does, whatever the mask holds (the checker is pinned before the device is
  compared against it);
* its result equals an independent statement of the rule: sort the set of (allowed, compared) points recorded by a wrapper
  around the distance call;
* the post-filter answer (allowed entries of the plain search's final frontier) is element-wise >= the masked result;
* on the data of tests/test_delete_cpu.py the masked result's tie-aware recall is >= the post-filter baseline's: an exact
  inequality, the masked list is the top-k of a superset;
* every case of tests/test_masked_search_gpu.py meets the regime it is there for, so that no device test passes vacuously;
* the new C-ABI symbols exist, the ABI version is still 3, and the bitmap helpers pack as the header says.
"""
import ctypes as C

import numpy as np
import pytest

import delete_ref as dr
import filtered_cases as fc
from filtered_cases import random_rows as _data
import masked_cases as mc
import masked_ref
from parlayann_amd import datasets

TRAVERSAL = ("frontier_size", "visited_count", "dist_cmps", "degree_sum")


PIN = [(dt, m, beam) for dt, m in ((np.uint8, "l2"), (np.int8, "mips"), (np.float32, "l2")) for beam in (8, 64, 200)]
PIN_N, PIN_NQ = 1200, 8


def _pin_case(dtype, metric, beam):
    X, Q = _data(dtype, PIN_N, 24, 11 + beam), _data(dtype, PIN_NQ, 24, 12 + beam)
    G = fc.random_graph(PIN_N, 16, 13 + beam)
    kw = dict(k=min(10, beam), beam=beam, metric=metric, out_k=min(beam, 64), visited_cap=PIN_N, queries=Q)
    allow = np.random.default_rng(14 + beam).random(PIN_N) < 0.4
    return X, G, kw, allow


@pytest.mark.parametrize("dtype,metric,beam", PIN, ids=[f"{np.dtype(d).name}-{m}-b{b}" for d, m, b in PIN])
def test_traversal_equals_the_oracle_for_any_mask(oracle, dtype, metric, beam):
    X, G, kw, allow = _pin_case(dtype, metric, beam)
    r = oracle.batch_search(X, G, **kw)
    assert r["rc"] == 0
    runs = [masked_ref.masked_batch_search(X, G, a, **kw) for a in (allow, np.ones(PIN_N, bool), np.zeros(PIN_N, bool))]
    for g in runs:
        for f in TRAVERSAL:
            assert np.array_equal(g[f], r[f]), f
        assert np.array_equal(g["frontier_ids"], r["ids"]) and np.array_equal(g["frontier_dists"], r["dists"])
        for i in range(PIN_NQ):
            v = int(r["visited_count"][i])
            assert np.array_equal(g["visited_ids"][i, :v], r["visit_order_ids"][i, :v])
    assert (runs[0]["ids"] != runs[1]["ids"]).any()                       # the mask does change the result
    assert (runs[2]["result_count"] == 0).all() and (runs[2]["ids"] == 0xFFFFFFFF).all() and np.isinf(runs[2]["dists"]).all()
    assert (runs[2]["allowed_cmps"] == 0).all() and np.array_equal(runs[1]["allowed_cmps"], r["dist_cmps"])


@pytest.mark.parametrize("dtype,metric,beam", PIN, ids=[f"{np.dtype(d).name}-{m}-b{b}" for d, m, b in PIN])
def test_result_is_the_sorted_set_of_allowed_compared_points(dtype, metric, beam):
    X, G, kw, allow = _pin_case(dtype, metric, beam)
    log = [[] for _ in range(PIN_NQ)]
    g = masked_ref.masked_batch_search(X, G, allow, on_distance=lambda qi, a, v: log[qi].append((v, a)), **kw)
    ok = kw["out_k"]
    for qi in range(PIN_NQ):
        assert len(log[qi]) == g["dist_cmps"][qi]                         # every full distance went through the hook
        want = sorted({e for e in log[qi] if allow[e[1]]})[:ok]
        assert g["result_count"][qi] == len(want)
        assert g["ids"][qi, :len(want)].tolist() == [a for _, a in want]
        assert g["dists"][qi, :len(want)].tolist() == [v for v, _ in want]
        assert (g["ids"][qi, len(want):] == 0xFFFFFFFF).all() and np.isinf(g["dists"][qi, len(want):]).all()
        assert g["allowed_cmps"][qi] == sum(1 for e in log[qi] if allow[e[1]])
        assert len(set(g["ids"][qi, :len(want)].tolist())) == len(want)   # a point compared twice is listed once
    # the post-filter answer is never better, entry by entry (padding = +inf, 0xFFFFFFFF)
    pid, pd = masked_ref.post_filter(g, allow, ok)
    key = lambda d, i: list(zip(d.tolist(), i.tolist()))
    for qi in range(PIN_NQ):
        assert all(p >= m for p, m in zip(key(pd[qi], pid[qi]), key(g["dists"][qi], g["ids"][qi])))
    if beam == 8:                  # a small beam throws compared points away: there the two answers must differ somewhere
        assert (pd > g["dists"]).any() or (pid != g["ids"]).any()


# ---- quality: the data of tests/test_delete_cpu.py -------------------------------------------------------------
QN, QD, QR, QL, QALPHA, QBEAM, QK, QNQ = 2000, 32, 32, 64, 1.2, 32, 10, 200


def quality(oracle, seed):
    """tie-aware recall@10 over the allowed points of (masked result, post-filter baseline); 20 % of the points disallowed"""
    X = datasets.sift_like(QN, QD, seed=1000 + seed, dtype=np.uint8)
    Q = datasets.sift_like(QNQ, QD, seed=2000 + seed, dtype=np.uint8)
    G, _ = oracle.vamana_build(X, QR, QL, QALPHA, num_passes=1, seed=seed)
    D = dr.seeded_ids(QN, 0.20, 3000 + seed, keep=(0,))
    allow = np.ones(QN, bool); allow[D] = False
    live = np.flatnonzero(allow).astype(np.uint32)
    gt_local, gt_d = oracle.bruteforce_knn(X[live], Q, 50)
    gt = live[gt_local]
    g = masked_ref.masked_batch_search(X, G, allow, queries=Q, k=QK, beam=QBEAM, starts=(0,))
    pid, _ = masked_ref.post_filter(g, allow, QK)
    return oracle.recall(g["ids"], gt, gt_d, QK), oracle.recall(pid, gt, gt_d, QK), g, allow


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_masked_recall_is_at_least_the_post_filter_baseline(oracle, seed):
    """Measured while this test was written (recall@10 masked / post-filter): the figures are in DESIGN.md "Masked search"."""
    masked, post, g, allow = quality(oracle, seed)
    print(f"seed {seed}: recall@10 masked {masked:.4f} post-filter {post:.4f}")
    found = g["ids"][g["ids"] != 0xFFFFFFFF]
    assert allow[found].all()                               # hard: a disallowed id is never returned
    assert masked >= post


# ---- the GPU cases are not vacuous -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.CASES, ids=mc.CASE_IDS)
def test_gpu_cases_meet_their_regime(oracle, case):
    name, layout, deg, kw, mkind, regime = case
    r = mc.case_reference(case)
    X, Q, metric, _ = mc.layout_data(layout)
    q = dict(query_ids=mc.QUERY_IDS) if kw.get("query_ids") else dict(queries=Q)
    o = oracle.batch_search(X, mc.graph(deg), metric=metric, **q, **mc.search_kw(kw))
    for f in TRAVERSAL:                                     # the restatement walks as the oracle does on this very case
        assert np.array_equal(r[f], o[f]), f
    assert np.array_equal(r["frontier_ids"], o["ids"])
    beam = kw["beam"]
    if beam > 1:
        assert (r["visited_count"] > 1).all()
    if mkind in ("rand50", "rows_differ", "far_only"):
        assert (r["result_count"] == kw["out_k"]).all() and (r["ids"] != r["frontier_ids"]).any()
    if mkind == "start_off":
        starts = list(kw.get("starts", (0,)))
        assert not np.isin(r["ids"], starts).any() and np.isin(r["frontier_ids"], starts).any()
    if mkind == "only_start":
        assert (r["result_count"] == 1).all() and (r["ids"][:, 0] == 0).all()
    if regime == "recompared":
        assert r["recompared_in_result"].sum() > 0, "no re-compared point in any result"
    if regime == "short":
        assert (r["result_count"] < kw["out_k"]).any() and (r["result_count"] > 0).any()
    if regime == "empty":
        assert (r["result_count"] == 0).all() and (r["allowed_cmps"] == 0).all()
    if regime == "beyond_cutoff":
        assert r["from_beyond_cutoff"].sum() > 0 and (r["frontier_size"] == beam).all()
    if regime == "unmerged":
        assert r["from_unmerged"].sum() > 0 and (r["visited_count"] == kw["limit"]).any()
    if regime == "skip_off":
        assert kw["limit"] < 2 * beam and (r["visited_count"] == kw["limit"]).all()
    if deg == 96:
        assert (r["degree_sum"] > 64 * r["visited_count"]).all()
    if name == "u8-b64-rand50":                             # ids of the last bitmap word take part, with both verdicts
        m = mc.mask(mkind, layout)
        assert m[mc.N - 5] and not m[mc.N - 4]
        packed = mc.pack(m)
        assert packed.shape == (mc.WORDS,) and packed[-1] >> 25 == (1 << 7) - 1          # the dead bits are set
        assert np.array_equal(masked_ref.unpack_allow(packed, mc.N, 1)[0], m)


def test_last_word_ids_reach_a_result(oracle):
    """some query of some case returns an id >= 2976 (the last bitmap word), and one case compares a disallowed id there"""
    hit = False
    for case in mc.CASES[:1] + [c for c in mc.CASES if c[0] == "u8-b300-o64-rand5"]:
        r = mc.case_reference(case)
        found = r["ids"][r["ids"] != 0xFFFFFFFF]
        hit |= bool((found >= (mc.WORDS - 1) * 32).any())
    assert hit


def test_line_case_overflows_the_default_dropped_list(oracle):
    X, G, Q, allow = mc.line_case()
    o = oracle.batch_search(X, G, queries=Q, k=1, beam=16, cut=1.0, out_k=2)
    assert o["visited_count"].max() > 600


# ---- host-only surface -------------------------------------------------------------------------------------------
def test_new_symbols_exported_and_bound():
    from parlayann_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    for s in ("pann_batch_search_masked", "pann_batch_search_masked_dev"):
        assert hasattr(lib, s), s
        assert s in _capi.SIGNATURES, s
    assert len(_capi.SIGNATURES["pann_batch_search_masked"][1]) == 13
    assert len(_capi.SIGNATURES["pann_batch_search_masked_dev"][1]) == 14
    assert _capi.load().pann_abi_version() == 3


def test_bitmap_helpers():
    from parlayann_amd import allow_bitmap
    from parlayann_amd.index import pack_allow
    a = allow_bitmap(70)
    assert a.dtype == np.uint32 and a.tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 0x3F]       # bits >= n stay clear
    assert allow_bitmap(70, allowed_ids=[0, 33, 69]).tolist() == [1, 2, 1 << 5]
    assert allow_bitmap(70, deleted_ids=[31, 32]).tolist() == [0x7FFFFFFF, 0xFFFFFFFE, 0x3F]
    assert allow_bitmap(70, allowed_ids=[1, 2], deleted_ids=[2]).tolist() == [2, 0, 0]
    m = np.random.default_rng(1).random((3, mc.N)) < 0.5
    p = pack_allow(m, mc.N)
    assert p.shape == (3, mc.WORDS) and np.array_equal(masked_ref.unpack_allow(p, mc.N, 3), m)
    assert np.array_equal(p, mc.pack(m, stray_bits=False))
    assert pack_allow(p, mc.N) is not None and np.array_equal(pack_allow(p[0], mc.N), p[0])
    with pytest.raises(ValueError):
        pack_allow(np.ones(mc.N - 1, bool), mc.N)
    with pytest.raises(ValueError):
        pack_allow(np.ones(mc.WORDS - 1, np.uint32), mc.N)


def test_null_handle_is_an_error_not_a_crash():
    from parlayann_amd import _capi
    lib = _capi.load()
    rc = lib.pann_batch_search_masked(None, None, None, 0, 0, None, 0, None, None, 0, None, None, None)
    assert rc != 0 and lib.pann_last_error()
