"""The float test helper and its checkers, trusted before any GPU run (no GPU here):
* grid data: the oracle's sequential f32 `distance`, `bruteforce_knn` and `leaf_knn` equal a float64 numpy evaluation bit
  for bit, for the three float element types, both metrics and the 2^s copies -- the property that lets
  tests/test_fast_float_gpu.py demand bit-exactness of every summation order and algebraic form;
* real-valued data: the tolerance checker accepts the oracle's own (sequential f32) results inside the derived bounds,
  and REJECTS three mutations of them -- a checker that always passes would pass everything."""
import numpy as np
import pytest

import float_cases as fc
from parlayann_amd import bfloat16

SCALES = {np.dtype(np.float16): (-14, 12), np.dtype(np.float32): (-40, 40), bfloat16: (-40, 40)}


@pytest.mark.parametrize("dtype", fc.FLOAT_TYPES, ids=fc.type_name)
@pytest.mark.parametrize("metric", ["l2", "mips"])
@pytest.mark.parametrize("d", [32, 96, 200, 256])
def test_grid_oracle_equals_float64_bit_for_bit(oracle, dtype, metric, d):
    for s in (0,) + SCALES[np.dtype(dtype)]:
        c = fc.grid_like(1500, d, 5, dtype, metric, nq=40, s=s)
        X, Q = c.X, c.Q
        Xw = fc.widen(X)
        assert 0.35 < np.mean(Xw < 0) < 0.65 and np.mean(Xw * 2.0 ** -s != np.rint(Xw * 2.0 ** -s)) > 0.5   # signed, fractional
        if np.dtype(dtype) == np.dtype(np.float16) and s == -14:
            assert np.mean((Xw != 0) & (np.abs(Xw) < 2.0 ** -14)) > 0.05                                  # f16 subnormals
        ref = fc.ref_matrix(Q, X, metric)
        # the same distances at every scale: ids unchanged, values times 4^s exactly
        base = fc.ref_matrix(*(lambda b: (b.Q, b.X))(fc.grid_like(1500, d, 5, dtype, metric, nq=40)), metric)
        np.testing.assert_array_equal(ref, base * 4.0 ** s)
        rng = np.random.default_rng(d)
        for i, j in zip(rng.integers(0, len(Q), 60), rng.integers(0, len(X), 60)):
            got = np.float32(oracle.distance(Q[i], X[j], metric))
            assert got == np.float32(ref[i, j]) and np.float64(got) == ref[i, j]
        for k in (10, 100):
            oi, od = oracle.bruteforce_knn(X, Q, k, metric)
            ei, ed = fc.f64_knn(ref, k)
            np.testing.assert_array_equal(oi, ei)
            np.testing.assert_array_equal(od, ed)
        ids = rng.choice(len(X), 300, replace=False).astype(np.uint32)
        ids[:4] = [c.planted["dup"][0][0], c.planted["dup"][0][1], c.planted["zero"][0], c.planted["neg"][0]]
        ids = np.unique(ids).astype(np.uint32)
        li, ld = oracle.leaf_knn(X, ids, 10, metric)
        sub = fc.ref_matrix(X[ids], X[ids], metric)
        ei, ed = fc.f64_knn(sub, 10, exclude=np.arange(len(ids)))
        np.testing.assert_array_equal(li, ids[ei])
        np.testing.assert_array_equal(ld, ed)


def test_grid_plants_what_it_promises():
    c = fc.grid_like(5000, 128, 3, np.float16, "mips", nq=64)
    Xw, Qw = fc.widen(c.X), fc.widen(c.Q)
    p = c.planted
    assert not Xw[p["zero"][0]].any()
    for a, b in p["dup"]:
        assert np.array_equal(Xw[a], Xw[b]) and a != b
    assert np.array_equal(Xw[p["neg"][0]], -Xw[p["neg"][1]]) and Xw[p["neg"][0]].any()
    assert not (Qw[6:] @ Xw[p["orth"]].T).any() and Xw[p["orth"][0]].any()              # orthogonal to the padded queries
    assert np.signbit(Xw[:, -1]).sum() > 4900 and (Xw[:, -1] == 0).sum() > 10             # -0.0 in the table
    for qi in p["queries"]["mixed"]:
        ip = np.sort(Qw[qi] @ Xw.T)[::-1][:100]
        assert ip[0] > 0 and (ip == 0).any() and ip[-1] < 0                                # all three signs inside one top-100
    with pytest.raises(AssertionError):                                                    # sums leave 2^24 / 64: refused
        fc.assert_grid_exact(np.full((2, 700), 100.0), np.zeros((0, 700)), 0, np.float32)
    with pytest.raises(AssertionError):                                                    # 51 200 * 2 is no f16
        fc.grid_like(500, 64, 1, np.float16, "l2", s=13)
    with pytest.raises(AssertionError):                                                    # below the f16 subnormals
        fc.grid_like(500, 64, 1, np.float16, "l2", s=-22)


def _real_case(oracle, name, dtype, metric, k=10):
    X, Q = fc.real_set(name, 3000, 40, dtype)
    ref = fc.ref_matrix(Q, X, metric)
    tol = fc.tolerances(Q, X, metric, fc.gather_form(metric), ref=ref if metric == "l2" else None)   # sequential f32 = difference form
    ids, dists = oracle.bruteforce_knn(X, Q, k, metric)
    return ref, tol, ids, dists


@pytest.mark.parametrize("dtype", fc.FLOAT_TYPES, ids=fc.type_name)
@pytest.mark.parametrize("name,metric", [("deep", "l2"), ("deep", "mips"), ("t2i", "mips"), ("t2i", "l2"), ("offset", "l2"),
                                         ("offset", "mips")])
def test_checker_accepts_the_sequential_f32_reference(oracle, name, dtype, metric):
    ref, tol, ids, dists = _real_case(oracle, name, dtype, metric, k=100)
    st = fc.Stats()
    fc.check_topk(ids, dists, ref, tol, metric == "l2", stats=st, what=name)
    assert st.err_over_tol <= 1.0
    X, Q = fc.real_set(name, 3000, 40, dtype)
    a = np.arange(0, 400); b = (a * 7 + 3) % 3000
    b[:3] = [3000 // 2, 1, 5]; a[:3] = [3000 // 5, 2999, 5]                      # the planted duplicates and a row with itself
    got = np.array([oracle.distance(X[i], X[j], metric) for i, j in zip(a, b)], np.float32)
    fc.check_dists(got, fc.ref_pairs(X[a], X[b], metric), fc.tolerances_pairs(X[a], X[b], metric, fc.gather_form(metric)),
                   metric == "l2", stats=st)
    if metric == "l2":
        assert (got[:3] == 0).all()
    # the norm-form bound contains the difference-form bound
    if metric == "l2":
        assert (fc.tolerances(Q, X, "l2", "norm") >= tol).all()


@pytest.mark.parametrize("name,metric", [("deep", "l2"), ("t2i", "mips"), ("offset", "l2")])
def test_checker_rejects_mutations(oracle, name, metric):
    k = 10
    ref, tol, ids, dists = _real_case(oracle, name, np.float16, metric, k)
    l2 = metric == "l2"
    fc.check_topk(ids, dists, ref, tol, l2)
    far_i, far_d = oracle.bruteforce_knn(*fc.real_set(name, 3000, 40, np.float16), k + 5, metric)
    # 1. one neighbour swapped for the (k+5)-th (with that point's own correct distance: only completeness can see it)
    for slot in (k - 1, 3):
        i2, d2 = ids.copy(), dists.copy()
        i2[7, slot], d2[7, slot] = far_i[7, k + 4], far_d[7, k + 4]
        if slot != k - 1:                                        # keep the row sorted: the mutation is the missing neighbour
            o = np.lexsort((i2[7], d2[7])); i2[7], d2[7] = i2[7][o], d2[7][o]
        with pytest.raises(AssertionError, match="closer than the last neighbour"):
            fc.check_topk(i2, d2, ref, tol, l2)
    # 2. one distance moved by 4 x tol (the last slot, upwards: the row stays sorted)
    for sign in (1.0, -1.0):
        d2 = dists.copy()
        slot = k - 1 if sign > 0 else 0
        t = tol[5, ids[5, slot]]
        assert t > 0
        d2[5, slot] = np.float32(d2[5, slot] + sign * 4.0 * t)
        assert d2[5, slot] != dists[5, slot]
        with pytest.raises(AssertionError, match="outside the bound"):
            fc.check_topk(ids, d2, ref, tol, l2)
    pd = np.array([dists[5, 0]], np.float64)
    with pytest.raises(AssertionError, match="outside the bound"):
        fc.check_dists(pd + 4.0 * tol[5, ids[5, 0]], ref[5, ids[5, :1]], tol[5, ids[5, :1]], l2)
    # 3. a row with a duplicated id
    i2, d2 = ids.copy(), dists.copy()
    i2[9, 4], d2[9, 4] = i2[9, 3], d2[9, 3]
    with pytest.raises(AssertionError, match="duplicated id"):
        fc.check_topk(i2, d2, ref, tol, l2)
    # and the rest of what the checker promises: order, tie order, sign, range
    d2 = dists.copy(); d2[2, 4], d2[2, 5] = dists[2, 5], dists[2, 4]
    if d2[2, 4] != d2[2, 5]:
        with pytest.raises(AssertionError):
            fc.check_topk(ids, d2, ref, tol, l2)
    i2 = ids.copy(); i2[0, 0] = 3000
    with pytest.raises(AssertionError, match="out of range"):
        fc.check_topk(i2, dists, ref, tol, l2)
    if l2:
        q = 1                                                    # the query that equals two base rows: true distance 0
        assert dists[q, 0] == 0 and dists[q, 1] == 0 and ids[q, 0] < ids[q, 1]
        d2 = dists.copy(); d2[q, 0] = -1e-30
        with pytest.raises(AssertionError):
            fc.check_topk(ids, d2, ref, tol + 1e-20, l2)         # inside a (widened) bound, still refused: negative L2
        i2 = ids.copy(); i2[q, 0], i2[q, 1] = ids[q, 1], ids[q, 0]
        with pytest.raises(AssertionError, match="not ordered by id"):
            fc.check_topk(i2, dists, ref, tol, l2)
