"""GPU checks of the exact range ground truth (pann_bruteforce_range -> csrc/range_gt.hip), of the beam-seeded range query
(pann_range_query) and of the recall that ties the two together.  Expected values come from numpy (int64 / float64),
tests/float_cases.py and the CPU oracle; nothing here is derived from what the device returns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import float_cases as fc
from parlayann_amd import DeviceIndex, PannError, _capi, bfloat16, datasets, io, to_bf16
from parlayann_amd.recall import range_recall

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(off, ids):
    return [ids[int(off[i]): int(off[i + 1])] for i in range(len(off) - 1)]


def _expect_csr(inside):
    """boolean nq x n matrix -> (offsets, ids): ids of a row ascending"""
    off = np.zeros(len(inside) + 1, np.uint64)
    off[1:] = np.cumsum(inside.sum(1))
    return off, np.nonzero(inside)[1].astype(np.uint32)


def _check_csr(got, inside, what):
    off, ids = got
    eoff, eids = _expect_csr(inside)
    assert off.dtype == np.uint64 and ids.dtype == np.uint32
    np.testing.assert_array_equal(off, eoff, err_msg=f"{what}: offsets")
    np.testing.assert_array_equal(ids, eids, err_msg=f"{what}: ids")


def _int_data(n, nq, d, dtype):
    X = datasets.sift_like(n, d, seed=1234, dtype=np.float32)
    Q = datasets.sift_like(nq, d, seed=4321, dtype=np.float32)
    if dtype == np.int8:
        X, Q = (X - 128).clip(-127, 127), (Q - 128).clip(-127, 127)
    return X.astype(dtype), Q.astype(dtype)


def _int_dists(X, Q, metric):
    """exact int64 distances (float64 products of one-byte values and their sums over d <= 200 are exact)"""
    Xf, Qf = X.astype(np.float64), Q.astype(np.float64)
    dot = Qf @ Xf.T
    if metric == "mips":
        return (-dot).astype(np.int64)
    return ((Qf * Qf).sum(1)[:, None] + (Xf * Xf).sum(1)[None, :] - 2.0 * dot).astype(np.int64)


# ---- 1. integer types: exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 100, 128, 200])
@pytest.mark.parametrize("dtype,metric", [(np.uint8, "l2"), (np.int8, "l2"), (np.int8, "mips")])
def test_integer_types_equal_int64_brute_force(dtype, metric, d):
    n, nq = 10007, 130                      # no multiple of any tile
    X, Q = _int_data(n, nq, d, dtype)
    D = _int_dists(X, Q, metric)
    Df = D.astype(np.float32)               # the reference's distanceType: one cast of the integer sum (exact below 2^24)
    assert np.abs(D).max() < 2 ** 24
    ix = DeviceIndex(X, max_degree=4, metric=metric)
    r_med = float(np.median(np.partition(Df, 29, axis=1)[:, 29]))
    r_tie = float(Df[7, 1234])              # IS a pair's distance: == is inside
    assert (Df == np.float32(r_tie)).any()
    for name, r in (("median30", r_med), ("tie", r_tie)):
        inside = Df <= np.float32(r)
        assert inside.any() and not inside.all()
        _check_csr(ix.bruteforce_range(Q, r), inside, f"{name} r={r}")
    off, ids = ix.bruteforce_range(Q, float(Df.min()) - 1.0)                    # below every distance
    assert (off == 0).all() and len(off) == nq + 1 and len(ids) == 0
    off, ids = ix.bruteforce_range(Q, float(Df.max()) + 1.0)                    # above every distance
    np.testing.assert_array_equal(off, np.arange(nq + 1, dtype=np.uint64) * n)
    np.testing.assert_array_equal(ids.reshape(nq, n), np.broadcast_to(np.arange(n, dtype=np.uint32), (nq, n)))
    ix.close()


# ---- 1b. two-byte floats on the matrix cores, unaligned query rows -----------------------------------------------------------
@pytest.mark.parametrize("d", [100, 132])
@pytest.mark.parametrize("metric", ["l2", "mips"])
@pytest.mark.parametrize("dtype", [np.float16, bfloat16], ids=["f16", "bf16"])
def test_two_byte_floats_unaligned_query_rows(dtype, metric, d):
    """range_join_mfma_kernel, one (d = 100) and two (d = 132) segments; the query rows are packed at 200 / 264 bytes, so every
    odd row starts 8 bytes off a 16-byte boundary.  Values are integers in 0..15: every product and every sum is an integer far
    below 2^24, so the norm form |a|^2 + |b|^2 - 2 a.b is exact in f32 and equals the int64 brute force."""
    n, nq = 1003, 70
    rng = np.random.default_rng(1000 + d)
    Xi, Qi = rng.integers(0, 16, (n, d)), rng.integers(0, 16, (nq, d))
    cast = (lambda a: to_bf16(a.astype(np.float32))) if np.dtype(dtype) == bfloat16 else (lambda a: a.astype(dtype))
    X, Q = cast(Xi), cast(Qi)
    assert Q.flags.c_contiguous and (Q.strides[0] % 16) == 8
    dot = Qi.astype(np.int64) @ Xi.astype(np.int64).T
    D = -dot if metric == "mips" else (Qi * Qi).sum(1)[:, None] + (Xi * Xi).sum(1)[None, :] - 2 * dot
    assert np.abs(D).max() < 2 ** 24
    r = float(np.median(D))
    inside = D <= r
    assert inside.any() and not inside.all()
    ix = DeviceIndex(X, max_degree=4, metric=metric)
    _check_csr(ix.bruteforce_range(Q, r), inside, f"{metric} d={d} r={r}")
    ix.close()


# ---- 2. grid floats: exact in any order and any algebraic form -------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 6, -6])
@pytest.mark.parametrize("metric", ["l2", "mips"])
@pytest.mark.parametrize("dtype", fc.FLOAT_TYPES, ids=fc.type_name)
def test_grid_floats_bit_exact(dtype, metric, s):
    n, nq = 5003, 70
    for d in (128, 200):
        g = fc.grid_like(n, d, 77 + d, dtype, metric, nq=nq, s=s)
        ref = fc.ref_matrix(g.Q, g.X, metric)
        ix = DeviceIndex(g.X, max_degree=4, metric=metric)
        r = np.float32(np.median(np.partition(ref, 29, axis=1)[:, 29]))
        inside = ref <= np.float64(r)
        assert inside.any() and not inside.all()
        _check_csr(ix.bruteforce_range(g.Q, float(r)), inside, f"{fc.type_name(dtype)} {metric} d={d} s={s}")
        if metric == "l2":                  # r = 0: the planted duplicates and the query that equals a base row, nothing else
            zero = ref == 0.0
            got = ix.bruteforce_range(g.Q, 0.0)
            _check_csr(got, zero, f"{fc.type_name(dtype)} r=0 d={d} s={s}")
            rows = _rows(*got)
            np.testing.assert_array_equal(rows[g.planted["queries"]["dup"]], sorted([n // 5, n // 2]))
            np.testing.assert_array_equal(rows[g.planted["queries"]["zero"]], g.planted["zero"])
            assert int(got[0][-1]) == int(zero.sum())
        ix.close()


# ---- 3. real-valued floats, default mode: decided outside the derived bound ---------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "mips"])
@pytest.mark.parametrize("dtype", fc.FLOAT_TYPES, ids=fc.type_name)
@pytest.mark.parametrize("name", sorted(fc.REAL_SETS))
def test_real_valued_floats_within_the_derived_bound(name, dtype, metric):
    """the kernel's forms are those of dense_form: difference form for f32, norm form (matrix cores) for f16 / bf16, inner
    product for MIPS"""
    n, nq = 20000, 100
    X, Q = fc.real_set(name, n, nq, dtype)
    ref = fc.ref_matrix(Q, X, metric)
    tol = fc.tolerances(Q, X, metric, fc.dense_form(dtype, metric), ref=ref if metric == "l2" else None)
    ix = DeviceIndex(X, max_degree=4, metric=metric)
    for rank in (30, 300):
        r = np.float32(np.median(np.partition(ref, rank - 1, axis=1)[:, rank - 1]))
        r64 = np.float64(r)
        must = ref <= r64 - tol
        never = ref > r64 + tol
        band = int((~must & ~never).sum())
        matches = int((ref <= r64).sum())
        print(f"{name} {fc.type_name(dtype)} {metric} rank {rank}: {matches} matches, undecided band {band}")
        assert band <= 0.01 * matches, (band, matches)          # a cap on the test's own inputs, before the device is asked
        off, ids = ix.bruteforce_range(Q, float(r))
        got = np.zeros((nq, n), bool)
        for i, row in enumerate(_rows(off, ids)):
            assert (np.diff(row.astype(np.int64)) > 0).all(), f"row {i}: ids not ascending and distinct"
            assert len(row) == 0 or row[-1] < n
            got[i, row] = True
        assert not (must & ~got).any(), f"rank {rank}: {int((must & ~got).sum())} pairs inside by more than the bound are missing"
        assert not (never & got).any(), f"rank {rank}: {int((never & got).sum())} pairs outside by more than the bound are reported"
    ix.close()


# ---- 4. exact float order -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "mips"])
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_exact_float_order_equals_the_sequential_oracle(oracle, dtype, metric):
    n, nq = 3000, 60
    X = datasets.deep_like(n, 96, seed=1234).astype(dtype); Q = datasets.deep_like(nq, 96, seed=4321).astype(dtype)
    gi, gd = oracle.bruteforce_knn(X, Q, n, metric)              # every distance, sequential f32 sums
    ix = DeviceIndex(X, max_degree=4, metric=metric, exact_float_order=True)
    for rank in (30, 400):
        r = np.float32(np.median(gd[:, rank - 1]))
        rows = _rows(*ix.bruteforce_range(Q, float(r)))
        for i in range(nq):
            want = np.sort(gi[i][gd[i] <= r])
            np.testing.assert_array_equal(rows[i], want, err_msg=f"rank {rank} query {i}")
    ix.close()


# ---- 5. protocol ----------------------------------------------------------------------------------------------------------------
def test_protocol_count_only_overflow_stride_pieces():
    n, nq, d = 10007, 130, 100
    X, Q = _int_data(n, nq, d, np.uint8)
    Df = _int_dists(X, Q, "l2").astype(np.float32)
    r = float(np.median(np.partition(Df, 29, axis=1)[:, 29]))
    eoff, eids = _expect_csr(Df <= np.float32(r))
    total = len(eids)
    ix = DeviceIndex(X, max_degree=4)
    lib, h = _capi.load(), ix.handle
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    # count only
    off = np.full(nq + 1, 99, np.uint64)
    assert lib.pann_bruteforce_range(h, p(Q), nq, d, r, p(off), None, 0) == 0
    np.testing.assert_array_equal(off, eoff)
    # one short: overflow, offsets valid, buffer untouched
    off[:] = 99
    buf = np.full(total, 0xABABABAB, np.uint32)
    assert lib.pann_bruteforce_range(h, p(Q), nq, d, r, p(off), p(buf), total - 1) == _capi.PANN_ERR_OVERFLOW
    assert lib.pann_last_error()
    np.testing.assert_array_equal(off, eoff)
    assert (buf == 0xABABABAB).all()
    # exactly enough
    assert lib.pann_bruteforce_range(h, p(Q), nq, d, r, p(off), p(buf), total) == 0
    np.testing.assert_array_equal(buf, eids)
    # nq = 0
    off0 = np.full(1, 99, np.uint64)
    assert lib.pann_bruteforce_range(h, p(Q), 0, d, r, p(off0), None, 0) == 0 and off0[0] == 0
    o, i = ix.bruteforce_range(Q[:0], r)
    assert len(o) == 1 and o[0] == 0 and len(i) == 0
    # a query stride wider than a row
    wide = np.full((nq, d + 28), 255, np.uint8)
    wide[:, :d] = Q
    off[:] = 99; buf[:] = 0
    assert lib.pann_bruteforce_range(h, p(wide), nq, d + 28, r, p(off), p(buf), total) == 0
    np.testing.assert_array_equal(off, eoff); np.testing.assert_array_equal(buf, eids)
    # bad arguments
    assert lib.pann_bruteforce_range(h, p(Q), nq, d, float("nan"), p(off), None, 0) == 1 and lib.pann_last_error()
    assert lib.pann_bruteforce_range(h, None, nq, d, r, p(off), None, 0) == 1 and lib.pann_last_error()
    assert lib.pann_bruteforce_range(h, p(Q), nq, d, r, None, None, 0) == 1 and lib.pann_last_error()
    assert lib.pann_bruteforce_range(h, p(Q), nq, d - 1, r, p(off), None, 0) == 1 and lib.pann_last_error()
    # results never depend on how the base is cut
    for pieces in (1, 3, 8):
        ix.set_option("gt_pieces", pieces)
        o, i = ix.bruteforce_range(Q, r)
        np.testing.assert_array_equal(o, eoff, err_msg=f"gt_pieces={pieces}")
        np.testing.assert_array_equal(i, eids, err_msg=f"gt_pieces={pieces}")
    ix.close()


# ---- 6. / 7. range query --------------------------------------------------------------------------------------------------------
def _graph_setup(oracle, n, d, dtype, metric="l2", R=32):
    X, Q = _int_data(n, 200, d, dtype)
    G, _ = oracle.vamana_build(X, R, 2 * R, 1.2 if metric == "l2" else 1.0, seed=5, metric=metric)
    return X, Q, G


def _same(o, g, what):
    np.testing.assert_array_equal(o["counts"], g["counts"], err_msg=what)
    np.testing.assert_array_equal(o["truncated"], g["truncated"], err_msg=what)
    np.testing.assert_array_equal(o["ids"], g["ids"], err_msg=what)


@pytest.mark.parametrize("dtype,metric,d", [(np.uint8, "l2", 128), (np.float16, "l2", 128), (np.float32, "l2", 200),
                                            (np.int8, "mips", 100)])
def test_range_query_equals_search_then_range_search(oracle, dtype, metric, d):
    n = 6000
    X, Q, G = _graph_setup(oracle, n, d, dtype, metric)
    ix = DeviceIndex(X, G, metric=metric)
    r = float(np.median(oracle.bruteforce_knn(X, Q, 40, metric)[1][:, -1]))
    cap = 44                                                     # small enough to truncate some queries, not all
    qid = (np.arange(150, dtype=np.uint32) * 7) % n
    for beam in (10, 48):
        for kw in (dict(queries=Q), dict(query_ids=qid)):
            what = f"beam {beam} {'external' if 'queries' in kw else 'base-point'}"
            g = ix.range_query(radius=r, beam=beam, max_results=cap, **kw)
            s = ix.batch_search(k=beam, beam=beam, cut=0.0, **kw)
            c = ix.range_search(s["ids"], r, cap, **kw)
            _same(c, g, what + " vs device composition")
            np.testing.assert_array_equal(g["search_cmps"], s["dist_cmps"]); np.testing.assert_array_equal(g["visited"], s["visited_count"])
            so = oracle.batch_search(X, G, k=beam, beam=beam, cut=0.0, metric=metric, **kw)
            o = oracle.range_search(X, G, so["ids"], r, cap, metric=metric, **kw)
            _same(o, g, what + " vs oracle composition")
            np.testing.assert_array_equal(g["search_cmps"], so["dist_cmps"]); np.testing.assert_array_equal(g["visited"], so["visited_count"])
            ok = o["truncated"] == 0            # a truncated query stops early; where exactly is not part of the contract
            np.testing.assert_array_equal(g["range_cmps"][ok], o["dist_cmps"][ok])
            np.testing.assert_array_equal(g["range_cmps"], g["dist_cmps"])
            assert o["truncated"].any() and not o["truncated"].all(), what
    with pytest.raises(PannError):
        ix.range_query(Q, radius=r, beam=10, k=20)               # k > beam
    with pytest.raises(PannError):
        ix.range_query(Q, radius=r, beam=10, starts=(n,))
    with pytest.raises(ValueError):
        ix.range_query(radius=r)
    ix.close()


@pytest.mark.parametrize("dtype,metric,d", [(np.uint8, "l2", 128), (np.int8, "mips", 100)])
def test_the_loop_closes_recall_against_the_exact_truth(oracle, dtype, metric, d):
    n = 6000
    X, Q, G = _graph_setup(oracle, n, d, dtype, metric)
    ix = DeviceIndex(X, G, metric=metric)
    r = float(np.median(oracle.bruteforce_knn(X, Q, 40, metric)[1][:, -1]))
    off, ids = ix.bruteforce_range(Q, r)
    truth = _rows(off, ids)
    cap = max(1, max(len(t) for t in truth))
    prev = (0.0, 0.0)
    for beam in (10, 48, 128):
        g = ix.range_query(Q, radius=r, beam=beam, max_results=cap)
        assert not g["truncated"].any()
        for i in range(len(Q)):
            assert np.isin(g["ids"][i, : g["counts"][i]], truth[i]).all(), f"beam {beam} query {i}: a reported id is no true match"
        rec = range_recall(g["ids"], g["counts"], off, ids)
        print(f"{np.dtype(dtype).name} {metric} d={d} beam {beam}: pointwise {rec['pointwise']:.4f} cumulative {rec['cumulative']:.4f} "
              f"reported {rec['reported']} of {rec['total']}")
        assert rec["reported"] == int(g["counts"].sum())         # the intersection is everything that was reported
        assert 0.0 < rec["pointwise"] <= 1.0 and 0.0 < rec["cumulative"] <= 1.0
        assert rec["pointwise"] >= prev[0] and rec["cumulative"] >= prev[1], f"recall fell at beam {beam}"
        prev = (rec["pointwise"], rec["cumulative"])
    ix.close()


# ---- 8. the data_tools CLI --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tp,df", [("uint8", "Euclidian"), ("float", "mips")])
def test_compute_range_groundtruth_cli(tmp_path, tp, df):
    exe = os.path.join(ROOT, "parlayann_amd", "host", "compute_range_groundtruth")
    assert os.path.exists(exe), "build the host mirror first (__graft_entry__.build())"
    n, nq, d = 4001, 90, 64
    if tp == "uint8":
        X, Q = _int_data(n, nq, d, np.uint8)
        D = _int_dists(X, Q, "l2").astype(np.float64)
    else:                                   # integer-valued floats: every sum is exact, so the file is determined
        X, Q = _int_data(n, nq, d, np.int8)
        X, Q = X.astype(np.float32), Q.astype(np.float32)
        D = _int_dists(X, Q, "mips").astype(np.float64)
    r = float(np.float32(np.median(np.partition(D, 19, axis=1)[:, 19])))
    io.write_bin(tmp_path / "base.bin", X); io.write_bin(tmp_path / "query.bin", Q)
    subprocess.run([exe, "-base_path", str(tmp_path / "base.bin"), "-query_path", str(tmp_path / "query.bin"), "-data_type", tp,
                    "-dist_func", df, "-r", repr(r), "-gt_path", str(tmp_path / "cli.gt")], check=True, timeout=300)
    ix = DeviceIndex(X, max_degree=4, metric=df)
    off, ids = ix.bruteforce_range(Q, r)
    ix.close()
    _check_csr((off, ids), D <= r, "python result")
    io.write_range_gt(tmp_path / "py.gt", off, ids)
    assert (tmp_path / "cli.gt").read_bytes() == (tmp_path / "py.gt").read_bytes()
    o2, i2 = io.read_range_gt(tmp_path / "cli.gt")
    np.testing.assert_array_equal(o2, off); np.testing.assert_array_equal(i2, ids)
