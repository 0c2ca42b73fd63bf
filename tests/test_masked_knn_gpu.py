"""Exact kNN under an allow bitmap on the device (DESIGN.md "Exact masked kNN") against the CPU oracle: ids, distances and counts
bit for bit, on the case tables of tests/masked_knn_cases.py (tests/test_masked_knn_cpu.py shows that they reach their regimes).
Integer-valued data with copied rows, so every element type is exact and ties on distance are decided by the id; the
real-valued cases compare with pann_query_distances (default mode) and with the oracle (exact-float-order mode)."""
import ctypes as C

import numpy as np
import pytest

import masked_knn_cases as kc
from parlayann_amd import DeviceIndex, _capi, allow_count
from parlayann_amd.index import pack_allow

pytestmark = pytest.mark.gpu
PAD = kc.PAD_ID


def _same(got, want, msg):
    gi, gd, gc = got
    wi, wd, wc = want
    np.testing.assert_array_equal(gi, wi, err_msg=f"{msg}: ids")
    np.testing.assert_array_equal(gd.view(np.uint32), wd.view(np.uint32), err_msg=f"{msg}: dists")
    np.testing.assert_array_equal(gc, wc, err_msg=f"{msg}: counts")


# ---- shared bitmap -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tname,metric,d", kc.GRID, ids=kc.GRID_IDS)
def test_shared_bitmap_equals_the_oracle(oracle, tname, metric, d):
    n = kc.N_SHARED
    X, Q = kc.data(tname, d, n)
    ix = DeviceIndex(X, max_degree=4, metric=metric)
    kmax = max(kc.KS_SHARED)
    fixed = {name: kc.reference(oracle, X, Q, a, kmax, metric) for name, a in kc.shared_masks(n, kmax).items()
             if name not in ("exactly_k", "k_minus_1")}
    for k in kc.KS_SHARED:
        for name, a in kc.shared_masks(n, k).items():
            want = kc.head(fixed[name], k) if name in fixed else kc.reference(oracle, X, Q, a, k, metric)
            _same(ix.bruteforce_knn_masked(Q, k, kc.pack_shared(a, n)), want, f"k={k} mask={name}")
            if name == "all":                    # and what the plain brute force of the same handle returns
                bi, bd = ix.bruteforce_knn(Q, k)
                _same((bi, bd, np.full(kc.NQ, k, np.uint32)), want, f"k={k} bruteforce_knn")
    ix.close()


def test_shared_bitmap_with_three_pieces(oracle):
    n, k = kc.N_SHARED, 100
    X, Q = kc.data("f16", 128, n)
    ix = DeviceIndex(X, max_degree=4, metric="l2")
    ix.set_option("gt_pieces", 3)
    for name in ("50pct", "1pct", "all"):
        a = kc.shared_masks(n, k)[name]
        _same(ix.bruteforce_knn_masked(Q, k, kc.pack_shared(a, n)), kc.reference(oracle, X, Q, a, k, "l2"), name)
    ix.close()


# ---- per-query bitmaps ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tname,metric,d", kc.GRID, ids=kc.GRID_IDS)
def test_per_query_bitmaps_equal_the_oracle(oracle, tname, metric, d):
    n = kc.N_ROWS
    X, Q = kc.data(tname, d, n)
    A, _ = kc.row_masks(n)
    ix = DeviceIndex(X, max_degree=4, metric=metric)
    ref = kc.reference(oracle, X, Q, A, max(kc.KS_ROWS), metric)
    rows = pack_allow(A, n)
    for k in kc.KS_ROWS:
        _same(ix.bruteforce_knn_masked(Q, k, rows), kc.head(ref, k), f"k={k}")
    # a row stride wider than a row, the extra words (and the dead bits of the last word) all ones
    wide = np.full((kc.NQ, rows.shape[1] + 3), 0xFFFFFFFF, np.uint32)
    wide[:, :rows.shape[1]] = rows
    wide[:, rows.shape[1] - 1] |= np.uint32((0xFFFFFFFF << (n & 31)) & 0xFFFFFFFF)
    _same(ix.bruteforce_knn_masked(Q, 10, wide), kc.head(ref, 10), "stride W + 3")
    ix.close()


@pytest.mark.parametrize("tname,metric,d", [("u8", "l2", 128), ("f32", "mips", 200), ("bf16", "l2", 100)])
def test_one_bitmap_as_shared_and_as_rows(tname, metric, d):
    n = kc.N_ROWS
    X, Q = kc.data(tname, d, n)
    ix = DeviceIndex(X, max_degree=4, metric=metric)
    for name in ("1pct", "50pct", "k_minus_1", "none"):
        w = kc.pack_shared(kc.shared_masks(n, 10)[name], n)
        si, sd, sc = ix.bruteforce_knn_masked(Q, 10, w)
        ri, rd, rc = ix.bruteforce_knn_masked(Q, 10, np.tile(w, (kc.NQ, 1)))
        np.testing.assert_array_equal(si, ri, err_msg=name)
        np.testing.assert_array_equal(sd.view(np.uint32), rd.view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(sc, rc, err_msg=name)
    ix.close()


# ---- real-valued data ----------------------------------------------------------------------------------------------------

def _real(n, nq, d, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)).astype(dtype), rng.standard_normal((nq, d)).astype(dtype)


@pytest.mark.parametrize("dtype,metric,d", [(np.float32, "l2", 100), (np.float32, "mips", 200), (np.float16, "l2", 128),
                                            (np.float16, "mips", 100)])
def test_real_valued_rows_score_as_query_distances(dtype, metric, d):
    """default float mode, per-query route: every distance is pann_query_distances' for the same pair, bit for bit, and the
    row is the head of the host sort by (dist, id) of those distances over the row's allowed ids"""
    n, k = kc.N_ROWS, 10
    X, Q = _real(n, kc.NQ, d, dtype, 5)
    A, _ = kc.row_masks(n)
    ix = DeviceIndex(X, max_degree=4, metric=metric)
    gi, gd, gc = ix.bruteforce_knn_masked(Q, k, A)
    for q in range(kc.NQ):
        live = np.flatnonzero(A[q]).astype(np.uint32)
        c = min(k, len(live))
        assert gc[q] == c and (gi[q, c:] == PAD).all() and np.isinf(gd[q, c:]).all()
        if c == 0:
            continue
        dq = ix.query_distances(Q[q:q + 1], live)[0]
        order = np.lexsort((live, dq))[:c]
        np.testing.assert_array_equal(gi[q, :c], live[order], err_msg=f"row {q}")
        np.testing.assert_array_equal(gd[q, :c].view(np.uint32), dq[order].view(np.uint32), err_msg=f"row {q}")
        back = ix.query_distances(Q[q:q + 1], gi[q, :c])[0]
        np.testing.assert_array_equal(gd[q, :c].view(np.uint32), back.view(np.uint32), err_msg=f"row {q}")
    ix.close()


@pytest.mark.parametrize("route", ["shared", "rows"])
def test_real_valued_exact_float_order_equals_the_oracle(oracle, route):
    n, k = kc.N_ROWS, 10
    X, Q = _real(n, kc.NQ, 100, np.float32, 6)
    ix = DeviceIndex(X, max_degree=4, metric="l2", exact_float_order=True)
    if route == "shared":
        a = kc.shared_masks(n, k)["1pct"]
        _same(ix.bruteforce_knn_masked(Q, k, kc.pack_shared(a, n)), kc.reference(oracle, X, Q, a, k, "l2"), route)
    else:
        A, _ = kc.row_masks(n)
        _same(ix.bruteforce_knn_masked(Q, k, A), kc.reference(oracle, X, Q, A, k, "l2"), route)
    ix.close()


# ---- status codes --------------------------------------------------------------------------------------------------------

def test_status_codes_and_untouched_outputs():
    n, d, nq = 1000, 32, 4
    rng = np.random.default_rng(1)
    X = rng.integers(0, 256, (n, d), dtype=np.uint8)
    Q = rng.integers(0, 256, (nq, d), dtype=np.uint8)
    ix = DeviceIndex(X, max_degree=4)
    four = DeviceIndex.from_packed(rng.integers(0, 256, (n, d // 2), dtype=np.uint8), d, "u4", max_degree=4)
    lib = _capi.load()
    W = (n + 31) // 32
    assert W > 1
    shared, rows = np.full(W, 0xFFFFFFFF, np.uint32), np.full((nq, W), 0xFFFFFFFF, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(h, q, nq_, k, allow, stride, want, null_ids=False):
        ids, dists, cnt = np.full((nq, 129), 0x5A5A5A5A, np.uint32), np.full((nq, 129), 7.5, np.float32), np.full(nq, 77, np.uint32)
        rc = lib.pann_bruteforce_knn_masked(h, p(q), nq_, d, k, p(allow), stride, None if null_ids else p(ids), p(dists), p(cnt))
        assert rc == want, (rc, want, lib.pann_last_error())
        assert (ids == 0x5A5A5A5A).all() and (dists == 7.5).all() and (cnt == 77).all()      # nothing was written

    BAD, UNS = _capi.PANN_ERR_BAD_ARG, _capi.PANN_ERR_UNSUPPORTED
    call(ix.handle, Q, nq, 10, None, 0, BAD)                    # NULL bitmap
    call(ix.handle, None, nq, 10, shared, 0, BAD)               # NULL queries
    call(ix.handle, Q, nq, 10, shared, 0, BAD, null_ids=True)   # NULL output
    call(ix.handle, Q, nq, 10, rows, 1, BAD)                    # a stride between 1 and W - 1
    call(ix.handle, Q, nq, 10, rows, W - 1, BAD)
    call(ix.handle, Q, nq, 0, shared, 0, BAD)                   # k == 0
    call(ix.handle, Q, nq, 65, rows, W, UNS)                    # k > 64 with per-query rows
    call(ix.handle, Q, nq, 129, shared, 0, UNS)                 # k > 128 with a shared bitmap
    call(four.handle, Q, nq, 10, shared, 0, UNS)                # a four-bit handle
    call(ix.handle, Q, 0, 10, shared, 0, _capi.PANN_OK)         # nq == 0: nothing to do
    rc = lib.pann_bruteforce_knn_masked(ix.handle, p(Q), nq, d - 1, 10, p(shared), 0, p(np.zeros((nq, 10), np.uint32)),
                                        p(np.zeros((nq, 10), np.float32)), None)
    assert rc == BAD                                            # a query stride shorter than a row
    gi, gd, gc = ix.bruteforce_knn_masked(Q, 64, rows)          # the limits themselves are served
    assert (gc == 64).all() and (gi != PAD).all()
    gi, gd, gc = ix.bruteforce_knn_masked(Q, 128, shared)
    assert (gc == 128).all() and (gi != PAD).all()
    ix.close(); four.close()


# ---- pann_allow_count_dev and the device entry ---------------------------------------------------------------------------

def test_allow_count_dev_and_device_entry(oracle):
    import torch
    lib = _capi.load()
    vp = lambda t: C.c_void_p(t.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    n = kc.N_SHARED
    masks = kc.shared_masks(n, 10)
    for name, a in masks.items():
        w = kc.pack_shared(a, n)
        t_w, t_c = torch.from_numpy(w.view(np.int32)).cuda(), torch.full((1,), -1, dtype=torch.int32, device="cuda")
        _capi.check(lib.pann_allow_count_dev(vp(t_w), n, 1, 0, vp(t_c), C.c_void_p(stream)))
        torch.cuda.synchronize()
        assert int(t_c.cpu()[0]) == allow_count(w, n) == int(a.sum()), name
    n = kc.N_ROWS
    A, _ = kc.row_masks(n)
    rows = pack_allow(A, n)
    wide = np.full((kc.NQ, rows.shape[1] + 3), 0xFFFFFFFF, np.uint32)
    wide[:, :rows.shape[1]] = rows
    wide[:, rows.shape[1] - 1] |= np.uint32((0xFFFFFFFF << (n & 31)) & 0xFFFFFFFF)
    t_w, t_c = torch.from_numpy(wide.view(np.int32)).cuda(), torch.full((kc.NQ,), -1, dtype=torch.int32, device="cuda")
    _capi.check(lib.pann_allow_count_dev(vp(t_w), n, kc.NQ, wide.shape[1], vp(t_c), C.c_void_p(stream)))
    torch.cuda.synchronize()
    assert t_c.cpu().numpy().tolist() == A.sum(axis=1).tolist() == allow_count(wide, n).tolist()
    assert lib.pann_allow_count_dev(vp(t_w), n, kc.NQ, 5, vp(t_c), C.c_void_p(stream)) == _capi.PANN_ERR_BAD_ARG
    assert lib.pann_allow_count_dev(None, n, kc.NQ, 0, vp(t_c), C.c_void_p(stream)) == _capi.PANN_ERR_BAD_ARG
    # the device entry on the same rows (wide stride) and on one shared row, on the caller's stream
    X, Q = kc.data("f16", 128, n)
    ix = DeviceIndex(X, max_degree=4)
    k = 10
    t_q = torch.from_numpy(Q.view(np.uint8).reshape(kc.NQ, -1).copy()).cuda()
    t_i = torch.zeros((kc.NQ, k), dtype=torch.int32, device="cuda")
    t_d = torch.zeros((kc.NQ, k), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for stride, allow, first_row in ((wide.shape[1], A, 0), (0, A[3], 3)):         # row 3 of the table as the shared bitmap
        ix.bruteforce_knn_masked_dev(t_q.data_ptr(), kc.NQ, 256, k, t_w.data_ptr() + first_row * wide.shape[1] * 4, stride,
                                     t_i.data_ptr(), t_d.data_ptr(), t_c.data_ptr(), stream)
        torch.cuda.synchronize()
        got = (t_i.cpu().numpy().view(np.uint32), t_d.cpu().numpy(), t_c.cpu().numpy().view(np.uint32))
        _same(got, kc.reference(oracle, X, Q, allow, k, "l2"), f"device entry, stride {stride}")
    ix.close()


# ---- GraphIndex: exact_below ---------------------------------------------------------------------------------------------

def test_graph_index_exact_below(tmp_path):
    from parlayann_amd.graph_index import UInt8EuclidianIndex
    n, d, nq, k, beam = 3000, 64, 16, 10, 32
    rng = np.random.default_rng(3)
    X = rng.integers(0, 256, (n, d), dtype=np.uint8)
    Q = rng.integers(0, 256, (nq, d), dtype=np.uint8)
    bix = DeviceIndex(X, max_degree=16)
    bix.vamana_build(16, 32, 1.2, num_passes=1, seed=2)
    G = bix.get_graph()
    bix.close()
    with open(tmp_path / "base.bin", "wb") as f:
        np.array([n, d], np.uint32).tofile(f); X.tofile(f)
    with open(tmp_path / "graph.bin", "wb") as f:       # graph.h:147-232: [n][maxDeg][deg[n]][edges]
        np.array([n, G.shape[1] - 1], np.uint32).tofile(f); G[:, 0].tofile(f)
        np.concatenate([G[i, 1:1 + G[i, 0]] for i in range(n)]).astype(np.uint32).tofile(f)
    gi = UInt8EuclidianIndex(str(tmp_path / "base.bin"), str(tmp_path / "graph.bin"))
    assert np.array_equal(gi.graph, G) and np.array_equal(gi.points, X)
    allow = rng.random(n) < 0.02
    c = int(allow.sum())
    walk = gi.index.batch_search_masked(Q, allow=allow, out_k=k, **gi._qp(k, beam, -1))
    exact = gi.index.bruteforce_knn_masked(Q, k, allow)
    assert (walk["ids"] != exact[0]).any()              # the two routes do differ on this mask
    for fn in (lambda **kw: gi.batch_search_masked(Q, k, beam, allow, **kw), lambda **kw: gi.batch_search(Q, k, beam, allow=allow, **kw)):
        for kw, (wi, wd) in (({}, (walk["ids"], walk["dists"])), (dict(exact_below=None), (walk["ids"], walk["dists"])),
                             (dict(exact_below=c - 1), (walk["ids"], walk["dists"])), (dict(exact_below=c), exact[:2]),
                             (dict(exact_below=n), exact[:2])):
            ids, dists = fn(**kw)
            assert np.array_equal(ids, wi) and np.array_equal(dists.view(np.uint32), wd.view(np.uint32)), kw
    # per-query rows on both sides of the threshold: every row is its route's row, in the given order
    rows = np.stack([rng.random(n) < (0.01 if q % 3 else 0.5) for q in range(nq)])
    cnt = rows.sum(axis=1)
    thr = 200
    assert (cnt <= thr).any() and (cnt > thr).any()
    walk = gi.index.batch_search_masked(Q, allow=rows, out_k=k, **gi._qp(k, beam, -1))
    exact = gi.index.bruteforce_knn_masked(Q, k, rows)
    ids, dists = gi.batch_search_masked(Q, k, beam, rows, exact_below=thr)
    for q in range(nq):
        wi, wd = (exact[0][q], exact[1][q]) if cnt[q] <= thr else (walk["ids"][q], walk["dists"][q])
        assert np.array_equal(ids[q], wi) and np.array_equal(dists[q].view(np.uint32), wd.view(np.uint32)), q
    ids0, dists0 = gi.batch_search_masked(Q, k, beam, rows)
    assert np.array_equal(ids0, walk["ids"]) and np.array_equal(dists0, walk["dists"])
