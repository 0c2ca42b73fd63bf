"""Label predicates on the exact route and the two helpers (DESIGN.md "Label predicates"):
    pann_labels_to_allow_dev     rows equal pack(label_allow(...)), dead bits of the last word written 0, words past a row untouched
    pann_label_count_dev         equals allow_count of those rows
    pann_bruteforce_knn_labeled  one predicate (the shared route: expanded on the device, then the compaction + dense kernels) and
                                 one per query (the label scan), bit-equal to tests/masked_knn_cases.reference -- the CPU oracle's
                                 brute force over the allowed rows -- and to pann_bruteforce_knn_masked on the expanded rows.
Shapes as tests/masked_knn_cases.py: n = 20 011 (three compaction blocks and five tiles of the count kernel, the last partial; two
workgroups of the expansion kernel), n = 5 003 with nq = 65 (three scan steps, the last partial).  The labels carry a RANK field (bits 8..31: the
point's place in a random permutation), so a RANGE window selects an exact number of points: 0, fewer than k, exactly k, half."""
import ctypes as C

import numpy as np
import pytest

import label_cases as lc
import masked_knn_cases as kc
from parlayann_amd import DeviceIndex, PannError, _capi, allow_count
from parlayann_amd.index import label_allow, pack_allow

pytestmark = pytest.mark.gpu


def rank_labels(n, seed=31):
    """bits 8..31: rank in a random permutation (n < 2^24); low byte: random"""
    rng = np.random.default_rng(seed)
    rank = np.empty(n, np.uint32)
    rank[rng.permutation(n)] = np.arange(n, dtype=np.uint32)
    return ((rank << np.uint32(8)) | rng.integers(0, 256, n).astype(np.uint32)).astype(np.uint32)


def window(lo, count):
    """the RANGE predicate that selects the `count` points of ranks lo .. lo + count - 1 (count 0: a > b)"""
    if count == 0:
        return ((lo + 1) << 8, lo << 8)
    return (lo << 8, ((lo + count - 1) << 8) | 0xFF)


def _same(got, want, msg):
    for g, w, f in zip(got, want, ("ids", "dists", "counts")):
        np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg=f"{msg}: {f}")


# ---- the helpers ----

@pytest.mark.parametrize("n", [lc.N, kc.N_SHARED])
def test_labels_to_allow_and_label_count(n):
    import torch
    lib = _capi.load()
    rng = np.random.default_rng(n)
    X = rng.integers(0, 255, (n, 16)).astype(np.uint8)
    ix = DeviceIndex(X, max_degree=4)
    try:
        labels = rank_labels(n)
        labels[n - 3:] = [0xFFFFFFFF, 0x00000001, 0x80000000]                   # the last word: labels at the ends of the range
        ix.set_labels(labels)
        w = (n + 31) // 32
        assert n % 32 != 0
        many = {"any": np.array([[1 << (q % 8) | (q // 8) << 9, 0] for q in range(65)], np.uint32),
                "match": np.array([[0xFF, q] for q in range(65)], np.uint32),
                "range": np.array([window(7 * q, c) for q, c in enumerate([0, 1, 9, 10, 63, 64, 65, n // 2, n - 7 * 8] + [100 + q for q in range(56)])],
                                  np.uint32)}
        for kind, preds in many.items():
            want = label_allow(labels, kind, preds)
            packed = pack_allow(want, n)
            assert packed.shape == (65, w)
            got = ix.labels_to_allow((kind, preds))
            np.testing.assert_array_equal(got, packed, err_msg=kind)             # dead bits clear: pack_allow pads with zeros
            np.testing.assert_array_equal(ix.labels_to_allow((kind, tuple(preds[7].tolist()))), packed[7])
            cnt = ix.label_count((kind, preds))
            np.testing.assert_array_equal(cnt, allow_count(packed, n), err_msg=kind)
            np.testing.assert_array_equal(cnt, want.sum(axis=1))
            assert ix.label_count((kind, tuple(preds[8].tolist()))) == int(want[8].sum())      # one predicate
            if kind == "range":
                assert cnt[0] == 0 and cnt[1] <= 1 and n // 2 - 3 <= cnt[7] <= n // 2      # (three ranks were overwritten above)
        # rows further apart than a row is long, over a buffer of ones: the dead bits are WRITTEN 0, the words behind a row stay
        preds = many["any"][:3]
        stride = w + 2
        t_a = torch.full((3, stride), -1, dtype=torch.int32, device="cuda")
        t_p = torch.from_numpy(preds.view(np.int32)).cuda()
        torch.cuda.synchronize()
        st = torch.cuda.current_stream()
        _capi.check(lib.pann_labels_to_allow_dev(ix.handle, 0, C.c_void_p(t_p.data_ptr()), 3, C.c_void_p(t_a.data_ptr()), stride,
                                                 C.c_void_p(st.cuda_stream or None)))
        st.synchronize()
        a = t_a.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(a[:, :w], pack_allow(label_allow(labels, "any", preds), n))
        assert (a[:, w:] == 0xFFFFFFFF).all() and (a[:, w - 1] >> np.uint32(n & 31) == 0).all()
        # refusals: a stride shorter than a row, an unknown kind, null / misaligned pointers, a handle without labels
        BAD = _capi.PANN_ERR_BAD_ARG
        pp, ap = C.c_void_p(t_p.data_ptr()), C.c_void_p(t_a.data_ptr())
        assert lib.pann_labels_to_allow_dev(ix.handle, 0, pp, 3, ap, w - 1, None) == BAD
        assert lib.pann_labels_to_allow_dev(ix.handle, 3, pp, 3, ap, stride, None) == BAD
        assert lib.pann_labels_to_allow_dev(ix.handle, 0, None, 3, ap, stride, None) == BAD
        assert lib.pann_labels_to_allow_dev(ix.handle, 0, C.c_void_p(t_p.data_ptr() + 4), 1, ap, stride, None) == BAD
        assert lib.pann_label_count_dev(ix.handle, 0, pp, 3, None, None) == BAD
        assert lib.pann_label_count_dev(ix.handle, -1, pp, 3, ap, None) == BAD
        ix.drop_labels()
        assert lib.pann_labels_to_allow_dev(ix.handle, 0, pp, 3, ap, stride, None) == BAD
        assert lib.pann_label_count_dev(ix.handle, 0, pp, 3, ap, None) == BAD
        torch.cuda.synchronize()
        np.testing.assert_array_equal(t_a.cpu().numpy().view(np.uint32), a)      # nothing was written by the refused calls
    finally:
        ix.close()


# ---- one predicate for the batch: the shared route ----

@pytest.mark.parametrize("tname,metric,d", [("f16", "l2", 128), ("u8", "mips", 100)])
def test_shared_predicate_equals_the_oracle(oracle, tname, metric, d):
    n = kc.N_SHARED
    X, Q = kc.data(tname, d, n)
    ix = DeviceIndex(X, max_degree=4, metric=metric)
    try:
        labels = rank_labels(n)
        labels[kc.dup_groups(n).ravel()] |= np.uint32(1)               # ANY bit 0 allows the copied rows: ties meet in a result
        ix.set_labels(labels)
        for k in (10, 128):
            wheres = {"none": ("range", window(5, 0)), "k_minus_1": ("range", window(11, k - 1)), "exactly_k": ("range", window(3, k)),
                      "half": ("any", (1, 0)), "byte": ("match", (0xFF, 0x41)), "any_zero": ("any", (0, 0)), "all": ("match", (0, 0))}
            for name, (kind, preds) in wheres.items():
                allow = label_allow(labels, kind, preds)
                c = int(allow.sum())
                assert c == {"none": 0, "k_minus_1": k - 1, "exactly_k": k, "any_zero": 0, "all": n}.get(name, c)
                if name == "half":
                    assert 0.45 * n < c < 0.55 * n
                if name == "byte":
                    assert 10 < c < 128                                # fewer than k = 128, more than k = 10
                want = kc.reference(oracle, X, Q, allow, k, metric)
                got = ix.bruteforce_knn_labeled(Q, k, (kind, preds))
                _same(got, want, f"k={k} {name}")
                _same(got, ix.bruteforce_knn_masked(Q, k, kc.pack_shared(allow, n)), f"k={k} {name}: bitmap entry")
                assert (got[2] == min(k, c)).all()
    finally:
        ix.close()


# ---- one predicate per query: the label scan ----

@pytest.mark.parametrize("tname,metric,d", [("f16", "l2", 128), ("i8", "mips", 100), ("f32", "l2", 200)])
def test_per_query_predicates_equal_the_oracle(oracle, tname, metric, d):
    n, nq = kc.N_ROWS, kc.NQ
    X, Q = kc.data(tname, d, n)
    ix = DeviceIndex(X, max_degree=4, metric=metric)
    try:
        labels = rank_labels(n)
        for g, ids in enumerate(kc.dup_groups(n)):                     # the copied rows of group g share byte g and bit 7
            labels[ids] = (labels[ids] & np.uint32(0xFFFFFF00)) | np.uint32(0x80 | g)
        ix.set_labels(labels)
        counts = [0, 1, 63, 64, 65, n // 2, n, 2048, 2049, 4096, n - 4096] + [3 * q + 2 for q in range(nq - 11)]
        sets = {
            "range": np.array([window(0 if c > n - 64 else (17 * q) % 64, c) for q, c in enumerate(counts)], np.uint32),
            "match": np.array([[0xFF, (0x80 | q) if q < 4 else q] for q in range(nq)], np.uint32),       # about n / 256 points each
            "any": np.array([[1 << (q % 8) if q else 0, 0] for q in range(nq)], np.uint32),              # about half each; query 0: none
        }
        for kind, preds in sets.items():
            allow = label_allow(labels, kind, preds)
            assert allow.shape == (nq, n)
            c = allow.sum(axis=1)
            if kind == "range":
                np.testing.assert_array_equal(c, counts)                 # 0, fewer than k, exactly k = 64, half, everything
            if kind == "match":
                for g, ids in enumerate(kc.dup_groups(n)):
                    assert allow[g, ids].all()                           # query g equals the rows of group g: the ties lead its list
            ref = kc.reference(oracle, X, Q, allow, 64, metric)
            rows = pack_allow(allow, n)
            for k in (1, 64):
                got = ix.bruteforce_knn_labeled(Q, k, (kind, preds))
                _same(got, kc.head(ref, k), f"{kind} k={k}")
                _same(got, ix.bruteforce_knn_masked(Q, k, rows), f"{kind} k={k}: bitmap entry")
            assert (ref[2] == np.minimum(c, 64)).all()
    finally:
        ix.close()


def test_dev_entry_and_refusals():
    import torch
    lib = _capi.load()
    n, nq, d = kc.N_ROWS, kc.NQ, 128
    X, Q = kc.data("u8", d, n)
    ix = DeviceIndex(X, max_degree=4)
    u4 = DeviceIndex.from_packed(X[:, :64] & 0x77, 128, "u4", max_degree=4)
    try:
        labels = rank_labels(n)
        ix.set_labels(labels); u4.set_labels(labels)
        preds = np.array([window(q, 5 * q) for q in range(nq)], np.uint32)
        host = ix.bruteforce_knn_labeled(Q, 10, ("range", preds))
        t_q, t_p = torch.from_numpy(Q).cuda(), torch.from_numpy(preds.view(np.int32)).cuda()
        t_i = torch.zeros((nq, 10), dtype=torch.int32, device="cuda"); t_d = torch.zeros((nq, 10), dtype=torch.float32, device="cuda")
        t_c = torch.zeros(nq, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        vp = lambda t: C.c_void_p(t.data_ptr())
        for npreds in (nq, 1):                                           # the scan, then the shared route (which synchronises)
            _capi.check(lib.pann_bruteforce_knn_labeled_dev(ix.handle, vp(t_q), nq, d, 10, _capi.PANN_PRED_RANGE, vp(t_p), npreds, vp(t_i),
                                                            vp(t_d), vp(t_c), C.c_void_p(stream.cuda_stream)))
            stream.synchronize()
            want = host if npreds == nq else ix.bruteforce_knn_labeled(Q, 10, ("range", tuple(preds[0].tolist())))
            _same((t_i.cpu().numpy(), t_d.cpu().numpy(), t_c.cpu().numpy()), want, f"dev npreds={npreds}")
        assert (t_c.cpu().numpy() == 0).all()                            # preds[0] is the empty window: every row is padding

        def code(fn):
            with pytest.raises(PannError) as e:
                fn()
            assert str(e.value)
            return e.value.code
        BAD, UNS = _capi.PANN_ERR_BAD_ARG, _capi.PANN_ERR_UNSUPPORTED
        assert code(lambda: ix.bruteforce_knn_labeled(Q, 65, ("range", preds))) == UNS          # k = 65 with per-query predicates
        assert code(lambda: ix.bruteforce_knn_labeled(Q, 129, ("range", (0, 5)))) == UNS        # k = 129 with one
        ids, _, cnt = ix.bruteforce_knn_labeled(Q, 65, ("range", window(0, 70)))                # k = 65 with one is the shared route
        assert (cnt == 65).all() and (ids < n).all()
        assert code(lambda: ix.bruteforce_knn_labeled(Q, 0, ("range", preds))) == BAD
        assert code(lambda: ix.bruteforce_knn_labeled(Q, 10, (5, preds))) == BAD                # unknown kind
        Q4 = np.ascontiguousarray(Q[:, :64] & 0x77)
        assert code(lambda: u4.bruteforce_knn_labeled(Q4, 10, ("range", preds))) == UNS         # a four-bit handle
        assert lib.pann_bruteforce_knn_labeled_dev(ix.handle, vp(t_q), nq, d, 10, 2, vp(t_p), 2, vp(t_i), vp(t_d), vp(t_c), None) == BAD
        assert lib.pann_bruteforce_knn_labeled_dev(ix.handle, vp(t_q), nq, d, 10, 2, C.c_void_p(t_p.data_ptr() + 4), 1, vp(t_i), vp(t_d),
                                                   vp(t_c), None) == BAD
        with pytest.raises(ValueError):
            ix.bruteforce_knn_labeled(Q, 10, ("range", preds[:-1]))                             # predicates != queries
        ix.drop_labels()
        assert code(lambda: ix.bruteforce_knn_labeled(Q, 10, ("range", preds))) == BAD          # no labels
    finally:
        ix.close(); u4.close()
