"""Float test data and checkers for the fast (default-mode) float paths: signed, fractional and real-valued data.

Two kinds of data:

* `grid_like`: clustered vectors whose coordinates are m / 8 (m integer, |m| <= 100), optionally times 2**s.  They are
  exact in f32, f16 and bf16 (7 significant bits), and for d <= 256 every square, product, partial sum, row norm and
  |a|^2 + |b|^2 - 2 a.b is a multiple of 2**(2s) / 64 below 2**(2s) * 2**24 / 64: an f32 evaluation in ANY order and ANY
  algebraic form (difference form, norm form, blocked matrix-core accumulation) is exact, so a kernel must agree with the
  sequential oracle bit for bit.  The helper asserts this precondition in float64 on every call.
* `real_sets`: DEEP-, T2I-shaped and "offset" (SIFT-shaped plus a fraction) data, where only a derived error bound holds:
  `tolerances` gives the running-error bound of an f32 sum of d terms in any order, per kernel form.

The checkers (`check_dists`, `check_topk`) compare device results with float64 numpy on the STORED (already rounded) values.
"""
import numpy as np

from parlayann_amd import bfloat16, datasets, from_bf16, to_bf16

U = 2.0 ** -24                       # unit roundoff of f32
SENTINEL = 0xFFFFFFFF
FLOAT_TYPES = [np.float32, np.float16, bfloat16]
GRID_MAX = 100                       # |m| <= 100: 7 significant bits
EXACT_LIMIT = float(1 << 24)         # integers below 2^24 are exact in f32


def type_name(dtype):
    return "bf16" if np.dtype(dtype) == bfloat16 else np.dtype(dtype).name


def cast(x, dtype):
    """float array -> `dtype` (round to nearest even), C-contiguous"""
    with np.errstate(over="ignore"):             # an overflow shows as inf and is refused by the caller's round-trip check
        return to_bf16(x) if np.dtype(dtype) == bfloat16 else np.ascontiguousarray(np.asarray(x).astype(dtype))


def widen(a):
    """stored values of any float element type -> float64 (exact)"""
    a = np.asarray(a)
    return from_bf16(a).astype(np.float64) if a.dtype == bfloat16 else a.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------------------------------------
def ref_matrix(Q, X, metric):
    """float64 distances of every row of Q (nq x d) to every row of X (n x d): sum((q - x)^2) in the difference form (a true
    zero stays zero) or -q.x"""
    Q = widen(Q); X = widen(X)
    if metric == "mips":
        return -(Q @ X.T)
    out = np.empty((len(Q), len(X)), np.float64)
    for i, q in enumerate(Q):
        t = X - q
        out[i] = np.einsum("nd,nd->n", t, t)
    return out


def ref_pairs(A, B, metric):
    A = widen(A); B = widen(B)
    return -np.einsum("nd,nd->n", A, B) if metric == "mips" else np.einsum("nd,nd->n", A - B, A - B)


def tolerances(Q, X, metric, form, ref=None):
    """Derived bound of |device - float64| per (query, point) for one kernel form, u = 2^-24 (running-error bound of an f32 sum
    of d terms in any order, blocked matrix-core accumulation included):
      "diff" (gather kernels, f32 dense VALU), L2 : (d + 3) u ref
      "ip"   (every MIPS kernel)                  : (d + 1) u sum|a_i b_i|
      "norm" (two-byte dense kernels), L2         : (d + 3) u (|a|^2 + |b|^2 + 2 sum|a_i b_i|)"""
    Qw = widen(Q); Xw = widen(X)
    d = Qw.shape[1]
    if metric == "mips":
        return (d + 1) * U * (np.abs(Qw) @ np.abs(Xw).T)
    if form == "diff":
        return (d + 3) * U * (ref_matrix(Q, X, "l2") if ref is None else ref)
    assert form == "norm", form
    S = (Qw * Qw).sum(1)[:, None] + (Xw * Xw).sum(1)[None, :] + 2.0 * (np.abs(Qw) @ np.abs(Xw).T)
    return (d + 3) * U * S


def tolerances_pairs(A, B, metric, form):
    Aw = widen(A); Bw = widen(B)
    d = Aw.shape[1]
    sab = np.einsum("nd,nd->n", np.abs(Aw), np.abs(Bw))
    if metric == "mips":
        return (d + 1) * U * sab
    if form == "diff":
        return (d + 3) * U * ref_pairs(A, B, "l2")
    return (d + 3) * U * ((Aw * Aw).sum(1) + (Bw * Bw).sum(1) + 2.0 * sab)


def dense_form(dtype, metric):
    """the algebraic form of the dense all-pairs kernels (leaf kNN, brute force) in default mode"""
    if metric == "mips":
        return "ip"
    return "diff" if np.dtype(dtype) == np.dtype(np.float32) else "norm"


def gather_form(metric):
    """the gather kernels (search, pair / query distances, rerank, prune): one lane group per candidate"""
    return "ip" if metric == "mips" else "diff"


# ------------------------------------------------------------------------------------------------------------------------
# grid data
# ------------------------------------------------------------------------------------------------------------------------
class GridCase:
    """X (n x d) and Q (nq x d) of one element type, `planted`: name -> row ids, s: the power-of-two exponent applied"""

    def __init__(self, X, Q, planted, s, metric):
        self.X, self.Q, self.planted, self.s, self.metric = X, Q, planted, s, metric


def _grid_m(n, d, seed):
    """integer numerators m of clustered vectors m / 8 centred on 0: the SIFT-shaped mixture without its offset"""
    x = datasets._mixture(n, d, seed, 256, 16, center_scale=22.0, basis_scale=9.0, noise_scale=12.0)
    return np.clip(np.rint(x.astype(np.float64)), -GRID_MAX, GRID_MAX)


def assert_grid_exact(Xm, Qm, s, dtype):
    """the precondition of bit-exactness, in float64, from the numerators (values are m / 8 * 2^s):
    every value has at most 7 significant bits and survives the cast; 64 * 2^(-2s) * (L2 sum, both norms, |dot| and every
    intermediate of the norm form) stays below 2^24 for EVERY pair of rows; nothing leaves the normal range of f32."""
    allm = np.concatenate([Xm, Qm]) if len(Qm) else Xm
    assert np.array_equal(allm, np.rint(allm)) and np.abs(allm).max(initial=0) <= 127
    nrm = (allm * allm).sum(1).max(initial=0.0)           # = 64 * max |row|^2 of the unscaled data
    # L2 sum <= 2 (|a|^2 + |b|^2) <= 4 max|row|^2; |a.b| and sum|a_i b_i| <= max|row|^2; |a|^2 + |b|^2, 2 a.b and their
    # partial combinations <= 4 max|row|^2; every partial sum of non-negative terms is below its total
    assert 4.0 * nrm < EXACT_LIMIT, (nrm, "sums leave 2^24 / 64")
    vals = allm / 8.0 * 2.0 ** s
    assert np.array_equal(widen(cast(vals, dtype)), vals), "not representable in the element type"
    nz = np.abs(vals[vals != 0])
    if len(nz):
        assert nz.min() ** 2 >= 2.0 ** -126 and 4.0 * nrm / 64.0 * 4.0 ** s < 2.0 ** 127, "f32 range"


def grid_like(n, d, seed, dtype, metric, nq=0, s=0):
    """Clustered vectors with coordinates m / 8 * 2^s, |m| <= 100, about half of them negative, most with a fraction.
    Planted (when the table is large enough): an all-zero row, two pairs of identical rows, a row and its negation, rows
    orthogonal to the zero-padded query set, and -- for mixed-sign inner products inside one top-k -- a last coordinate
    that is <= 0 (zeros are -0.0) except in five rows, with queries that look at that coordinate alone."""
    assert d <= 256
    Xm = _grid_m(n, d, seed)
    Qm = _grid_m(nq, d, seed + 7919) if nq else np.zeros((0, d))
    dz = max(1, d // 4)
    planted = {}
    if n >= 64:
        Xm[:, d - 1] = -np.abs(Xm[:, d - 1])                                    # zeros become -0.0
        pos = np.array([n // 8 + 3 * i for i in range(5)])
        Xm[pos, d - 1] = [24, 24, 16, 8, 4]                                      # 3, 3, 2, 1, 0.5
        zero = n // 3
        Xm[zero] = 0.0
        dup = [(n // 5, n // 2), (1, n - 1)]
        for a, b in dup:
            Xm[b] = Xm[a]
        neg = (n // 4, n // 4 + 1)
        Xm[neg[1]] = -Xm[neg[0]]
        orth = np.array([n // 6, n // 6 + 1, n - 2])
        Xm[orth, : d - dz] = 0.0
        Xm[orth[0], d - dz:] = np.where(Xm[orth[0], d - dz:] == 0, 8, Xm[orth[0], d - dz:])
        planted = {"positive_last": pos, "zero": np.array([zero]), "dup": np.array(dup), "neg": np.array(neg), "orth": orth}
    if nq:
        Qm[:, d - dz:] = 0.0                                                    # the zero-padded query set
    if nq >= 8 and n >= 64:
        Qm[0] = 0.0                                                             # every distance is a zero: ids decide
        Qm[1] = Xm[n // 5]                                                      # equal to two base rows
        Qm[2] = -Xm[n // 4]                                                     # equal to the negated row
        Qm[3] = 0.0; Qm[3, d - 1] = 16                                          # inner products > 0, == 0 and < 0 in one top-k
        Qm[4] = 0.0; Qm[4, d - 1] = 1
        Qm[5] = 0.0; Qm[5, d - 1] = -8                                          # long runs of equal positive products
        planted["queries"] = {"zero": 0, "dup": 1, "neg": 2, "mixed": (3, 4), "ties": 5}
    assert_grid_exact(Xm, Qm, s, dtype)
    scale = 2.0 ** s / 8.0
    return GridCase(cast(Xm * scale, dtype), cast(Qm * scale, dtype), planted, s, metric)


def f64_knn(ref, k, exclude=None):
    """k smallest of every row of `ref` by (distance as f32, id); `exclude`: one id per row that is no candidate.  On grid data
    ref is exact, so this IS the expected result (ids, f32 distances, SENTINEL / +inf beyond the candidates)."""
    nq, n = ref.shape
    ids = np.full((nq, k), SENTINEL, np.uint32); dd = np.full((nq, k), np.inf, np.float32)
    for i in range(nq):
        r = ref[i].astype(np.float32) + np.float32(0.0)                        # -0.0 == +0.0: the id decides
        cand = np.arange(n)
        if exclude is not None:
            cand = cand[cand != exclude[i]]
        order = cand[np.lexsort((cand, r[cand]))][:k]
        ids[i, : len(order)] = order; dd[i, : len(order)] = r[order]
    return ids, dd


# ------------------------------------------------------------------------------------------------------------------------
# real-valued data
# ------------------------------------------------------------------------------------------------------------------------
REAL_SETS = {"deep": 96, "t2i": 200, "offset": 128}


def real_set(name, n, nq, dtype, seed=1234):
    """(X, Q) of `dtype` with two duplicated rows planted (true L2 distance 0) and one query equal to a base row"""
    d = REAL_SETS[name]
    if name == "deep":
        X, Q = datasets.deep_like(n, d, seed=seed), datasets.deep_like(nq, d, seed=seed + 1)
    elif name == "t2i":
        X, Q = datasets.t2i_like(n, d, seed=seed), datasets.t2i_like(nq, d, seed=seed + 1)
    else:       # SIFT-shaped integers plus a fraction: a large common mean, the worst case of the norm form
        r = np.random.default_rng(seed)
        X = datasets.sift_like(n, d, seed=seed, dtype=np.float32) + r.uniform(-0.5, 0.5, (n, d)).astype(np.float32)
        Q = datasets.sift_like(nq, d, seed=seed + 1, dtype=np.float32) + r.uniform(-0.5, 0.5, (nq, d)).astype(np.float32)
    X = X.copy(); Q = Q.copy()
    X[n // 2] = X[n // 5]; X[n - 1] = X[1]
    if nq > 1:
        Q[1] = X[n // 5]
    return cast(X, dtype), cast(Q, dtype)


# ------------------------------------------------------------------------------------------------------------------------
# checkers
# ------------------------------------------------------------------------------------------------------------------------
class Stats:
    """largest |err| / tol and largest relative error seen by the checkers (reports, not assertions)"""

    def __init__(self):
        self.err_over_tol = 0.0
        self.rel = 0.0

    def add(self, err, tol, ref):
        err = np.asarray(err, np.float64); tol = np.asarray(tol, np.float64); ref = np.abs(np.asarray(ref, np.float64))
        ok = tol > 0
        if ok.any():
            self.err_over_tol = max(self.err_over_tol, float((err[ok] / tol[ok]).max()))
        nz = ref > 0
        if nz.any():
            self.rel = max(self.rel, float((err[nz] / ref[nz]).max()))

    def __repr__(self):
        return f"max |err|/tol = {self.err_over_tol:.3g}, max rel err = {self.rel:.3g}"


def check_dists(got, ref, tol, l2, stats=None, what=""):
    """plain distances: every value within tol of the float64 reference; L2 values are >= 0"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite distance"
    err = np.abs(got - ref)
    if stats is not None:
        stats.add(err, tol, ref)
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} distances outside the bound, worst {float((err - tol).max()):.3g} at {np.argwhere(bad)[0]}"
    if l2:
        assert (got >= 0).all(), f"{what}: negative L2 distance {float(got.min()):.3g}"


def check_topk(ids, dists, ref, tol, l2, exclude=None, ncand=None, stats=None, what=""):
    """k-nearest-neighbour rows against the float64 reference `ref` (nq x n, +inf where a point is no candidate of the row):
    * ids valid and distinct, exactly min(k, candidates) of them, the rest SENTINEL / +inf
    * distances non-decreasing, equal neighbours ordered by id
    * every returned distance within tol of the reference distance of its id; L2 distances >= 0
    * completeness: with D the row's last returned distance, NO other candidate p has ref(q, p) < D - tol(q, p)"""
    ids = np.asarray(ids); dists = np.asarray(dists)
    nq, n = ref.shape
    k = ids.shape[1]
    assert ids.shape == dists.shape and len(ids) == nq, (what, ids.shape, dists.shape, ref.shape)
    for i in range(nq):
        cand_ok = np.isfinite(ref[i])
        if exclude is not None:
            cand_ok[exclude[i]] = False
        nc = int(cand_ok.sum()) if ncand is None else int(ncand[i])
        kk = min(k, nc)
        row, dd = ids[i, :kk].astype(np.int64), dists[i, :kk].astype(np.float64)
        tag = f"{what} row {i}"
        assert (ids[i, kk:] == SENTINEL).all() and np.isposinf(dists[i, kk:]).all(), f"{tag}: slots beyond the candidates are used"
        assert (row < n).all(), f"{tag}: id out of range"
        assert cand_ok[row].all(), f"{tag}: an id that is no candidate"
        assert len(np.unique(row)) == kk, f"{tag}: duplicated id"
        assert np.isfinite(dd).all(), f"{tag}: non-finite distance"
        if kk > 1:
            dif = np.diff(dd)
            assert (dif >= 0).all(), f"{tag}: distances decrease"
            assert (np.diff(row)[dif == 0] > 0).all(), f"{tag}: equal distances not ordered by id"
        err = np.abs(dd - ref[i, row])
        if stats is not None:
            stats.add(err, tol[i, row], ref[i, row])
        assert (err <= tol[i, row]).all(), f"{tag}: distance outside the bound by {float((err - tol[i, row]).max()):.3g}"
        if l2:
            assert (dd >= 0).all(), f"{tag}: negative L2 distance {float(dd.min()):.3g}"
        if kk:
            rest = cand_ok.copy(); rest[row] = False
            miss = rest & (ref[i] < dd[-1] - tol[i])
            assert not miss.any(), f"{tag}: point {int(np.argmax(miss))} is closer than the last neighbour by more than the bound"
