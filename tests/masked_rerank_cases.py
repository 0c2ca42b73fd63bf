"""Cases shared by the tests of the masked fused search (pann_batch_search_masked_rerank*, DESIGN.md "Masked search on the
fused path"): tests/test_masked_rerank_cases_cpu.py asserts on the CPU restatement alone that every regime a device case is
there for really occurs (so that no device test passes vacuously); tests/test_masked_rerank_gpu.py runs the same cases on the
device.  Plain Python: nothing here needs a GPU.

Shapes are the smallest at which each piece can go wrong:
    n = 3001        not a multiple of 32: the last bitmap word has 25 live bits, and the packed masks have the 7 stray bits SET
    real values     datasets.deep_like x 2 (L2) and datasets.t2i_like (MIPS): the quantisers are not casts
    l2_64           u8 rows of 64 bytes: the masked register-frontier (b64) kernel at beam <= 64
    l2_96           u8 rows on a 128-byte stride: no masked b64 instantiation, the masked generic kernel at beam <= 64
    l2_128_u4       four-bit rows of 64 bytes: the b64 route
    mips_200        i8 rows of 200 bytes (256-byte stride: the b64 route), normalize_first
    mips_100_i4     four-bit MIPS rows of 50 bytes (the b64 route), normalize_first
    (beam, k, rf)   pool = min(k * rf, beam, 64) = 16 / 64 / 6 / 64 / 64; beam 100: generic kernel, hash filter in LDS; beam 300: hash
                    filter in HBM
The restatement (L2 u8 datasets): the oracle's euclid_u8_params / euclid_u8_translate, an oracle Vamana graph (R = 32, L = 64)
of the float rows, tests/masked_ref.py on the translated rows with out_k = pool, oracle.distance on the float rows for the
rerank, lexsort((id, dist)), k kept, padding 0xFFFFFFFF / +inf.
"""
import numpy as np

import masked_ref
from parlayann_amd import datasets

N, NQ, R, L = 3001, 8, 32, 64
WORDS = (N + 31) // 32
SENT = 0xFFFFFFFF

# name -> (d, metric, bits)
DATASETS = {"l2_64": (64, "l2", 8), "l2_96": (96, "l2", 8), "l2_128_u4": (128, "l2", 4), "mips_200": (200, "mips", 8),
            "mips_100_i4": (100, "mips", 4)}
RESTATED = ["l2_64", "l2_96"]                     # the datasets the CPU restatement covers (the oracle has the u8 quantiser)
SWEEP = [(16, 10, 100), (64, 10, 100), (64, 2, 3), (100, 10, 100), (300, 10, 100)]
MASK_KINDS = ["ones", "rand50", "rand5", "zeros", "start_off", "rows_differ", "far_only"]
# The 5 % mask: 150 allowed points.  A search at beam 16 compares about 500 points, 25 of them allowed, so no list is shorter than k; with
# the walk stopped after SHORT_LIMIT visits (the Python mirror always passes a visit limit) about 150 are compared, and at these
# seeds the lists of some queries hold fewer than k = 10 entries and those of others at least 10 (CPU test)
RAND5_SEED = {"l2_64": 5, "l2_96": 7}
SHORT_LIMIT = 5

_data, _graphs, _quant, _refs, _knn = {}, {}, {}, {}, {}


def pool(beam, k, rf):
    return min(k * rf, beam, 64)


def data(name):
    """(X, Q) float32: the rows as given (a MIPS index normalises its own copy)"""
    if name not in _data:
        d, metric, _ = DATASETS[name]
        if metric == "mips":
            X, Q = datasets.t2i_like(N, d, seed=11), datasets.t2i_like(NQ, d, seed=12)
        else:
            X = (datasets.deep_like(N, d, seed=11) * 2.0).astype(np.float32)
            Q = (datasets.deep_like(NQ, d, seed=12) * 2.0).astype(np.float32)
        _data[name] = (np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(Q, dtype=np.float32))
    return _data[name]


def graph(name):
    """the oracle's Vamana graph of the float rows (L2 datasets)"""
    if name not in _graphs:
        import oracle_api
        assert DATASETS[name][1] == "l2"
        _graphs[name], _ = oracle_api.load().vamana_build(data(name)[0], R, L, 1.2, num_passes=1, seed=5)
    return _graphs[name]


def quantised(name):
    """(slope, offset, Xq, Qq): the oracle's u8 quantiser and the translated rows"""
    if name not in _quant:
        import oracle_api
        o = oracle_api.load()
        X, Q = data(name)
        slope, offset = o.euclid_u8_params(X)
        _quant[name] = (slope, offset, o.euclid_u8_translate(X, slope, offset), o.euclid_u8_translate(Q, slope, offset))
    return _quant[name]


def knn_exact(name, kk):
    """ids of each query's kk exact nearest points (f64)"""
    if (name, kk) not in _knn:
        X, Q = data(name)
        Xf, Qf = X.astype(np.float64), Q.astype(np.float64)
        if DATASETS[name][1] == "mips":
            Xf = Xf / np.maximum(np.linalg.norm(Xf, axis=1, keepdims=True), 1e-300)
            D = -(Qf @ Xf.T)
        else:
            D = (Qf * Qf).sum(1)[:, None] - 2.0 * (Qf @ Xf.T) + (Xf * Xf).sum(1)[None, :]
        _knn[(name, kk)] = np.argsort(D, axis=1, kind="stable")[:, :kk]
    return _knn[(name, kk)]


def mask(kind, name, seed=None):
    """boolean allow mask: (N,) for the shared kinds, (NQ, N) for the per-query kinds; start point 0 throughout"""
    if seed is None:
        seed = RAND5_SEED.get(name, 5) if kind == "rand5" else 5
    rng = np.random.default_rng(seed)
    if kind == "ones":
        return np.ones(N, bool)
    if kind == "zeros":
        return np.zeros(N, bool)
    if kind == "start_off":
        m = np.ones(N, bool); m[0] = False
        return m
    if kind == "rand50":
        m = rng.random(N) < 0.5
        m[N - 5:] = [True, False, True, True, False]       # ids in the last bitmap word, both verdicts
        return m
    if kind == "rand5":
        m = rng.random(N) < 0.05
        m[N - 2] = True
        return m
    if kind == "rows_differ":                              # per-query rows: another random half for every query
        return rng.random((NQ, N)) < 0.5
    if kind == "far_only":                                 # per-query rows: each query's 200 exact nearest points are disallowed
        m = np.ones((NQ, N), bool)
        nn = knn_exact(name, 200)
        for q in range(NQ):
            m[q, nn[q]] = False
        return m
    raise KeyError(kind)


def pack(m):
    """boolean (N,) / (nq, N) -> packed uint32 rows with the 7 dead bits of the last word SET (they must be ignored)"""
    m = np.asarray(m, bool)
    full = np.ones(m.shape[:-1] + (WORDS * 32,), bool)
    full[..., :N] = m
    return np.ascontiguousarray(np.packbits(full, axis=-1, bitorder="little")).view("<u4").astype(np.uint32)


def rerank_rows(name, cand, counts, k):
    """exact distances of cand[i, :counts[i]] on the float rows (oracle.distance), sorted by (dist, id), k kept, padded"""
    import oracle_api
    o = oracle_api.load()
    X, Q = data(name)
    ids = np.full((len(Q), k), SENT, np.uint32)
    dists = np.full((len(Q), k), np.inf, np.float32)
    for i in range(len(Q)):
        c = np.asarray(cand[i][:int(counts[i])], np.uint32)
        d = np.array([o.distance(Q[i], X[j]) for j in c], np.float32)
        order = np.lexsort((c, d))[:k]
        ids[i, :len(order)] = c[order]; dists[i, :len(order)] = d[order]
    return ids, dists


def restate(name, beam, k, rf, mkind, **qp):
    """The rule on the CPU, computed once per key and never changed: masked_ref's fields for the quantised search (ids / dists:
    the quantised list of `pool` entries) plus "rr_ids" / "rr_dists", the reranked k."""
    key = (name, beam, k, rf, mkind, tuple(sorted(qp.items())))
    if key not in _refs:
        _, _, Xq, Qq = quantised(name)
        r = masked_ref.masked_batch_search(Xq, graph(name), mask(mkind, name), queries=Qq, k=k, beam=beam, cut=1.35,
                                           out_k=pool(beam, k, rf), **qp)
        r["rr_ids"], r["rr_dists"] = rerank_rows(name, r["ids"], r["result_count"], k)
        _refs[key] = r
    return _refs[key]


def plain_rerank(name, beam, k, rf, **qp):
    """the plain fused call restated: the first min(k * rf, frontier size) frontier ids reranked, k kept -> (ids, dists, restatement)"""
    r = restate(name, beam, k, rf, "ones", **qp)
    fr = r["final_frontier"]
    cand = [[e[1] for e in f] for f in fr]
    counts = [min(len(f), k * rf) for f in fr]
    ids, dists = rerank_rows(name, cand, counts, k)
    return ids, dists, r


LINE_N = 1500


def line_case():
    """The dropped-list retry: the line graph and the mask of masked_cases.line_case (vertex i linked to i+-1, i+-2, every third
    point disallowed) under real-valued rows.  The rows of masked_cases.line_case itself run from 0 to 1499 along one axis; their u8
    copy puts six neighbours on every level and the quantised walk ends at its start, so the rows here are a monotone staircase
    through the cube (coordinate j runs over 256 levels while i is in [255 j, 255 (j + 1)]) at a spacing of 0.37: every vertex
    keeps a quantised row of its own, and the quantiser is not a cast.  With cut = 1.0 and k = 1 the frontier stays at one entry
    while the walk visits every other vertex up to the query: it drops far more entries than a small dropped list holds.
    -> (X, G, Q, allow, Xq, Qq), Xq / Qq the oracle's translation (for the CPU check)"""
    import masked_cases
    import oracle_api
    o = oracle_api.load()
    _, G, _, allow = masked_cases.line_case()
    assert len(G) == LINE_N
    i = np.arange(LINE_N)[:, None]
    X = (np.clip(i - 255 * np.arange(8)[None, :], 0, 255) * 0.37).astype(np.float32)
    Q = (X[[1499, 1400, 700]] + np.float32(0.09)).astype(np.float32)
    slope, offset = o.euclid_u8_params(X)
    assert slope != 1.0
    return X, G, Q, allow, o.euclid_u8_translate(X, slope, offset), o.euclid_u8_translate(Q, slope, offset)
