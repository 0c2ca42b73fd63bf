"""Cases shared by the masked-search tests: tests/test_masked_ref_cpu.py asserts on the restatement alone that every case meets
the regime it is there for (so that no device test passes vacuously); tests/test_masked_search_gpu.py runs the same cases on the
device and compares every output with tests/masked_ref.py bit for bit.  Plain Python: nothing here needs a GPU.

Shapes are the smallest at which each piece can go wrong:
    n = 3001         not a multiple of 32: the last bitmap word has 25 live bits and 7 that must be ignored
    degree 32 / 96   one pass over an adjacency row / rows wider than a wavefront (gstride 96)
    "vamana"         the oracle's Vamana graph (R = 32) of the u8 rows: neighbour lists overlap, so at beam 8 (1 024 filter
                     slots for 3 001 ids) points are compared again and reach the result
    "line"           points on a line, vertex i linked to i+-1, i+-2: a walk long enough to end at `limit` while merges are
                     being skipped (a random graph's search ends after about `beam` visits)
    layouts          u8 d128 (8 lanes per candidate), f16 d128 (16), f32 d128 (32), f32 d200 (64-byte granules, query in LDS),
                     i8 MIPS d100, bf16 d128, bf16 d200 (rows of several chunks), packed u4 and i4 d128 (integer-valued data:
                     any summation order is exact).  u8 d128, i8 d100 and bf16 d200 take the generic kernel at every beam
    beams            1, 8, 64: register-frontier kernel (on the layouts that have it); 65, 128: generic kernel, hash filter in LDS; 300: generic kernel, hash
                     filter in HBM, persistent grid
    out_k            1, 10, 64
The other graphs are seeded random graphs (not good graphs: they only have to fill the frontier).  NQ queries per case.
"""
import numpy as np

import filtered_cases as fc
import masked_ref
import wide_cases
from parlayann_amd import bfloat16, quantize

N, NQ = 3001, 8
WORDS = (N + 31) // 32

# name -> (kind, d, metric)
LAYOUTS = {
    "u8": ("u8", 128, "l2"), "f16": ("f16", 128, "l2"), "f32": ("f32", 128, "l2"), "f32d200": ("f32", 200, "l2"),
    "i8mips": ("i8", 100, "mips"), "bf16": ("bf16", 128, "l2"), "bf16d200": ("bf16", 200, "l2"), "u4": ("u4", 128, "l2"),
    "i4": ("i4", 128, "mips"), "line": ("line", 8, "l2"),
}
_DT = {"u8": np.uint8, "f16": np.float16, "f32": np.float32, "i8": np.int8, "bf16": bfloat16}
_data, _graphs, _refs = {}, {}, {}


def layout_data(layout):
    """(X, Q, metric, kind): the rows the CHECKER searches -- for the four-bit kinds the unpacked nibble values, one per byte
    (tests/test_quant4_gpu.py: the device computes the same integers; I4 distances are 256 x the checker's)"""
    if layout not in _data:
        kind, d, metric = LAYOUTS[layout]
        if kind == "line":
            X = np.zeros((N, d), np.float32); X[:, 0] = np.arange(N)
            Q = np.zeros((NQ, d), np.float32); Q[:, 0] = [2999.0, 1400.5, 700.0, 333.25, 2100.0, 90.0, 1000.0, 2500.5]
        elif kind in ("u4", "i4"):
            rng = np.random.default_rng(77)
            lo, hi, dt = (0, 16, np.uint8) if kind == "u4" else (-8, 8, np.int8)
            X, Q = rng.integers(lo, hi, (N, d)).astype(dt), rng.integers(lo, hi, (NQ, d)).astype(dt)
        else:
            X, Q = wide_cases.rows_of(N, d, _DT[kind], 1234), wide_cases.rows_of(NQ, d, _DT[kind], 4321)
        _data[layout] = (np.ascontiguousarray(X), np.ascontiguousarray(Q), metric, kind)
    return _data[layout]


def device_rows(layout):
    """(rows, queries, scale) as the device takes them: packed nibbles for the four-bit kinds"""
    X, Q, _, kind = layout_data(layout)
    if kind in ("u4", "i4"):
        return quantize.pack_nibbles(X), quantize.pack_nibbles(Q), 256.0 if kind == "i4" else 1.0
    return X, Q, 1.0


def graph(deg):
    """deg: 32 / 96 -- a seeded random graph of that maximum degree; "vamana" / "line": see the module docstring"""
    if deg not in _graphs:
        if deg == "vamana":
            import oracle_api
            _graphs[deg], _ = oracle_api.load().vamana_build(layout_data("u8")[0], 32, 64, 1.2, num_passes=1, seed=1)
        elif deg == "line":
            G = np.zeros((N, 5), np.uint32)
            for i in range(N):
                nb = [j for j in (i - 2, i - 1, i + 1, i + 2) if 0 <= j < N]
                G[i, 0] = len(nb); G[i, 1:1 + len(nb)] = nb
            _graphs[deg] = G
        else:
            _graphs[deg] = fc.random_graph(N, deg, 500 + deg)
            assert deg <= 64 or (_graphs[deg][:, 0] > 64).all()
    return _graphs[deg]


def knn_exact(layout, kk):
    """ids of each query's kk exact nearest points (f64 on the integer-valued rows)"""
    X, Q, metric, kind = layout_data(layout)
    from parlayann_amd import from_bf16
    Xf = (from_bf16(X) if kind == "bf16" else X).astype(np.float64)
    Qf = (from_bf16(Q) if kind == "bf16" else Q).astype(np.float64)
    D = -(Qf @ Xf.T) if metric == "mips" else ((Qf[:, None, :] - Xf[None, :, :]) ** 2).sum(-1)
    return np.argsort(D, axis=1, kind="stable")[:, :kk]


def mask(kind, layout, starts=(0,), seed=5):
    """boolean allow mask: (N,) for the shared kinds, (NQ, N) for the per-query kinds"""
    rng = np.random.default_rng(seed)
    if kind == "ones":
        return np.ones(N, bool)
    if kind == "zeros":
        return np.zeros(N, bool)
    if kind == "only_start":
        m = np.zeros(N, bool); m[list(starts)] = True
        return m
    if kind == "start_off":
        m = np.ones(N, bool); m[list(starts)] = False
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
        nn = knn_exact(layout, 200)
        for q in range(NQ):
            m[q, nn[q]] = False
        return m
    raise KeyError(kind)


def pack(m, stray_bits=True):
    """boolean (N,) / (nq, N) -> packed uint32 rows; stray_bits: the 7 dead bits of the last word are SET (they must be ignored)"""
    m = np.asarray(m, bool)
    full = np.zeros(m.shape[:-1] + (WORDS * 32,), bool)
    full[..., :N] = m
    if stray_bits:
        full[..., N:] = True
    return np.ascontiguousarray(np.packbits(full, axis=-1, bitorder="little")).view("<u4").astype(np.uint32)


# name, layout, degree, search keywords, mask kind, regime (what the restatement must show, tests/test_masked_ref_cpu.py)
# Which kernel a beam <= 64 case runs depends on the layout: 128-byte rows (u8 d128, i8 d100) and bf16 d200 have no MASKED
# instantiation of the register-frontier kernel and take the generic one (DESIGN.md "Masked search"); f16, f32, f32d200, bf16
# d128, u4, i4 and the line do.  The u8 / i8mips / bf16d200 cases at beams <= 64 are there for that fallback route.
CASES = [
    ("f16-b64-rand50", "f16", 32, dict(beam=64, k=10, out_k=10), "rand50", None),
    ("f16-b1-ones", "f16", 32, dict(beam=1, k=1, out_k=1), "ones", None),
    ("f32-b8-rand50", "f32", 32, dict(beam=8, k=4, out_k=8), "rand50", None),
    ("f16-vamana-b8-rand50", "f16", "vamana", dict(beam=8, k=4, out_k=8), "rand50", "recompared"),
    ("u4-b8-o1-only_start", "u4", 32, dict(beam=8, k=1, out_k=1), "only_start", None),
    ("f16-deg96-b64-rand50", "f16", 96, dict(beam=64, k=10, out_k=10), "rand50", None),
    ("f32d200-deg96-b8-rand50", "f32d200", 96, dict(beam=8, k=4, out_k=8), "rand50", None),
    ("f16-b64-far_only", "f16", 32, dict(beam=64, k=10, out_k=10), "far_only", "beyond_cutoff"),
    ("f16-b64-query_ids", "f16", 32, dict(beam=64, k=10, out_k=10, query_ids=True), "rand50", None),
    ("f16-b64-starts4", "f16", 32, dict(beam=64, k=10, out_k=10, starts=(0, 7, 1999, 3000)), "start_off", None),
    ("f32-b64-limit40", "f32", 32, dict(beam=64, k=10, out_k=10, limit=40), "rand50", "skip_off"),
    ("f16-b64-k0", "f16", 32, dict(beam=64, k=0, out_k=10), "rand50", None),
    ("f16-b64-rows_differ", "f16", 32, dict(beam=64, k=10, out_k=10), "rows_differ", None),
    # the fallback route (generic kernel at beam <= 64) and the remaining layouts and beams
    ("u8-b64-rand50", "u8", 32, dict(beam=64, k=10, out_k=10), "rand50", None),
    ("u8-b1-ones", "u8", 32, dict(beam=1, k=1, out_k=1), "ones", None),
    ("u8-b8-rand50", "u8", 32, dict(beam=8, k=4, out_k=8), "rand50", None),
    ("u8-vamana-b8-rand50", "u8", "vamana", dict(beam=8, k=4, out_k=8), "rand50", "recompared"),
    ("f16-b64-o64-rand5-limit20", "f16", 32, dict(beam=64, k=10, out_k=64, limit=20), "rand5", "short"),
    ("f32-b64-rand50", "f32", 32, dict(beam=64, k=10, out_k=10), "rand50", None),
    ("f32d200-b64-rand50", "f32d200", 32, dict(beam=64, k=10, out_k=10), "rand50", None),
    ("f32-b65-rand50", "f32", 32, dict(beam=65, k=10, out_k=10), "rand50", None),
    ("f32d200-b128-o64-ones", "f32d200", 32, dict(beam=128, k=10, out_k=64), "ones", None),
    ("i8mips-b300-rand50", "i8mips", 32, dict(beam=300, k=10, out_k=10), "rand50", None),
    ("bf16-b64-start_off", "bf16", 32, dict(beam=64, k=10, out_k=10), "start_off", None),
    ("bf16d200-b64-rand50", "bf16d200", 32, dict(beam=64, k=10, out_k=10), "rand50", None),
    ("u4-b64-rand50", "u4", 32, dict(beam=64, k=10, out_k=10), "rand50", None),
    ("i4-b128-rand50", "i4", 32, dict(beam=128, k=10, out_k=10), "rand50", None),
    ("u8-deg96-b64-rand50", "u8", 96, dict(beam=64, k=10, out_k=10), "rand50", None),
    ("f16-deg96-b65-rand5", "f16", 96, dict(beam=65, k=10, out_k=10), "rand5", None),
    ("f32d200-b64-zeros", "f32d200", 32, dict(beam=64, k=10, out_k=10), "zeros", "empty"),
    ("i8mips-b8-o1-only_start", "i8mips", 32, dict(beam=8, k=1, out_k=1), "only_start", None),
    ("u8-b300-o64-rand5", "u8", 32, dict(beam=300, k=10, out_k=64), "rand5", None),
    ("f16-b128-rows_differ", "f16", 32, dict(beam=128, k=10, out_k=10), "rows_differ", None),
    ("u8-b64-rows_differ", "u8", 32, dict(beam=64, k=10, out_k=10), "rows_differ", None),
    # the three diagnostics
    ("u8-b64-far_only", "u8", 32, dict(beam=64, k=10, out_k=10), "far_only", "beyond_cutoff"),
    ("line-b64-limit128-unmerged", "line", "line", dict(beam=64, k=10, out_k=64, limit=128), "ones", "unmerged"),
    ("line-b65-limit130-unmerged", "line", "line", dict(beam=65, k=10, out_k=64, limit=130), "ones", "unmerged"),
    # other modes
    ("u8-b64-query_ids", "u8", 32, dict(beam=64, k=10, out_k=10, query_ids=True), "rand50", None),
    ("f16-b65-query_ids", "f16", 32, dict(beam=65, k=10, out_k=10, query_ids=True), "rand50", None),
    ("u8-b64-starts4", "u8", 32, dict(beam=64, k=10, out_k=10, starts=(0, 7, 1999, 3000)), "start_off", None),
    ("f32-b128-starts4", "f32", 32, dict(beam=128, k=10, out_k=10, starts=(0, 7, 1999, 3000)), "rand50", None),
    ("u8-b64-limit40", "u8", 32, dict(beam=64, k=10, out_k=10, limit=40), "rand50", "skip_off"),
    ("f32-b300-limit100", "f32", 32, dict(beam=300, k=10, out_k=10, limit=100), "rand50", "skip_off"),
    ("u8-b64-k0", "u8", 32, dict(beam=64, k=0, out_k=10), "rand50", None),
    ("f16-b65-k0", "f16", 32, dict(beam=65, k=0, out_k=10), "rand50", None),
]
CASE_IDS = [c[0] for c in CASES]
# the six mask kinds on both kernels (f16, degree 32: beam 64 -> register-frontier kernel, beam 65 -> generic kernel)
KIND_LAYOUT = "f16"
MASK_KINDS = ["ones", "zeros", "only_start", "start_off", "rand50", "rand5"]
KIND_BEAMS = [64, 65]

QUERY_IDS = np.array([(17 + 331 * i) % N for i in range(NQ)], np.uint32)


def search_kw(kw):
    """keyword arguments common to masked_ref and DeviceIndex.batch_search[_masked] (queries / query_ids excluded)"""
    kw = dict(kw)
    kw.pop("query_ids", None)
    kw.setdefault("cut", 1.35)
    kw.setdefault("visited_cap", 2048)
    return kw


def reference(layout, deg, kw, allow, key=None):
    """masked_ref for a case, computed once per key and never changed"""
    if key is not None and key in _refs:
        return _refs[key]
    X, Q, metric, _ = layout_data(layout)
    q = dict(query_ids=QUERY_IDS) if kw.get("query_ids") else dict(queries=Q)
    r = masked_ref.masked_batch_search(X, graph(deg), allow, metric=metric, **q, **search_kw(kw))
    if key is not None:
        _refs[key] = r
    return r


def case_reference(case):
    name, layout, deg, kw, mkind, _ = case
    return reference(layout, deg, kw, mask(mkind, layout, kw.get("starts", (0,))), key=name)


# ---- the dropped-list retry: points on a line, cut = 1.0 keeps the frontier short (tests/test_edge_cases_gpu.py) ----
LINE_N = 1500


def line_case():
    X = np.zeros((LINE_N, 8), np.float32)
    X[:, 0] = np.arange(LINE_N)
    G = np.zeros((LINE_N, 5), np.uint32)
    for i in range(LINE_N):
        nb = [j for j in (i - 2, i - 1, i + 1, i + 2) if 0 <= j < LINE_N]
        G[i, 0] = len(nb); G[i, 1:1 + len(nb)] = nb
    Q = np.zeros((3, 8), np.float32); Q[:, 0] = [1499.0, 1400.5, 700.0]
    allow = np.arange(LINE_N) % 3 != 0
    return X, G, Q, allow
