"""Cases shared by the steered-search tests (DESIGN.md "Steered masked search").  Plain Python: nothing here needs a GPU.

Shapes are the smallest at which each piece can go wrong: n = 3 000 points, 64 queries, k = 10; the oracle's Vamana graph of every
layout's own rows (R = 32; R = 8 for the narrow rows), whose rows are mostly shorter than R; max_deg 80 for rows wider than a
wavefront (tests/wide_cases.py's graph).  Masks are made of TENANTS: point i belongs to tenant t[i], drawn uniformly from T
tenants, and a query may return the points of one tenant -- 1 / T of them.  The same content is a bitmap row, or a label with an
ANY, a MATCH or a RANGE predicate (labels_of), so the labeled entry points run on the very masks the bitmap ones run on.

    layouts   u8 L2 d32 (64-byte rows, query in LDS) | f16 L2 d128 (query in registers) | i8 MIPS d100 (128-byte rows) |
              f32 L2 d96 (three chunks per lane, query in LDS) | bf16 L2 d200 (seven chunks)
"""
import numpy as np

import wide_cases
from parlayann_amd import bfloat16

N, NQ = 3000, 64
WORDS = (N + 31) // 32
# name -> (dtype, d, metric)
LAYOUTS = {"u8": (np.uint8, 32, "l2"), "f16": (np.float16, 128, "l2"), "i8mips": (np.int8, 100, "mips"), "f32": (np.float32, 96, "l2"),
           "bf16": (bfloat16, 200, "l2")}
QUERY_IDS = np.array([(17 + 331 * i) % N for i in range(NQ)], np.uint32)
_data, _graphs, _refs = {}, {}, {}


def layout_data(layout):
    if layout not in _data:
        dtype, d, metric = LAYOUTS[layout]
        _data[layout] = (np.ascontiguousarray(wide_cases.rows_of(N, d, dtype, 1234)), np.ascontiguousarray(wide_cases.rows_of(NQ, d, dtype, 4321)),
                         metric)
    return _data[layout]


def graph(layout, deg):
    """deg 32 / 8: the oracle's Vamana graph of the layout's rows with R = deg; 80: wide_cases' graph of rows up to 80 wide"""
    import oracle_api
    if (layout, deg) not in _graphs:
        X, _, metric = layout_data(layout)
        if deg == 80:
            G = wide_cases.wide_graph(X, 80, 180, metric)
        else:
            G, _ = oracle_api.load().vamana_build(X, deg, 2 * deg, 1.2, num_passes=1, seed=1, metric=metric)
        _graphs[(layout, deg)] = G
    return _graphs[(layout, deg)]


def tenants(T, seed=5):
    """tenant of every point, uniform over T tenants (T == 0: a mask nobody is in -- every point is tenant 1, queries ask for 0)"""
    if T == 0:
        return np.ones(N, np.uint32)
    return np.random.default_rng(seed + T).integers(0, T, N).astype(np.uint32)


def mask(T, per_query, n=N, nq=NQ):
    """boolean (n,): tenant 0's points -- or (nq, n): query q sees tenant q % T"""
    t = tenants(T)[:n]
    if not per_query:
        return t == 0
    return t[None, :] == (np.arange(nq, dtype=np.uint32) % max(T, 1))[:, None]


def labels_of(T, kind, per_query, nq=NQ):
    """(labels uint32 (N,), preds): the mask(T, per_query) as label predicates of `kind`.  ANY needs a bit per tenant: T <= 32."""
    t = tenants(T)
    rng = np.random.default_rng(900 + T)
    want = (np.arange(nq, dtype=np.uint32) % max(T, 1)) if per_query else np.zeros(1, np.uint32)
    if kind == "any":
        assert T <= 32
        lab = np.uint32(1) << t
        preds = np.stack([np.uint32(1) << want, np.zeros_like(want)], 1)
    elif kind == "match":
        lab = t | (rng.integers(0, 1 << 20, N).astype(np.uint32) << np.uint32(12))        # tenant in the low 12 bits, noise above
        preds = np.stack([np.full_like(want, 0xFFF), want], 1)
    else:
        lab = (t << np.uint32(20)) + rng.integers(0, 1 << 20, N).astype(np.uint32)         # tenants above 2 047 would pass 2^31: unsigned compare
        preds = np.stack([want << np.uint32(20), (want << np.uint32(20)) + np.uint32((1 << 20) - 1)], 1)
    preds = np.ascontiguousarray(preds, np.uint32)
    return lab.astype(np.uint32), (preds if per_query else (int(preds[0, 0]), int(preds[0, 1])))


def pack(m, n=N, stray_bits=True):
    """boolean (n,) / (nq, n) -> packed uint32 rows; stray_bits: the dead bits of the last word are SET (they must be ignored)"""
    m = np.asarray(m, bool)
    words = (n + 31) // 32
    full = np.zeros(m.shape[:-1] + (words * 32,), bool)
    full[..., :n] = m
    if stray_bits:
        full[..., n:] = True
    return np.ascontiguousarray(np.packbits(full, axis=-1, bitorder="little")).view("<u4").astype(np.uint32)


# name, layout, graph degree, search keywords, tenants T (allowed share 1 / T; 0: nobody), per-query rows, fill
CASES = [
    ("u8-b64-5pc-fill0", "u8", 32, dict(beam=64), 20, False, 0),
    ("f16-b64-5pc-fill16", "f16", 32, dict(beam=64), 20, True, 16),
    ("i8mips-b32-50pc-fill1", "i8mips", 32, dict(beam=32), 2, False, 1),
    ("f32-b100-5pc-fill0", "f32", 32, dict(beam=100), 20, True, 0),
    ("bf16-b200-half-pc-fill37", "bf16", 32, dict(beam=200), 200, False, 37),            # fill above deg: clamped; table in HBM
    ("f16-b8-50pc-fill0", "f16", 32, dict(beam=8, k=4, out_k=8), 2, True, 0),
    ("u8-b64-limit40-5pc-fill16", "u8", 32, dict(beam=64, limit=40), 20, False, 16),     # limit < 2 beam: the skip rule is off
    ("f16-b64-all-fill16", "f16", 32, dict(beam=64), 1, False, 16),
    ("f16-b64-none-fill0", "f16", 32, dict(beam=64), 0, False, 0),
    ("u8-b32-half-pc-fill0", "u8", 32, dict(beam=32), 200, True, 0),
    ("f16-b64-dl20-5pc-fill10", "f16", 32, dict(beam=64, degree_limit=20), 20, False, 10),
    ("f16-b64-dl20-5pc-fill25", "f16", 32, dict(beam=64, degree_limit=20), 20, False, 25),   # clamped to degree_limit
    ("f32-b64-starts3-5pc-fill0", "f32", 32, dict(beam=64, starts=(0, 7, 1999)), 20, False, 0),
    ("u8-b64-query_ids-5pc-fill0", "u8", 32, dict(beam=64, query_ids=True), 20, True, 0),
    ("i8mips-b100-query_ids-50pc-fill16", "i8mips", 32, dict(beam=100, query_ids=True), 2, False, 16),
    ("f16-deg80-b64-5pc-fill0", "f16", 80, dict(beam=64), 20, False, 0),
    ("u8-deg80-b100-half-pc-fill40", "u8", 80, dict(beam=100), 200, True, 40),
    ("u8-deg8-b32-5pc-fill0", "u8", 8, dict(beam=32), 20, False, 0),
    ("bf16-deg8-b64-50pc-fill4", "bf16", 8, dict(beam=64), 2, True, 4),
    ("f32-b200-5pc-fill0", "f32", 32, dict(beam=200, out_k=64), 20, False, 0),
]
CASE_IDS = [c[0] for c in CASES]


def search_kw(kw):
    kw = dict(kw)
    kw.pop("query_ids", None)
    kw.setdefault("k", 10)
    kw.setdefault("out_k", kw["k"])
    kw.setdefault("cut", 1.35)
    kw.setdefault("visited_cap", 2048)
    return kw


def case_mask(case):
    """the case's mask; with three starts the second one is disallowed (and the others allowed)"""
    name, layout, deg, kw, T, per_query, fill = case
    m = mask(T, per_query).copy()
    st = kw.get("starts")
    if st is not None and len(st) == 3:
        m[..., st[0]] = True; m[..., st[1]] = False; m[..., st[2]] = True
    return m


def reference(case):
    """steered_ref for a case, computed once and never changed"""
    import steered_ref
    name, layout, deg, kw, T, per_query, fill = case
    if name not in _refs:
        X, Q, metric = layout_data(layout)
        q = dict(query_ids=QUERY_IDS) if kw.get("query_ids") else dict(queries=Q)
        _refs[name] = steered_ref.steered_batch_search(X, graph(layout, deg), case_mask(case), fill=fill, metric=metric, **q, **search_kw(kw))
    return _refs[name]
