"""Cases shared by the two-level search tests: tests/test_filtered_ref_cpu.py asserts on the CPU that every case is not
vacuous (the sketch really drops neighbours and changes results), tests/test_filtered_search_gpu.py runs the same cases on
the device against the checker (tests/filtered_ref.py).

A case = a float base (the sketch source), the points that are searched (the float rows themselves, or their one-byte
quantisation), a seeded random graph of out-degree <= 32 on n = 4000 (not a good graph: it only has to fill the frontier),
a sketch kind, a beam width, one QueryParams variation and a query form.

The list is a SAMPLE of dtype x kind x beam x QueryParams variation x query form, not the cross product (the Python checker
takes about a second per case): every beam meets three of the eight (dtype, kind) combinations, every combination meets three
beams, and the variations and query forms rotate.  EXTRA_CASES adds the crossings the rotation misses on the two kernel
variants: every sketch kind and Hamming mode at a beam whose hash filter sits in LDS (64) and at one whose filter sits in
HBM (200), with the small-limit variation on the HBM path.
"""
import numpy as np

from parlayann_amd import quantize
from parlayann_amd import sketch as sk

N, NQ, MAXDEG = 4000, 12, 32

# (name, search dtype, metric, sketch kind, hamming_as_written, d, exact_float_order)
COMBOS = [
    ("u8-l2-ebit", "u8", "l2", "euclid_bit", 0, 128, False),
    ("u8-l2-ebit-aw", "u8", "l2", "euclid_bit", 1, 200, False),
    ("i8-mips-mbit", "i8", "mips", "mips_bit", 0, 100, False),
    ("i8-mips-mbit-aw", "i8", "mips", "mips_bit", 1, 200, False),
    ("i8-mips-2bit", "i8", "mips", "mips_2bit", 0, 200, False),
    ("f32int-l2-ebit", "f32int", "l2", "euclid_bit", 0, 100, False),
    ("f32int-mips-2bit", "f32int", "mips", "mips_2bit", 0, 128, False),
    ("f32real-l2-ebit-exact", "f32real", "l2", "euclid_bit", 0, 100, True),
]
BEAMS = [4, 16, 32, 64, 65, 100, 128, 200]
# QueryParams variations: k (capped at beam / 2), cut, limit, degree_limit, starts
QPVARS = [
    ("k0", dict(k=0)),
    ("k10cut", dict(k=10, cut=1.35)),
    ("limit40", dict(k=10, cut=1.35, limit=40)),
    ("deglim20", dict(k=10, cut=1.35, degree_limit=20)),
    ("starts4", dict(k=10, cut=1.35, starts=(0, 7, 1999, 3999))),
]


def _cases():
    out = []
    for bi, beam in enumerate(BEAMS):
        for j in range(3):
            combo = COMBOS[(bi * 3 + j) % len(COMBOS)]
            qname, qp = QPVARS[(bi + 2 * j) % len(QPVARS)]
            form = "ids" if (bi + j) % 3 == 0 else "ext"
            out.append((f"{combo[0]}-b{beam}-{qname}-{form}", combo, beam, qname, form))
    return out


def _extra():
    out = []
    for ci in (0, 1, 2, 3, 4):                       # the five (kind, Hamming mode) combinations on one-byte points
        for beam, qname, form in ((64, "deglim20", "ext"), (200, "limit40", "ids")):
            combo = COMBOS[ci]
            name = f"x-{combo[0]}-b{beam}-{qname}-{form}"
            out.append((name, combo, beam, qname, form))
    return out


EXTRA_CASES = _extra()
CASES = _cases() + EXTRA_CASES
CASE_IDS = [c[0] for c in CASES]


def random_graph(n, maxdeg, seed):
    rng = np.random.default_rng(seed)
    g = np.zeros((n, maxdeg + 1), np.uint32)
    deg = rng.integers(maxdeg - 12, maxdeg + 1, size=n)
    for i in range(n):
        g[i, 0] = deg[i]
        g[i, 1:1 + deg[i]] = rng.choice(n, size=deg[i], replace=False)
    return g


def random_rows(dtype, n, d, seed):
    """seeded rows of the small pin cases in the test_*_ref_cpu.py files: u8 / i8 over their whole range, standard normal f32"""
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    if dtype == np.int8:
        return rng.integers(-127, 128, size=(n, d)).astype(np.int8)
    return rng.standard_normal((n, d)).astype(np.float32)


def float_data(kind, metric, n, d, seed):
    """the float rows the sketch is made from (and, for the f32 cases, the rows that are searched)"""
    rng = np.random.default_rng(seed)
    if kind == "u8":                                   # real-valued, quantised to u8 with a slope != 1
        return (rng.standard_normal((n, d)) * 30 + 120).astype(np.float32)
    if kind == "i8":                                   # normalised rows (graph_index.cpp:94-96)
        return quantize.normalize_rows(rng.standard_normal((n, d)).astype(np.float32))
    if kind == "f32int":                               # integer-valued: every float path is exact
        return np.rint(rng.standard_normal((n, d)) * 20).astype(np.float32)
    return rng.standard_normal((n, d)).astype(np.float32)      # f32real


def build_case(case):
    name, (cname, sdt, metric, kind, aw, d, exact), beam, qname, form = case
    seed = 1000 + CASE_IDS.index(name)
    Xf = float_data(sdt, metric, N, d, seed)
    Qf = float_data(sdt, metric, NQ, d, seed + 5000)
    if sdt == "u8":
        ep = quantize.euclid_u8_params(Xf)
        assert not ep.identity
        X, Q = quantize.euclid_u8_translate(Xf, ep), quantize.euclid_u8_translate(Qf, ep)
    elif sdt == "i8":
        mv = quantize.mips_i8_max_val(Xf, trim=True)
        X, Q = quantize.mips_i8_translate(Xf, mv), quantize.mips_i8_translate(Qf, mv)
    else:
        X, Q = Xf, Qf
    qp = dict(dict(QPVARS)[qname])
    qp["k"] = min(qp["k"], beam // 2)
    qp["beam"] = beam
    qp.setdefault("cut", 1.35)
    params = sk.sketch_params_numpy(Xf, kind, hamming_as_written=bool(aw))
    query_ids = np.array([(17 + 331 * i) % N for i in range(NQ)], np.uint32) if form == "ids" else None
    return dict(name=name, Xf=Xf, Qf=Qf, X=np.ascontiguousarray(X), Q=np.ascontiguousarray(Q), metric=metric, kind=kind,
                params=params, graph=random_graph(N, MAXDEG, seed + 77), qp=qp, query_ids=query_ids, exact=exact,
                queries=None if form == "ids" else np.ascontiguousarray(Q))


def checker_args(c, use_filtering):
    """keyword arguments of filtered_ref.filtered_batch_search for a built case"""
    a = dict(points=c["X"], graph=c["graph"], queries=c["queries"], query_ids=c["query_ids"], metric=c["metric"],
             out_k=c["qp"]["beam"], visited_cap=2000, use_filtering=use_filtering, **c["qp"])
    if use_filtering:
        a["sketches"] = sk.sketch_rows_numpy(c["Xf"], c["params"])
        a["sketch_params"] = c["params"]
        a["sketch_queries"] = None if c["queries"] is None else sk.sketch_rows_numpy(c["Qf"], c["params"])
    return a
