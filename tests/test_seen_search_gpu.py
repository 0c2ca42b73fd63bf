"""The beam-64 kernel with the second-sighting table V ("Second sightings"): rows of neighbours that the query
compared before are not fetched.  Every output must be what the C++ oracle computes, which fetches every row, and what the
same library computes with the table switched off (`set_option("b64_seen", 0)`), bit for bit.

All tables hold integer values small enough that every float sum is exact, so float types compare bit for bit too.  n = 4 096
with 64 neighbours per row makes the 1 024 slots of the filter H forget ids all the time: that is where V is consulted most
(tests/seen_ref.py counts the skipped rows of that very case on the CPU)."""
import numpy as np
import pytest

import filtered_cases as fc
import seen_ref
from parlayann_amd import DeviceIndex, datasets, quantize, to_bf16

pytestmark = pytest.mark.gpu

NQ = 200
FIELDS = ("ids", "frontier_size", "visited_count", "dist_cmps", "degree_sum", "visited_ids", "status")
_tables = {}


def base(name, oracle):
    """name -> (uint8 values X, Q, graph), built once: 'r64' 4 096 x 128 with a Vamana graph of degree 64, 'r32' 12 000 x 128
    with one of degree 32, 'd200' / 'd96' 6 000 rows with a random graph of degree 32, 'island' r32 with the 20 points around
    the start point linked among themselves only"""
    if name not in _tables:
        if name == "island":
            X, Q, G = base("r32", oracle)
            G = G.copy()
            rng = np.random.default_rng(5)
            for i in range(20):
                G[i, 0] = 8
                G[i, 1:9] = rng.choice(20, size=8, replace=False)
            _tables[name] = (X, Q, G)
        else:
            n, d, R, L = {"r64": (4096, 128, 64, 128), "r32": (12000, 128, 32, 64), "d200": (6000, 200, 32, 0),
                          "d96": (6000, 96, 32, 0)}[name]
            X = datasets.sift_like(n, d, seed=101 + d + R, dtype=np.uint8)
            Q = datasets.sift_like(NQ, d, seed=202 + d + R, dtype=np.uint8)
            G = oracle.vamana_build(X, R, L, 1.15, num_passes=1, seed=9)[0] if L else fc.random_graph(n, R, 17)
            _tables[name] = (X, Q, G)
    return _tables[name]


def typed(X, kind):
    """uint8 values -> (rows the oracle reads, metric, what the device's distances are of the oracle's: 256 for four-bit MIPS)"""
    if kind in ("u4", "i4"):
        V = (X >> 4).astype(np.uint8) if kind == "u4" else ((X >> 4).astype(np.int16) - 8).astype(np.int8)
        return V, "l2" if kind == "u4" else "mips", 1.0 if kind == "u4" else 256.0
    if kind == "i8":
        return (X.astype(np.int16) - 128).clip(-127, 127).astype(np.int8), "mips", 1.0
    if kind == "bf16":
        return to_bf16(X.astype(np.float32)), "l2", 1.0
    return X.astype({"u8": np.uint8, "f16": np.float16, "f32": np.float32}[kind]), "l2", 1.0


def device_index(V, kind, G, metric):
    if kind in ("u4", "i4"):
        ix = DeviceIndex.from_packed(quantize.pack_nibbles(V), V.shape[1], kind, max_degree=G.shape[1] - 1)
        ix.set_graph(G)
        return ix, quantize.pack_nibbles
    return DeviceIndex(V, G, metric=metric), (lambda q: q)


EIGHT = tuple(range(0, 8 * 401, 401))
FULL = tuple(range(0, 64 * 61, 61))          # `beam` start points: the frontier is full from the first merge on
CASES = [
    # name, table, type, search arguments, base-point queries?
    ("f16-r64", "r64", "f16", dict(k=10, beam=64), False),
    ("f16-r64-self-8starts", "r64", "f16", dict(k=10, beam=64, starts=EIGHT), True),
    ("f16-r64-build-mode", "r64", "f16", dict(k=0, beam=64, cut=0.0), True),
    ("u8-r64-limit40", "r64", "u8", dict(k=10, beam=64, limit=40), False),
    ("u8-r64-limit200", "r64", "u8", dict(k=10, beam=64, limit=200), False),
    ("f32-r64-deg40", "r64", "f32", dict(k=10, beam=64, degree_limit=40), False),
    ("i8-r32-mips", "r32", "i8", dict(k=10, beam=64), False),
    ("f32-r32-b40-deg20", "r32", "f32", dict(k=10, beam=40, degree_limit=20), False),
    ("bf16-r32-cut1-full", "r32", "bf16", dict(k=1, beam=64, cut=1.0, starts=FULL), False),
    ("bf16-r64-k1", "r64", "bf16", dict(k=1, beam=64), False),
    ("u4-r32", "r32", "u4", dict(k=10, beam=64), False),
    ("i4-r32-self", "r32", "i4", dict(k=10, beam=64), True),
    ("f16-d200", "d200", "f16", dict(k=10, beam=64), False),
    ("f32-d96-b48", "d96", "f32", dict(k=10, beam=48), False),
    ("bf16-d200-self", "d200", "bf16", dict(k=10, beam=64, starts=EIGHT), True),
    ("f16-island", "island", "f16", dict(k=10, beam=64), False),
    ("f16-r32-cut0", "r32", "f16", dict(k=10, beam=64, cut=0.0, starts=EIGHT), False),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_same_as_oracle_and_as_switched_off(oracle, case):
    name, table, kind, kw, self_q = case
    X, Q, G = base(table, oracle)
    V, metric, scale = typed(X, kind)
    Vq = typed(Q, kind)[0]
    kw = dict(dict(cut=1.35), **kw)
    kw.update(out_k=kw["beam"], visited_cap=2048)
    qids = np.arange(0, len(X), len(X) // NQ, dtype=np.uint32)[:NQ]
    o = oracle.batch_search(V, G, metric=metric, **(dict(query_ids=qids) if self_q else dict(queries=Vq)), **kw)
    assert o["rc"] == 0
    ix, qrows = device_index(V, kind, G, metric)
    try:
        assert ix.get_option("b64_seen") == 1                # a handle starts with the table on
        runs = {}
        for v_n in (0, 1):
            ix.set_option("b64_seen", v_n)
            assert ix.get_option("b64_seen") == v_n
            runs[v_n] = ix.batch_search(query_ids=qids, **kw) if self_q else ix.batch_search(qrows(Vq), **kw)
    finally:
        ix.close()
    for v_n, g in runs.items():
        for f in ("ids", "frontier_size", "visited_count", "dist_cmps", "degree_sum"):
            np.testing.assert_array_equal(o[f], g[f], err_msg=f"{f} v_n={v_n}")
        np.testing.assert_array_equal(o["dists"] * np.float32(scale), g["dists"], err_msg=f"dists v_n={v_n}")
        for i in range(NQ):
            nv = o["visited_count"][i]
            np.testing.assert_array_equal(o["visit_order_ids"][i, :nv], g["visited_ids"][i, :nv], err_msg=f"visit order v_n={v_n}")
        assert g["status"][0] == 0
    for f in FIELDS:                                         # bit for bit what the same library gives without the table
        np.testing.assert_array_equal(runs[0][f], runs[1][f], err_msg=f)
    assert np.array_equal(runs[0]["dists"].view(np.uint32), runs[1]["dists"].view(np.uint32))
    nv = runs[0]["visited_count"]
    for i in range(NQ):
        assert np.array_equal(runs[0]["visited_dists"][i, :nv[i]].view(np.uint32), runs[1]["visited_dists"][i, :nv[i]].view(np.uint32))
    if table == "island":
        assert (o["frontier_size"] < kw["beam"]).all()      # the frontier never fills: V is never consulted


def test_heavy_reuse_case_skips_rows_in_the_model(oracle):
    """the rule fires on the first case of this file: the CPU model (tests/seen_ref.py), which equals the oracle there, leaves
    distances out for every query.  The device has no counter for it; the bytes it fetches are measured."""
    X, Q, G = base("r64", oracle)
    V = X.astype(np.float16)
    g = seen_ref.seen_batch_search(V, G, queries=Q[:24].astype(np.float16), k=10, beam=64, v_n=512)
    o = oracle.batch_search(V, G, queries=Q[:24].astype(np.float16), k=10, beam=64)
    for f in ("ids", "dists", "dist_cmps", "visited_count"):
        assert np.array_equal(g[f], o[f]), f
    print(f"per query: {o['dist_cmps'].mean():.0f} comparisons, {g['repeats'].mean():.0f} repeats, {g['skipped'].mean():.0f} rows not fetched")
    assert (g["skipped"] > 0).all()
