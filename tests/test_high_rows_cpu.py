"""What the tests of rows past the 4 GiB line rest on (tests/high_rows.py, DESIGN.md "Rows past 4 GiB"), proven without a GPU:
the geometries sit exactly on the line, the block straddles it, the data keeps every float sum exact and lets the block stand for
the whole table, the sparse host arrays stay sparse, and the oracle's graph of the block never leaves the block."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import high_rows as hr

LINE = 4294967296
CASES = [(g, dt, m) for g in hr.GEOMS for dt, m in hr.GEOMS[g]["types"]]
CASE_IDS = [f"{g}-{hr.type_name(dt)}-{m}" for g, dt, m in CASES]


def _row_stride(d, itemsize):
    """choose_point_layout restated: a row is lanes x chunks x 16 bytes, which is the row rounded up to 64 bytes"""
    r64 = (d * itemsize + 63) // 64 * 64
    if r64 in (128, 256, 512):
        lpc, nch = r64 // 16, 1
    elif r64 % 256 == 0:
        lpc, nch = 16, r64 // 256
    elif r64 % 128 == 0:
        lpc, nch = 8, r64 // 128
    else:
        lpc, nch = 4, r64 // 64
    return lpc * nch * 16


def _gstride(max_deg):
    return (max_deg + 15) // 16 * 16


@pytest.mark.parametrize("geom,dtype,metric", CASES, ids=CASE_IDS)
def test_the_block_sits_on_the_line(geom, dtype, metric):
    g = hr.GEOMS[geom]
    stride = _row_stride(g["d"], np.dtype(dtype).itemsize)
    assert stride == hr.row_stride(geom, dtype)
    B0, lo = hr.b0(geom), hr.lo(geom)
    assert B0 * stride == LINE                                   # row B0 is the first one at a byte offset >= 2^32
    assert (g["n"] - 1) * stride + stride > LINE and g["n"] < 0x7FFFFFFF
    if geom == "B":
        assert _gstride(g["max_deg"]) == hr.gstride(geom) == 64 and B0 * _gstride(g["max_deg"]) == LINE     # graph ELEMENTS cross too
    else:
        assert g["n"] * _gstride(g["max_deg"]) < LINE
    assert B0 - lo >= 1024 and lo + hr.M - B0 >= 1024 and lo + hr.M <= g["n"] and lo > 0
    ids = hr.block_ids(geom)
    assert ids[0] == lo and ids[-1] == lo + hr.M - 1 and ids[-1] > (1 << 24)       # ids a float mantissa no longer holds
    X = hr.block(geom, dtype, metric)
    a, b = hr.DUPLICATES[0]
    assert {lo + a, lo + b} == {B0 - 1, B0} and X[a].tobytes() == X[b].tobytes()    # a duplicated pair across the line
    for a, b in hr.DUPLICATES:
        assert X[a].tobytes() == X[b].tobytes()


@pytest.mark.parametrize("geom,dtype,metric", CASES, ids=CASE_IDS)
def test_exactness_and_dominance(geom, dtype, metric):
    X, Q = hr.block(geom, dtype, metric), hr.queries(geom, dtype, metric)
    v = hr.as_int(X)
    assert (v >= (1 if metric == "mips" else 128)).all() and (v <= (127 if metric == "mips" else 255)).all()
    np.testing.assert_array_equal(hr.as_int(hr._typed(v, dtype)), v)                # the element type holds every value exactly
    t = hr.exactness_terms(Q, X, metric)
    assert max(t.values()) < (1 << 24), t
    D = hr.dist_matrix(Q, X, metric)
    zero = hr.zero_row_dist(Q, metric)
    if metric == "mips":
        assert (D < 0).all() and (zero == 0).all()
    else:
        assert (D.max(1) < zero).all()
    for qt in hr.RADIUS_QUANTILES:
        assert hr.radius(geom, dtype, metric, qt) < zero.min()
    # builder mode: block points as queries see the same order of things
    Db = hr.dist_matrix(X[::64], X, metric)
    assert (Db.max(1) < hr.zero_row_dist(X[::64], metric)).all() if metric == "l2" else (Db < 0).all()


_CHILD = r"""
import json, resource, sys
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np
import high_rows as hr, oracle_api
o = oracle_api.load()
out = {}
for geom in ("A", "B"):
    dt, metric = hr.GEOMS[geom]["types"][0]
    X = hr.sparse_points(geom, dt, metric)
    G, start = hr.block_graph(o, geom, dt, metric)
    lo, n = hr.lo(geom), hr.GEOMS[geom]["n"]
    rows = G[lo:lo + hr.M]
    live = np.arange(G.shape[1] - 1)[None, :] < rows[:, :1]
    nb = rows[:, 1:][live]
    b0 = hr.b0(geom)
    src = np.repeat(np.arange(lo, lo + hr.M), rows[:, 0])
    out[geom] = dict(virtual=int(X.nbytes + G.nbytes), inside=bool(((nb >= lo) & (nb < lo + hr.M)).all()),
                     min_deg=int(rows[:, 0].min()), mean_deg=float(rows[:, 0].mean()),
                     cross_up=int(((src < b0) & (nb >= b0)).sum()), cross_down=int(((src >= b0) & (nb < b0)).sum()),
                     start_in_block=bool(lo <= start < lo + hr.M),
                     # rows outside the block: sampled columns of the degree slot would touch every page -- the oracle writes
                     # only rows it was given, so check the two neighbours of the block and both ends of the table
                     outside=int(G[[0, 1, lo - 1, lo + hr.M, n - 1], 0].sum()) if lo + hr.M < n else int(G[[0, 1, lo - 1, n - 1], 0].sum()))
out["maxrss_kb"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
# after the measurement: EVERY row outside the block, on C, whose graph (2.2 GB) is the cheapest to read in full
dt, metric = hr.GEOMS["C"]["types"][0]
G, _ = hr.block_graph(o, "C", dt, metric)
lo, deg = hr.lo("C"), G[:, 0]
rows = hr.block_rows(G, "C")
out["C"] = dict(outside=int(deg[:lo].any()) + int(deg[lo + hr.M:].any()), min_deg=int(deg[lo:lo + hr.M].min()),
                local_max=int(rows[:, 1:].max()), shape=list(rows.shape))
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def child_report(oracle):
    """A's and B's sparse host arrays and oracle graphs, built in a process of their own: ru_maxrss is a high-water mark of the
    whole process, so only a fresh one measures these arrays and not whatever the suite ran before"""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = _CHILD % dict(root=os.path.dirname(tests), tests=tests)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    if p.returncode != 0 and ("MemoryError" in p.stderr or "refused" in p.stderr):
        pytest.fail("the host refused a lazily zeroed array of the full shape (B's graph is a 17.4 GB virtual allocation): "
                    + p.stderr.strip().splitlines()[-1])
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_sparse_arrays_stay_sparse(child_report):
    assert child_report["A"]["virtual"] > 8 << 30 and child_report["B"]["virtual"] > 20 << 30
    assert child_report["maxrss_kb"] < 3 << 20, f"peak RSS {child_report['maxrss_kb'] >> 10} MiB: the references touched the whole table"


@pytest.mark.parametrize("geom", ["A", "B"])
def test_oracle_graph_lives_in_the_block(child_report, geom):
    r = child_report[geom]
    assert r["inside"] and r["start_in_block"] and r["outside"] == 0
    assert r["min_deg"] >= 1 and r["mean_deg"] > 8                # a real graph, not a chain
    assert r["cross_up"] > 100 and r["cross_down"] > 100          # edges run across B0 in both directions


def test_outside_rows_of_a_block_graph_are_empty(child_report):
    """every row outside the block has degree 0, read in full on C"""
    r = child_report["C"]
    assert r["outside"] == 0 and r["min_deg"] >= 1
    assert r["shape"] == [hr.M, hr.GEOMS["C"]["max_deg"] + 1] and r["local_max"] < hr.M


def test_block_allow_and_references():
    n = hr.GEOMS["B"]["n"]
    ids = hr.block_ids("B")[::3]
    w = hr.block_allow(n, ids)
    assert w.shape == ((n + 31) // 32,) and w.dtype == np.uint32
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")
    np.testing.assert_array_equal(np.flatnonzero(bits), ids)
    # the references against the plainest statement, on a corner of the block
    dt, metric = hr.GEOMS["B"]["types"][1]
    X, Q = hr.block("B", dt, metric)[:300], hr.queries("B", dt, metric, 5)
    D = np.array([[-(int(np.dot(q.astype(np.int64), x.astype(np.int64)))) for x in X] for q in Q])
    np.testing.assert_array_equal(hr.dist_matrix(Q, X, metric), D)
    ids_k, d_k, cnt = hr.knn_ref(Q, X, 1000, 7, metric)
    for i in range(5):
        order = sorted(range(300), key=lambda j: (D[i, j], j))[:7]
        np.testing.assert_array_equal(ids_k[i], np.array(order) + 1000)
        np.testing.assert_array_equal(d_k[i], D[i, order].astype(np.float32))
    off, rid = hr.range_ref(Q, X, 1000, float(np.median(D)), metric)
    for i in range(5):
        np.testing.assert_array_equal(rid[int(off[i]):int(off[i + 1])], np.flatnonzero(D[i] <= np.median(D)) + 1000)
