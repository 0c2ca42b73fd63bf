"""Cases shared by the tests of the filter medoids (DESIGN.md "Entry points"): tests/test_entry_ref_cpu.py asserts from the
reference alone that the tables reach every regime they are there for, tests/test_entry_gpu.py runs them on the device and
compares ids, dists, counts and centroids bit for bit.  Plain Python.

Data, labels and shapes are those of tests/grouped_knn_cases.py (n = 20 011, integer-valued rows with copied rows, labels that
hold a rank so that a RANGE window allows an exact number of points).  Two tables:

    "groups"   grouped_knn_cases.table(E): G = 8; the allowed counts are n // 2 (20 pieces), E - 1 (fewer than per_filter), 0,
               7, E, n (40 pieces, the last bitmap word partly live), the last five ids, and n // 2 again (two equal entries)
    "pieces"   windows of exactly 1, P - 1, P, P + 1 and 3 P + 7 points, P = the list ids one workgroup sums
               ("centroid_piece_ids"); the four copied rows 31, 32, 33, 64 alone -- their centroid IS the row, so all four tie at
               the medoid and the id decides; and an empty window
"""
import numpy as np

import entry_ref
import grouped_knn_cases as gc
import masked_knn_cases as kc
from parlayann_amd.index import label_allow

P = 512                                              # pann_index_get_option("centroid_piece_ids"); the device test asserts it
N = gc.N
PER_FILTER = (1, 10, 128)
PIECES = ("one", "p_minus_1", "p", "p_plus_1", "several", "ties", "empty")
PIECE_COUNTS = {"one": 1, "p_minus_1": P - 1, "p": P, "p_plus_1": P + 1, "several": 3 * P + 7, "ties": 4, "empty": 0}
TIE_IDS = (31, 32, 33, 64)                           # masked_knn_cases.dup_groups(N)[2]: ranks DUP_RANK + 6 .. DUP_RANK + 9
GRID, GRID_IDS = gc.GRID, gc.GRID_IDS


def pieces_table():
    w = {"one": gc.window(9000, 1), "p_minus_1": gc.window(1000, P - 1), "p": gc.window(2000, P), "p_plus_1": gc.window(3000, P + 1),
         "several": gc.window(5000, 3 * P + 7), "ties": gc.window(gc.DUP_RANK + 6, 4), "empty": gc.window(5, 0)}
    return np.array([w[e] for e in PIECES], np.uint32)


def table(which, E):
    """uint32 (G, 2) RANGE predicates"""
    return gc.table(E) if which == "groups" else pieces_table()


def allow_rows(which, E):
    return label_allow(gc.labels(), "range", table(which, E))


def bitmap_rows(which, E):
    """the table as packed bitmap rows with their dead bits set"""
    return np.stack([kc.pack_shared(a, N) for a in allow_rows(which, E)])


_REF = {}


def reference(oracle, tname, metric, d, which, E):
    """entry_ref.filter_medoids for a table (fill_id 0xFFFFFFFF), computed once and shared: read only"""
    key = (tname, metric, d, which, E)
    if key not in _REF:
        X, _ = gc.data(tname, d)
        r = entry_ref.filter_medoids(oracle, X, allow_rows(which, E), E, metric)
        for a in r.values():
            a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def with_fill(ref, fill_id):
    """the reference with another fill id"""
    ids = ref["ids"].copy()
    ids[np.arange(ids.shape[1])[None, :] >= ref["counts"][:, None]] = fill_id
    return dict(ref, ids=ids)
