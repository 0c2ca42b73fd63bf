"""Cases shared by the subset-index tests (DESIGN.md "Subset index"): tests/test_subset_cases_cpu.py asserts on numpy alone that
the tables reach the regimes they are there for, tests/test_subset_gpu.py runs them on the device against tests/subset_ref.py.
Plain Python: nothing here needs a GPU.

Sizes: the smallest at which each piece of the bitmap compaction can go wrong.
    n = 20 011   626 bitmap words: three compaction blocks of 256 words, the last one partial, and a last word of 11 live bits
    n =  8 192   exactly one block and no partial word
    n =     37

Masks per n (packed bitmaps; name -> uint32 words):
    all, none, only_first, only_last (bit n - 1), 50pct, 1pct (at least one bit: the smallest n would draw none)
    block_edges  bits 8 191 and 8 192 only: the last position of one compaction block and the first of the next (n = 20 011)
    dead_bits    50pct with every bit >= n of the last word set (where n has a partial word): must give what 50pct gives

Layouts (points, metric, d, max_deg):
    u8       uint8   l2    24   8     baseline: 64-byte device rows, one 16-word graph row
    f32      float32 l2    17  16     an odd dimension
    f16      float16 l2   128  64     one full 256-byte graph row, the widest single-pass shape
    i8       int8    mips 200  32     several 16-byte chunks per lane
    u4       PANN_U4 l2    25  32     13-byte packed rows, the high nibble of the last byte zero
    u8_w65   uint8   l2    24  65     gstride 80: the multi-pass shape, 16 live lanes in the second pass
    u8_w200  uint8   l2    24 200     gstride 208: four passes

Graphs: the degree of every row is drawn from {0, 1, 63, 64, 65, max_deg - 1, max_deg} clipped to max_deg, the neighbours are
random, distinct and never the row's own id.  Rows wider than a wavefront get planted rows on top (kept by 50pct, full degree):
    late_loss   the first 64 neighbours are all kept by 50pct and every later one is dropped: the first pass of the renumbering
                kernel writes 64 slots, the later ones none
    late_keep   the first 64 neighbours are all dropped and every later one is kept: the running base is still 0 when the
                second pass writes
"""
import numpy as np

from parlayann_amd import datasets
from parlayann_amd.index import pack_allow

N_BIG, N_BLOCK, N_SMALL = 20011, 8192, 37
WAVE = 64
N_PLANTED = 4                                # rows of each planted kind

# name -> (dtype or "u4", metric, d, max_deg)
LAYOUTS = {
    "u8": (np.uint8, "l2", 24, 8),
    "f32": (np.float32, "l2", 17, 16),
    "f16": (np.float16, "l2", 128, 64),
    "i8": (np.int8, "mips", 200, 32),
    "u4": ("u4", "l2", 25, 32),
    "u8_w65": (np.uint8, "l2", 24, 65),
    "u8_w200": (np.uint8, "l2", 24, 200),
}
WIDE = tuple(k for k, v in LAYOUTS.items() if v[3] > WAVE)

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def bool_masks(n):
    """name -> boolean (n,), made once per n and never changed"""
    def make():
        rng = np.random.default_rng(1000 + n)
        m = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "only_first": np.arange(n) == 0, "only_last": np.arange(n) == n - 1,
             "50pct": rng.random(n) < 0.5}
        one = rng.random(n) < 0.01
        one[rng.integers(n)] = True
        m["1pct"] = one
        if n > 8192:
            m["block_edges"] = (np.arange(n) == 8191) | (np.arange(n) == 8192)
        return m
    return _once(("bool", n), make)


def masks(n):
    """name -> packed uint32 (ceil(n / 32),)"""
    def make():
        out = {k: pack_allow(v, n) for k, v in bool_masks(n).items()}
        if n & 31:
            dead = out["50pct"].copy()
            dead[-1] |= np.uint32((0xFFFFFFFF << (n & 31)) & 0xFFFFFFFF)
            out["dead_bits"] = dead
        return out
    return _once(("packed", n), make)


def mask_names(n):
    return tuple(masks(n))


def points(layout, n):
    """the rows of a layout as the array a DeviceIndex takes (u4: packed uint8 rows of ceil(d / 2) bytes)"""
    dtype, _, d, _ = LAYOUTS[layout]

    def make():
        if dtype == "u4":
            rows = np.random.default_rng(77).integers(0, 256, (n, (d + 1) // 2), dtype=np.uint8)
            if d & 1:
                rows[:, -1] &= 0x0F            # d is odd: the last byte holds one coordinate, in its low nibble
            return rows
        if np.dtype(dtype) == np.int8:
            return (datasets.sift_like(n, d, seed=1234, dtype=np.float32) - 128.0).clip(-127, 127).astype(np.int8)
        return datasets.sift_like(n, d, seed=1234, dtype=dtype)
    return _once(("points", dtype if dtype == "u4" else np.dtype(dtype).name, d, n), make)      # the three u8 layouts share rows


def queries(layout, nq=33):
    dtype, _, d, _ = LAYOUTS[layout]
    assert dtype != "u4"
    if np.dtype(dtype) == np.int8:
        return (datasets.sift_like(nq, d, seed=4321, dtype=np.float32) - 128.0).clip(-127, 127).astype(np.int8)
    return datasets.sift_like(nq, d, seed=4321, dtype=dtype)


def points_bytes(x):
    """any points array as the byte matrix of tests/subset_ref.py"""
    x = np.ascontiguousarray(x)
    return x.view(np.uint8).reshape(len(x), -1)


def labels(n):
    """one uint32 per point; the low three bits are what the predicate tests match on"""
    return _once(("labels", n), lambda: np.random.default_rng(5).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))


def degree_choices(max_deg):
    return sorted({min(v, max_deg) for v in (0, 1, WAVE - 1, WAVE, WAVE + 1, max_deg - 1, max_deg)})


def _distinct(rng, n, v, count, pool=None):
    """`count` distinct random ids, none of them v: from all n ids, or from the id array `pool`"""
    if pool is None:
        c = rng.integers(0, n - 1, 2 * count + 8)
        _, first = np.unique(c, return_index=True)
        c = (v + 1 + c[np.sort(first)][:count]) % n
    else:
        pool = pool[pool != v]
        c = pool[rng.permutation(len(pool))[:count]]
    assert len(c) == count
    return c


def planted(layout, n):
    """{"late_loss": ids, "late_keep": ids}: the planted rows of a wide layout (empty arrays for a narrow one or a small n)"""
    max_deg = LAYOUTS[layout][3]
    keep = bool_masks(n)["50pct"]
    if max_deg <= WAVE or keep.sum() < 2 * WAVE or (~keep).sum() < 2 * WAVE:
        return {"late_loss": np.zeros(0, np.int64), "late_keep": np.zeros(0, np.int64)}
    rows = np.flatnonzero(keep)[np.random.default_rng(3).permutation(int(keep.sum()))[:2 * N_PLANTED]]
    return {"late_loss": rows[:N_PLANTED], "late_keep": rows[N_PLANTED:]}


def graph(layout, n):
    """uint32 (n, max_deg + 1) in the reference layout, made once"""
    def make():
        max_deg = LAYOUTS[layout][3]
        rng = np.random.default_rng(100 + max_deg)
        deg = rng.choice(degree_choices(max_deg), size=n)
        deg = np.minimum(deg, n - 1)
        deg[0] = min(max_deg, n - 1)           # vertex 0, the default start of a search, has neighbours
        G = np.zeros((n, max_deg + 1), np.uint32)
        for v in range(n):
            G[v, 0] = deg[v]
            G[v, 1:1 + deg[v]] = _distinct(rng, n, v, int(deg[v]))
        keep = bool_masks(n)["50pct"]
        kept, dropped = np.flatnonzero(keep), np.flatnonzero(~keep)
        for kind, rows in planted(layout, n).items():
            first, later = (kept, dropped) if kind == "late_loss" else (dropped, kept)
            for v in rows:
                G[v, 0] = max_deg
                G[v, 1:1 + WAVE] = _distinct(rng, n, v, WAVE, first)
                G[v, 1 + WAVE:] = _distinct(rng, n, v, max_deg - WAVE, later)
        return G
    return _once(("graph", LAYOUTS[layout][3], n), make)


def case(layout, n):
    """(X, G, labels) of a layout at n points"""
    return points(layout, n), graph(layout, n), labels(n)
