"""Graph reachability restated on the CPU (DESIGN.md "Graph reachability"), and the cases its CPU and GPU tests share.

There is no reference behaviour to pin: these functions ARE the rule, written the plain way on the host graph layout
(n x (max_deg + 1) uint32, slot 0 = degree).  level[v] = the length of a shortest directed path from any start to v, 0xFFFFFFFF
without one; `consider` selects what counts as unreached and never steers the walk; max_rounds = r stops after r expansion
rounds.  Plain numpy: nothing here needs a GPU.
"""
import numpy as np

from parlayann_amd import allow_bitmap
from parlayann_amd.index import pack_allow

NONE = 0xFFFFFFFF
STAT_KEYS = ("reached_count", "unreached_count", "levels", "max_frontier", "truncated")


def neighbours(G, rows):
    """the ids in the rows given, slot order, repeats kept; an id >= n is skipped as on the device"""
    rows = np.asarray(rows, np.int64)
    slots = G[rows, 1:]
    nb = slots[np.arange(slots.shape[1])[None, :] < G[rows, :1]]
    return nb[nb < len(G)]


def unpack(bitmap, n):
    """packed uint32 words -> bool (n,); bits at positions >= n are dropped"""
    w = (n + 31) // 32
    return np.unpackbits(np.ascontiguousarray(bitmap[:w], "<u4").view(np.uint8), bitorder="little")[:n].astype(bool)


def reach_ref(G, starts, consider=None, max_rounds=0):
    """-> dict(level, reached, unreached_ids, reached_count, unreached_count, levels, max_frontier, truncated), the fields of
    DeviceIndex.reachability but `seconds`.  consider: None, bool (n,) or packed words (bits >= n ignored)."""
    n = len(G)
    starts = np.asarray(starts, np.int64).reshape(-1)
    if len(starts) == 0 or (starts >= n).any() or (starts < 0).any():
        raise ValueError("starts must be ids below n, at least one")
    level = np.full(n, NONE, np.uint32)
    frontier = np.unique(starts)
    level[frontier] = 0
    sizes, rounds, truncated = [len(frontier)], 0, False
    while len(frontier):
        if max_rounds and rounds == max_rounds:
            truncated = True
            break
        mark = np.zeros(n, bool)
        mark[neighbours(G, frontier)] = True
        frontier = np.flatnonzero(mark & (level == NONE))
        rounds += 1
        if len(frontier):
            level[frontier] = rounds
            sizes.append(len(frontier))
    got = level != NONE
    cons = np.ones(n, bool) if consider is None else unpack(pack_allow(consider, n), n)
    unreached = np.flatnonzero(~got & cons).astype(np.uint32)
    return dict(level=level, reached=pack_allow(got, n), unreached_ids=unreached, reached_count=int(got.sum()),
                unreached_count=len(unreached), levels=len(sizes), max_frontier=max(sizes), truncated=truncated)


def degrees_ref(G):
    """(out_deg, in_deg): slots holding an id below n; (row, slot) pairs naming a vertex -- repeats and self loops count"""
    n = len(G)
    slots = np.arange(G.shape[1] - 1)[None, :] < G[:, :1]
    live = slots & (G[:, 1:] < n)
    return live.sum(1).astype(np.uint32), np.bincount(G[:, 1:][live], minlength=n).astype(np.uint32)


def reconnect_ref(oracle, X, G, R, L, alpha, start=0, consider=None, max_rounds=3, metric="l2"):
    """DeviceIndex.reconnect on the oracle: rounds of reach_ref + vamana_insert_batch of the unreached ids, ascending, in
    consecutive batches of max(1, n // 50) -> (the new graph, {"unreached": [...], "remaining_ids": ...})"""
    n = len(G)
    G = np.array(G, np.uint32, copy=True)
    cons = None if consider is None else unpack(pack_allow(consider, n), n)
    if not 0 <= start < n or (cons is not None and not cons[start]):
        raise ValueError("start is not a considered vertex")
    b = max(1, n // 50)
    U = reach_ref(G, (start,), cons)["unreached_ids"]
    counts = [len(U)]
    for _ in range(max_rounds):
        if len(U) == 0:
            break
        for i in range(0, len(U), b):
            oracle.vamana_insert_batch(X, G, U[i:i + b], R, L, alpha, start=start, metric=metric)
        U = reach_ref(G, (start,), cons)["unreached_ids"]
        counts.append(len(U))
        if counts[-1] >= counts[-2]:
            break
    return G, {"unreached": counts, "remaining_ids": U}


def same_fields(got, ref):
    """a device answer against reach_ref's, field for field and exactly (arrays a test did not ask for are None on both sides)"""
    for k in STAT_KEYS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in ("level", "reached", "unreached_ids"):
        if got[k] is not None:
            assert got[k].dtype == np.uint32 and got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


# ---- cases -------------------------------------------------------------------------------------------------------

def host_rows(rows, max_deg):
    """lists of neighbour ids -> the host layout"""
    G = np.zeros((len(rows), max_deg + 1), np.uint32)
    for v, r in enumerate(rows):
        G[v, 0] = len(r)
        G[v, 1:1 + len(r)] = r
    return G


def path_graph(n, max_deg=4):
    """0 -> 1 -> ... -> n - 1: n levels of one vertex"""
    G = np.zeros((n, max_deg + 1), np.uint32)
    G[:n - 1, 0] = 1
    G[:n - 1, 1] = np.arange(1, n)
    return G


MP_FAN, MP_PARENTS, MP_TARGETS, MP_LOOSE = 32, 2000, 64, 3


def many_parents_graph():
    """0 -> 32 fan vertices -> 2 000 parents (level 2, every one of them) -> the SAME 64 targets (level 3), and 3 loose
    vertices nothing points at: n = 2 100, max_deg 64.  Every target is discovered by hundreds of waves at once and must enter
    the next queue once: the queues have n words."""
    n = 1 + MP_FAN + MP_PARENTS + MP_TARGETS + MP_LOOSE
    fan = np.arange(1, 1 + MP_FAN)
    parents = np.arange(1 + MP_FAN, 1 + MP_FAN + MP_PARENTS)
    targets = np.arange(parents[-1] + 1, parents[-1] + 1 + MP_TARGETS)
    rows = [[] for _ in range(n)]
    rows[0] = list(fan)
    for i, f in enumerate(fan):
        rows[f] = list(parents[i::MP_FAN])                       # 62 or 63 parents each, every parent once
    for p in parents:
        rows[p] = list(targets)
    return host_rows(rows, 64)


def random_graph(n, max_deg, seed):
    """full rows of random ids (repeats and self loops as they fall)"""
    rng = np.random.default_rng(seed)
    G = np.empty((n, max_deg + 1), np.uint32)
    G[:, 0] = max_deg
    G[:, 1:] = rng.integers(0, n, (n, max_deg))
    return G


def ragged_graph(n, max_deg, seed):
    """random rows of every degree 0 .. max_deg over a third of the ids (so that some stay unreached), with a self loop in every
    seventh row and a repeated neighbour in every fifth"""
    rng = np.random.default_rng(seed)
    G = np.zeros((n, max_deg + 1), np.uint32)
    deg = rng.integers(0, max_deg + 1, n)
    deg[:max_deg + 1] = np.arange(max_deg + 1)                   # every degree occurs, 0 and max_deg included
    deg[0] = max_deg
    for v in range(n):
        row = rng.integers(0, n // 3, deg[v])
        if deg[v] >= 2 and v % 5 == 0:
            row[1] = row[0]
        if deg[v] >= 1 and v % 7 == 0:
            row[-1] = v
        G[v, 0] = deg[v]
        G[v, 1:1 + deg[v]] = row
    return G


# the quality case of DESIGN.md "Graph reachability": clustered points, a small-R build, 30 % deleted
Q_N, Q_D, Q_R, Q_L, Q_ALPHA, Q_BUILD_SEED, Q_FRACTION, Q_SEEDS = 3000, 16, 8, 16, 1.2, 3, 0.3, (1, 2, 3)


def quality_points():
    rng = np.random.default_rng(11)
    c = rng.integers(0, 256, (20, 16))
    return np.clip(c[rng.integers(0, 20, Q_N)] + rng.normal(0, 12, (Q_N, 16)), 0, 255).astype(np.uint8)


def live_bitmap(n, deleted):
    return allow_bitmap(n, deleted_ids=deleted)
