"""The HCNNG build restated in plain Python (DESIGN.md "Build determinism"; oracle/pann_oracle.cpp, "HCNNG"; the `:NNN`
comments are lines of the reference's HCNNG/clusterEdge.h and HCNNG/hcnng_index.h).

tree() is the random two-pivot cluster tree of ONE tree of a forest: it returns the leaves in position order -- the device keeps
every cluster at its place in one ids array and emits leaves first-side-first, which is the same order -- and counts WHY every
halving happened, which neither the oracle nor the device report.  build() is the whole graph: per leaf the 10 nearest members
(oracle.leaf_knn: the distances and the (dist, id) tie rule stay the oracle's), the edge keys, the degree-bounded Kruskal with
the reference's DisjointSet, process_edges.  tests/test_hcnng_cases_cpu.py shows that build() equals oracle.hcnng_build on
every case of tests/hcnng_cases.py.  Plain Python and numpy: nothing here needs a GPU.

Split distances are integer arithmetic in int64: the data of every case is integer valued, so they are the exact values the
oracle's int32 / float32 sums hold.
"""
import numpy as np

M = 10                         # neighbours per leaf member (hcnng_index.h:140)
SENTINEL = 0xFFFFFFFF
_U64 = (1 << 64) - 1


def mix(x):
    """one splitmix64 step"""
    x = (x + 0x9e3779b97f4a7c15) & _U64
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & _U64
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & _U64
    return x ^ (x >> 31)


def ith_rand(r, i):
    return mix((r + i) & _U64)


def fork(r, i):
    return mix((mix(r) + i + 17) & _U64)


def tree_seed(seed, t):
    return mix(mix((seed + t) & _U64))


def split_distances(Xi, ids, p, metric):
    """distance of every row in ids to row p, int64; Xi: the rows as int64"""
    if metric == "mips":
        return -(Xi[ids] @ Xi[p])
    diff = Xi[ids] - Xi[p]
    return (diff * diff).sum(1)


def tree(X, cluster_size, seed, t, metric="l2", first_empty_guard=True):
    """-> (leaves, why): the leaves of tree t of the forest seeded by `seed` as uint32 id arrays in position order, and
    why = {"same": ..., "first_empty": ..., "second_empty": ..., "splits": ...}: the halvings by cause (bit-identical pivots;
    nothing on the first side; nothing on the second) and the number of all splits, halved or not.
    first_empty_guard = False is the WRONG tree of a builder without the empty-first-side guard: the cluster goes on whole as
    its own second side, under the second side's seed (tests/test_hcnng_cases_cpu.py: which cases would see that)."""
    Xi = np.asarray(X).astype(np.int64)
    assert (Xi == np.asarray(X)).all(), "integer-valued rows only"
    raw = np.ascontiguousarray(X)
    leaves, why = [], dict(same=0, first_empty=0, second_empty=0, splits=0)
    stack = [(np.arange(len(X), dtype=np.uint32), tree_seed(seed, t))]
    while stack:
        act, r = stack.pop()
        if len(act) <= cluster_size:                                   # :103-104
            leaves.append(act)
            continue
        why["splits"] += 1
        fi = ith_rand(r, 0) % len(act)                                 # select_two_random :40-50
        su = ith_rand(r, 1) % (len(act) - 1)
        si = su if su < fi else su + 1
        f, s = int(act[fi]), int(act[si])
        cause = None
        if raw[f].tobytes() == raw[s].tobytes():                       # Points[f] == Points[s] :107
            cause = "same"
        else:
            first = split_distances(Xi, act, f, metric) <= split_distances(Xi, act, s, metric)     # :71-83
            a, b = act[first], act[~first]                             # parlay::filter keeps the order: a stable partition
            if len(a) == 0 and first_empty_guard:
                cause = "first_empty"
            elif len(b) == 0:
                cause = "second_empty"
        if cause is not None:                                          # :108-115
            why[cause] += 1
            a, b = act[:len(act) // 2], act[len(act) // 2:]
        stack.append((b, fork(r, 1)))                                  # :86; popped after the whole first side
        if len(a):
            stack.append((a, fork(r, 0)))                              # :85
    return leaves, why


class DisjointSet:
    """hcnng_index.h:36-89.  unite compares rank[x] and rank[y], the ranks of the ARGUMENTS, not of their roots (:53-54);
    rank_of = "root" is the textbook rule (see leaf_mst)."""

    def __init__(self, n, rank_of="x"):
        self.parent, self.rank, self.rank_of = list(range(n)), [0] * n, rank_of

    def find(self, x):
        p = self.parent
        r = x
        while p[r] != r:
            r = p[r]
        while p[x] != r:
            p[x], x = r, p[x]
        return r

    def unite(self, x, y):
        xr, yr = self.find(x), self.find(y)
        xk, yk = (self.rank[x], self.rank[y]) if self.rank_of == "x" else (self.rank[xr], self.rank[yr])
        if xr == yr:
            return
        if xk < yk:
            self.parent[xr] = yr
        else:
            self.parent[yr] = xr
            if xk == yk:
                self.rank[xr] += 1

    def full(self):
        r = self.find(0)
        return all(self.find(i) == r for i in range(1, len(self.parent)))


def leaf_keys(nn_ids, nn_d, ids, n):
    """the edges of one leaf as (dist, i, j) rows, i < j LOCAL indices, sorted and without duplicates (:160-203): every member's
    kNN row gives one key per live slot, and an edge both ends list appears once"""
    N = len(ids)
    local = np.zeros(n, np.int64)
    local[ids] = np.arange(N)
    live = nn_ids != SENTINEL
    i = np.broadcast_to(np.arange(N)[:, None], nn_ids.shape)[live]
    j = local[nn_ids[live]]
    d = nn_d[live]
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    order = np.lexsort((hi, lo, d))                                    # less_dup :183-201
    d, lo, hi = d[order], lo[order], hi[order]
    keep = np.ones(len(d), bool)
    keep[1:] = (d[1:] != d[:-1]) | (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    return d[keep], lo[keep], hi[keep]


def leaf_mst(lo, hi, N, mst_deg, rank_of="x", stop_every_n=True):
    """the degree-bounded Kruskal over the sorted keys of one leaf (:208-226) -> the edges taken, in order, as local (a, b).
    Neither the rank rule nor the stop test can show in the edges taken: the rank rule picks which ROOT survives a union, never
    which members a set holds, and once every member is in one set no later edge passes the find test -- the stop only ends
    early a walk that would take nothing more.  They are restated because the device restates them, and
    tests/test_hcnng_cases_cpu.py asserts that switching them off changes nothing."""
    ds, deg, out = DisjointSet(N, rank_of), [0] * N, []
    for e, (a, b) in enumerate(zip(lo.tolist(), hi.tolist())):
        if ds.find(a) != ds.find(b) and deg[a] < mst_deg and deg[b] < mst_deg:
            out.append((a, b))
            deg[a] += 1
            deg[b] += 1
            ds.unite(a, b)
        if stop_every_n and e % N == 0 and ds.full():                  # :221-225
            break
    return out


def build(X, T, cluster_size, mst_deg, seed, metric, oracle, graph=None, rank_of="x", stop_every_n=True, leaves_out=None):
    """-> the graph of T trees in the reference layout (n x (max_deg + 1) uint32, slot 0 = degree).  graph=None starts from
    empty rows of T * mst_deg slots; a graph given is copied and appended to: a row takes an edge only while it has room
    (process_edges :117-131).  rank_of / stop_every_n switch to other rules (DisjointSet; no stop test) for the self-check of
    tests/test_hcnng_cases_cpu.py.  leaves_out: a list that receives (leaves, why) of every tree."""
    X = np.ascontiguousarray(X)
    n = len(X)
    G = np.zeros((n, T * mst_deg + 1), np.uint32) if graph is None else np.array(graph, np.uint32, copy=True)
    max_deg = G.shape[1] - 1
    for t in range(T):
        leaves, why = tree(X, cluster_size, seed, t, metric)
        if leaves_out is not None:
            leaves_out.append((leaves, why))
        for ids in leaves:
            N = len(ids)
            if N < 2:
                continue
            nn_ids, nn_d = oracle.leaf_knn(X, ids, M, metric)
            _, lo, hi = leaf_keys(nn_ids, nn_d, ids, n)
            for a, b in leaf_mst(lo, hi, N, mst_deg, rank_of, stop_every_n):
                for u, v in ((ids[a], ids[b]), (ids[b], ids[a])):      # MST_edges holds (a, b) then (b, a)
                    if G[u, 0] < max_deg:
                        G[u, 1 + G[u, 0]] = v
                        G[u, 0] += 1
    return G
