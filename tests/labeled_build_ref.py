"""One label-aware Vamana batch restated on the CPU (DESIGN.md "Label-aware build"): plain Python / numpy over the oracle's
distance and the walk of tests/beam_ref.py (a mask does not steer the walk); graphs in the reference layout (slot 0 = degree).
Candidates are the visited points plus the row; one that shares no label with the owner is none; a pick removes what it both
alpha-dominates and label-covers.  Rows are written, then every target of a new edge appends its sources or is pruned again."""
import numpy as np

import beam_ref


def starts_of(label, table, width):
    """the table rows of the label's set bits in bit order, no repeats, `width` ids, padded with the first"""
    out = []
    for b in (b for b in range(32) if (int(label) >> b) & 1):
        out += [int(s) for s in table[b] if int(s) not in out]
    out = out[:width]
    return out + [out[0]] * (width - len(out))


def prune(oracle, X, labels, p, cand, alpha, R, metric, filtered=True):
    """filtered robustPrune of owner p over candidate ids; filtered=False: the plain rule (every label test passes)"""
    lab = (lambda c: int(labels[c])) if filtered else (lambda c: 1)
    dist = lambda a, b: float(np.float32(oracle.distance(X[a], X[b], metric)))
    live = sorted({(dist(c, p), int(c)) for c in cand if int(c) != p and lab(c) & lab(p)})
    out = []
    while live and len(out) < R:
        c0 = live.pop(0)[1]
        out.append(c0)
        live = [(d, c) for d, c in live if not (alpha * dist(c0, c) <= d and (lab(c) & lab(p) & ~lab(c0)) == 0)]
    return out


def set_row(G, v, ids):
    G[v] = 0
    G[v, 0], G[v, 1:1 + len(ids)] = len(ids), ids


def insert_batch(oracle, X, G, labels, batch, table, R, L, alpha, metric="l2", filtered=True):
    """-> (the graph after one labeled batch, info: targets whose row was pruned again, the longest candidate list)"""
    G = np.array(G, np.uint32, copy=True)
    row_of = lambda v: [int(a) for a in G[v, 1:1 + G[v, 0]]]
    width = min(max(bin(int(w)).count("1") for w in labels) * np.asarray(table).shape[1], 64, max(L // 2, 1))
    rows, longest = {}, 0
    for p in (int(b) for b in batch):
        res = beam_ref.batch_search(X, G, query_ids=[p], k=0, beam=L, cut=0.0, limit=len(X), starts=starts_of(labels[p], table, width),
                                    metric=metric, out_k=0, visited_cap=len(X))
        cand = [int(v) for v in res["visited_ids"][0, :res["visited_count"][0]]] + row_of(p)
        longest = max(longest, len(set(cand)))
        rows[p] = prune(oracle, X, labels, p, cand, alpha, R, metric, filtered)
    sources = {}
    for p, r in rows.items():                  # (a dict keeps the batch order: the sources of a target in batch order)
        set_row(G, p, r)
        for v in r:
            sources.setdefault(v, []).append(p)
    heavy = [v for v, src in sources.items() if len(src) + G[v, 0] > R]
    for v, src in sources.items():
        old = row_of(v)
        set_row(G, v, prune(oracle, X, labels, v, src + old, alpha, R, metric, filtered) if v in heavy else src + [a for a in old if a not in src])
    return G, dict(heavy=heavy, longest=longest)
