"""CPU checker of the steered masked search (DESIGN.md "Steered masked search"): tests/masked_ref.py's restatement of
filtered_beam_search (beamSearch.h:22-214, use_filtering == false) with ONE change -- how the list `pruned` of a visited vertex is
made (:128-137):

    direct pass   for the first min(size, degree_limit) neighbours a of cur, in row order: seen(a) or a == self -> skipped;
                  allowed -> pruned; otherwise -> bridges
    two-hop pass  for each bridge b in order: stop when len(pruned) >= fill (a bridge's row is taken whole or not at all); for
                  the first min(size(b), degree_limit) neighbours c of b: not allowed -> skipped WITHOUT touching the hash filter;
                  seen(c) or c == self -> skipped; otherwise -> pruned

fill: 1..deg_eff, deg_eff = min(degree_limit, max_deg); 0 means deg_eff, a larger value is clamped.  Everything else -- the
cutoff, the distances, the skip rule, the merge, the cut-prune, the visited list, the result rule -- is masked_ref's, word for word.
Start points are compared whether allowed or not.

Returns the dictionary of masked_ref.masked_batch_search plus per query

    bridge_rows   bridge rows expanded
    hop2_cmps     entries the two-hop pass appended to pruned
    max_pruned    the longest `pruned` of any visit (diagnostic; bound: fill - 1 + deg_eff)
"""
import bisect
import ctypes as C
import math

import numpy as np

import oracle_api
from masked_ref import BIG, F, FilterSlots, _slots, unpack_allow


def effective_fill(fill, degree_limit, maxdeg):
    deg_eff = max(min(int(degree_limit), int(maxdeg)), 0)
    return deg_eff if fill == 0 or fill > deg_eff else int(fill)


def steered_batch_search(points, graph, allow, fill=0, queries=None, query_ids=None, k=10, beam=64, cut=1.35, limit=None,
                         degree_limit=None, starts=(0,), metric="l2", out_k=None, visited_cap=0, on_distance=None):
    o = oracle_api.load()
    points = np.ascontiguousarray(points)
    graph = np.ascontiguousarray(graph, dtype=np.uint32)
    n, d = points.shape
    maxdeg = graph.shape[1] - 1
    nq = len(queries) if queries is not None else len(query_ids)
    out_k = k if out_k is None else out_k
    limit = n if limit is None else limit
    degree_limit = maxdeg if degree_limit is None else degree_limit
    fill = effective_fill(fill, degree_limit, maxdeg)
    starts = [int(s) for s in starts]
    mcode = oracle_api.METRIC[metric.lower() if isinstance(metric, str) else metric]
    dt = oracle_api.DT[points.dtype]
    if queries is not None:
        queries = np.ascontiguousarray(queries)
        assert queries.dtype == points.dtype
    allow = unpack_allow(allow, n, nq)

    bits = max(10, int(math.ceil(math.log2(float(beam) * float(beam)))) - 2)           # :52
    if bits not in _slots:
        _slots[bits] = FilterSlots(o, bits)
    slot_of = _slots[bits]
    pbase, pstride = points.ctypes.data, points.strides[0]
    dist_fn = o.lib.pann_oracle_distance
    c_dt, c_m, c_d = C.c_int(dt), C.c_int(mcode), C.c_uint32(d)

    res = {
        "ids": np.full((nq, out_k), 0xFFFFFFFF, np.uint32), "dists": np.full((nq, out_k), np.inf, np.float32),
        "frontier_ids": np.full((nq, out_k), 0xFFFFFFFF, np.uint32), "frontier_dists": np.full((nq, out_k), np.inf, np.float32),
        "frontier_size": np.zeros(nq, np.uint32), "visited_count": np.zeros(nq, np.uint32),
        "dist_cmps": np.zeros(nq, np.uint32), "degree_sum": np.zeros(nq, np.uint32),
        "visited_ids": np.zeros((nq, visited_cap), np.uint32) if visited_cap else None,
        "visited_dists": np.zeros((nq, visited_cap), np.float32) if visited_cap else None,
        "result_count": np.zeros(nq, np.uint32), "allowed_cmps": np.zeros(nq, np.uint32),
        "from_beyond_cutoff": np.zeros(nq, np.uint32), "from_unmerged": np.zeros(nq, np.uint32),
        "recompared_in_result": np.zeros(nq, np.uint32),
        "bridge_rows": np.zeros(nq, np.uint32), "hop2_cmps": np.zeros(nq, np.uint32), "max_pruned": np.zeros(nq, np.uint32),
        "final_frontier": [],
    }

    for qi in range(nq):
        self_id = int(query_ids[qi]) if query_ids is not None else -1
        qrow = points[self_id] if query_ids is not None else queries[qi]
        qptr = C.c_void_p(qrow.ctypes.data)
        ok = allow[qi]
        seen_cmp = {}                                    # id -> [dist, times compared, first comparison was beyond the cutoff]
        allowed_cmps = 0

        def dist(a, cutoff=None):
            nonlocal allowed_cmps
            v = F(dist_fn(c_dt, c_m, C.c_void_p(pbase + a * pstride), qptr, c_d))
            if on_distance is not None:
                on_distance(qi, a, v)
            if ok[a]:
                allowed_cmps += 1
                e = seen_cmp.get(a)
                if e is None:
                    seen_cmp[a] = [v, 1, cutoff is not None and bool(v >= cutoff)]
                else:
                    e[1] += 1
            return v

        table = np.full(1 << bits, -1, dtype=np.int64)

        def seen(a):                                     # has_been_seen (:54-59)
            loc = slot_of[a]
            if table[loc] == a:
                return True
            table[loc] = a
            return False

        frontier = []
        for s in starts:                                 # :66-70: compared and inserted whether allowed or not
            frontier.append((dist(s), s))
            seen(s)
        frontier.sort()
        unvisited = list(frontier)
        visited, visit_order = [], []
        dist_cmps = len(starts)
        remain, num_visited, offset = len(frontier), 0, 0
        degree_sum = bridge_rows = hop2_cmps = max_pruned = 0
        cand = []

        while remain > offset and num_visited < limit:   # :107
            cur = unvisited[offset]
            bisect.insort_right(visited, cur)
            visit_order.append(cur)
            num_visited += 1
            full = len(frontier) == beam                 # :115
            row = graph[cur[1]]
            ne = max(min(int(row[0]), degree_limit), 0)  # :130
            degree_sum += ne                             # the visited vertices' rows only
            pruned, bridges = [], []
            for i in range(ne):                          # ---- direct pass ----
                a = int(row[1 + i])
                if seen(a) or a == self_id:
                    continue
                (pruned if ok[a] else bridges).append(a)
            for b in bridges:                            # ---- two-hop pass ----
                if len(pruned) >= fill:
                    break
                bridge_rows += 1
                brow = graph[b]
                for i in range(max(min(int(brow[0]), degree_limit), 0)):
                    c = int(brow[1 + i])
                    if not ok[c]:                        # the hash filter is neither consulted nor written: no third hop
                        continue
                    if seen(c) or c == self_id:
                        continue
                    pruned.append(c)
                    hop2_cmps += 1
            max_pruned = max(max_pruned, len(pruned))
            dist_cmps += len(pruned)                     # :137
            cutoff = frontier[-1][0] if full else BIG    # :150-152, once per visit
            for a in pruned:
                dv = dist(a, cutoff)
                if dv >= cutoff:                         # :157
                    continue
                cand.append((dv, a))
            if len(cand) == 0 or (limit >= 2 * beam and len(cand) < beam // 8 and offset + 1 < remain):   # :162-168
                offset += 1
                continue
            offset = 0
            cand.sort()
            uniq = []
            for c in cand:
                if not uniq or uniq[-1][1] != c[1]:
                    uniq.append(c)
            merged = sorted(set(frontier) | set(uniq))
            cand = []
            msize = min(beam, len(merged))
            if k > 0 and msize > k and mcode == 0:       # :190
                thr = (F(np.float64(cut) * np.float64(merged[k][0])), 0)
                ub = bisect.bisect_right(merged, thr, 0, msize)
                msize = max(ub, len(frontier))
            frontier = merged[:msize]
            vset = set(visited)
            unvisited = [e for e in frontier[:beam] if e not in vset]
            remain = len(unvisited)

        m = min(out_k, len(frontier))
        res["frontier_ids"][qi, :m] = [e[1] for e in frontier[:m]]
        res["frontier_dists"][qi, :m] = [e[0] for e in frontier[:m]]
        res["frontier_size"][qi] = len(frontier)
        res["visited_count"][qi] = len(visited)
        res["dist_cmps"][qi] = dist_cmps
        res["degree_sum"][qi] = degree_sum
        res["final_frontier"].append(list(frontier))
        if visited_cap:
            assert len(visited) <= visited_cap
            v = len(visited)
            res["visited_ids"][qi, :v] = [e[1] for e in visit_order]
            res["visited_dists"][qi, :v] = [e[0] for e in visit_order]
        keys = sorted((e[0], a) for a, e in seen_cmp.items())[:out_k]
        unmerged = {a for _, a in cand}
        res["ids"][qi, :len(keys)] = [a for _, a in keys]
        res["dists"][qi, :len(keys)] = [v for v, _ in keys]
        res["result_count"][qi] = len(keys)
        res["allowed_cmps"][qi] = allowed_cmps
        res["from_beyond_cutoff"][qi] = sum(1 for _, a in keys if seen_cmp[a][2])
        res["from_unmerged"][qi] = sum(1 for _, a in keys if a in unmerged)
        res["recompared_in_result"][qi] = sum(1 for _, a in keys if seen_cmp[a][1] > 1)
        res["bridge_rows"][qi] = bridge_rows
        res["hop2_cmps"][qi] = hop2_cmps
        res["max_pruned"][qi] = max_pruned
    return res
