"""CPU checker of the two-level search: a Python restatement of filtered_beam_search (beamSearch.h:22-214) WITH its
use_filtering branch (:98-100,117-123,139-146), which the C++ oracle does not have.

Distances and the hash are the oracle's own (pann_oracle_distance, pann_oracle_hash64_2); the threshold arithmetic is
np.float32; sketch rows and sketch distances are parlayann_amd.sketch's numpy reference.  With use_filtering=False the
function must equal oracle.batch_search field for field (tests/test_filtered_ref_cpu.py pins that before anything is
compared against it).

Returns every pann_search_out field (visited lists in VISIT order, as the device writes them; "visited_sorted_ids" is the
reference's (dist, id) order), "pruned_cmps" (the reference's local dist_cmps) and "sketch_dropped": per query, how many
neighbours the sketch kept from a full distance.
"""
import bisect
import ctypes as C
import math

import numpy as np

import masked_ref
import oracle_api
from parlayann_amd import sketch as sk

F = np.float32
BIG = F(2147483648.0)          # (distanceType) numeric_limits<int>::max()  (:152)


def filtered_batch_search(points, graph, queries=None, query_ids=None, k=10, beam=64, cut=1.35, limit=None, degree_limit=None,
                          starts=(0,), metric="l2", out_k=None, visited_cap=0, use_filtering=False, sketches=None,
                          sketch_queries=None, sketch_params=None):
    o = oracle_api.load()
    points = np.ascontiguousarray(points)
    graph = np.ascontiguousarray(graph, dtype=np.uint32)
    n, d = points.shape
    maxdeg = graph.shape[1] - 1
    nq = len(queries) if queries is not None else len(query_ids)
    out_k = k if out_k is None else out_k
    limit = n if limit is None else limit
    degree_limit = maxdeg if degree_limit is None else degree_limit
    starts = [int(s) for s in starts]
    mcode = oracle_api.METRIC[metric.lower() if isinstance(metric, str) else metric]
    dt = oracle_api.DT[points.dtype]
    if queries is not None:
        queries = np.ascontiguousarray(queries)
        assert queries.dtype == points.dtype
    if use_filtering:
        assert sketches is not None and sketch_params is not None
        assert (queries is None) == (sketch_queries is None)

    bits = max(10, int(math.ceil(math.log2(float(beam) * float(beam)))) - 2)           # :52
    hmask = (1 << bits) - 1
    slot_of = masked_ref.FilterSlots(o, bits)                                           # hash64_2(a) & ((1 << bits) - 1)
    pbase, pstride = points.ctypes.data, points.strides[0]
    dist_fn = o.lib.pann_oracle_distance
    c_dt, c_m, c_d = C.c_int(dt), C.c_int(mcode), C.c_uint32(d)

    res = {
        "ids": np.full((nq, out_k), 0xFFFFFFFF, np.uint32), "dists": np.full((nq, out_k), np.inf, np.float32),
        "frontier_size": np.zeros(nq, np.uint32), "visited_count": np.zeros(nq, np.uint32),
        "dist_cmps": np.zeros(nq, np.uint32), "degree_sum": np.zeros(nq, np.uint32),
        "visited_ids": np.zeros((nq, visited_cap), np.uint32) if visited_cap else None,
        "visited_dists": np.zeros((nq, visited_cap), np.float32) if visited_cap else None,
        "visited_sorted_ids": np.zeros((nq, visited_cap), np.uint32) if visited_cap else None,
        "pruned_cmps": np.zeros(nq, np.uint32), "sketch_dropped": np.zeros(nq, np.uint32),
    }

    for qi in range(nq):
        self_id = int(query_ids[qi]) if query_ids is not None else -1
        qrow = points[self_id] if query_ids is not None else queries[qi]
        qptr = C.c_void_p(qrow.ctypes.data)
        memo = {}

        def dist(a):                                     # Points[a].distance(p)
            v = memo.get(a)
            if v is None:
                v = memo[a] = F(dist_fn(c_dt, c_m, C.c_void_p(pbase + a * pstride), qptr, c_d))
            return v

        qq = None
        if use_filtering:
            qq = sketches[self_id] if query_ids is not None else sketch_queries[qi]

        def sdist(a):                                    # Q_Points[a].distance(qp)
            return F(sk.sketch_distance_numpy(sketches[a:a + 1], qq, sketch_params)[0])

        table = np.full(1 << bits, -1, dtype=np.int64)

        def seen(a):                                     # has_been_seen (:54-59)
            loc = slot_of[a]
            if table[loc] == a:
                return True
            table[loc] = a
            return False

        frontier = []                                    # (dist, id) tuples: tuple order == less (:46-48)
        for s in starts:                                 # :66-70
            frontier.append((dist(s), s))
            seen(s)
        frontier.sort()
        unvisited = list(frontier)
        visited, visit_order = [], []
        dist_cmps = full_dist_cmps = len(starts)         # :83-84
        remain, num_visited, offset = len(frontier), 0, 0
        degree_sum = dropped = 0
        cand = []
        fsum, fcount, fthr = F(0.0), 0, F(0.0)           # :98-100

        while remain > offset and num_visited < limit:   # :107
            cur = unvisited[offset]
            bisect.insort_right(visited, cur)            # :112-113
            visit_order.append(cur)
            num_visited += 1
            full = len(frontier) == beam                 # :115
            if use_filtering and full:                   # :119-123
                fsum = F(fsum + sdist(frontier[-1][1]))
                fcount += 1
                fthr = F(fsum / F(fcount))
            row = graph[cur[1]]
            ne = max(min(int(row[0]), degree_limit), 0)  # :130
            degree_sum += ne
            pruned = []
            for i in range(ne):
                a = int(row[1 + i])
                if seen(a) or a == self_id:              # :133
                    continue
                pruned.append(a)
            dist_cmps += len(pruned)                     # :137
            if use_filtering and full:                   # :140-146
                sd = sk.sketch_distance_numpy(sketches[pruned], qq, sketch_params) if pruned else []
                filtered = [a for a, v in zip(pruned, sd) if not (F(v) >= fthr)]
                dropped += len(pruned) - len(filtered)
            else:
                filtered = pruned
            cutoff = frontier[-1][0] if full else BIG    # :150-152
            for a in filtered:
                dv = dist(a)
                full_dist_cmps += 1
                if dv >= cutoff:                         # :157
                    continue
                cand.append((dv, a))
            if len(cand) == 0 or (limit >= 2 * beam and len(cand) < beam // 8 and offset + 1 < remain):   # :162-168
                offset += 1
                continue
            offset = 0
            cand.sort()                                  # :173
            uniq = []
            for c in cand:                               # std::unique by id (:174-175)
                if not uniq or uniq[-1][1] != c[1]:
                    uniq.append(c)
            merged = sorted(set(frontier) | set(uniq))   # set_union of two sorted, duplicate-free ranges (:178-181)
            cand = []
            msize = min(beam, len(merged))               # :185
            if k > 0 and msize > k and mcode == 0:       # :190 (is_metric(): L2 only)
                thr = (F(np.float64(cut) * np.float64(merged[k][0])), 0)
                ub = bisect.bisect_right(merged, thr, 0, msize)
                msize = max(ub, len(frontier))
            frontier = merged[:msize]                    # :198-200
            vset = set(visited)
            unvisited = [e for e in frontier[:beam] if e not in vset]      # :203-208
            remain = len(unvisited)

        m = min(out_k, len(frontier))
        res["ids"][qi, :m] = [e[1] for e in frontier[:m]]
        res["dists"][qi, :m] = [e[0] for e in frontier[:m]]
        res["frontier_size"][qi] = len(frontier)
        res["visited_count"][qi] = len(visited)
        res["dist_cmps"][qi] = full_dist_cmps            # what the reference returns (:213)
        res["pruned_cmps"][qi] = dist_cmps
        res["degree_sum"][qi] = degree_sum
        res["sketch_dropped"][qi] = dropped
        if visited_cap:
            assert len(visited) <= visited_cap
            v = len(visited)
            res["visited_ids"][qi, :v] = [e[1] for e in visit_order]
            res["visited_dists"][qi, :v] = [e[0] for e in visit_order]
            res["visited_sorted_ids"][qi, :v] = [e[1] for e in visited]
    return res
