"""CPU model of the beam-64 search with the second-sighting table V ("Second sightings"): a Python restatement of
filtered_beam_search (beamSearch.h:22-214, use_filtering == false), as tests/masked_ref.py, in which a neighbour that the
lossy filter H lets through a second time is NOT given a distance when V still knows it:

    V      v_n direct-mapped entries: entry id & (v_n - 1) holds id >> log2(v_n).  An id enters V when has_been_seen overwrites
           it in H with another id (victim policy); a match means "this query compared this id before".
    lookup for a neighbour that H kept (it is counted in dist_cmps as ever), while the frontier is full, the cutoff is at most
           the reference's BIG, and no cut-prune has left the frontier at or below k entries.  On a match the outcome comes
           from the state: in the frontier with dist < cutoff -> that (dist, id) joins the candidates; else among the pending
           candidates -> the same pair joins them again; else nothing.

Every other line is the reference's, so ids, dists and all counters must equal oracle.batch_search: that is the exactness
claim of the kernel, checked here where every step can be read.  `insert="all"` puts every compared id into V instead
(the policy the measurement in DESIGN.md compares the victims with).

Returns the plain search's outputs and, per query, "skipped" (distances not computed), "repeats" (comparisons of an id this
query compared before: what a V without misses would skip once the frontier is full) and "lookups" (neighbours looked up).
"""
import bisect
import ctypes as C
import math

import numpy as np

import oracle_api
from masked_ref import BIG, F, FilterSlots

_slots = {}


def seen_batch_search(points, graph, queries=None, query_ids=None, k=10, beam=64, cut=1.35, limit=None, degree_limit=None,
                      starts=(0,), metric="l2", out_k=None, v_n=512, insert="victims"):
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
    assert v_n == 0 or (v_n & (v_n - 1)) == 0
    vshift = v_n.bit_length() - 1
    assert v_n == 0 or n <= 0xFFFF << vshift             # every tag below the empty value
    cut_prunes = k > 0 and mcode == 0                    # :190 (is_metric(): L2 only)
    use_v = v_n != 0 and (not cut_prunes or cut >= 0.0)  # make_plan's conditions

    bits = max(10, int(math.ceil(math.log2(float(beam) * float(beam)))) - 2)           # :52
    if bits not in _slots:
        _slots[bits] = FilterSlots(o, bits)
    slot_of = _slots[bits]
    pbase, pstride = points.ctypes.data, points.strides[0]
    dist_fn = o.lib.pann_oracle_distance
    c_dt, c_m, c_d = C.c_int(dt), C.c_int(mcode), C.c_uint32(d)

    res = {
        "ids": np.full((nq, out_k), 0xFFFFFFFF, np.uint32), "dists": np.full((nq, out_k), np.inf, np.float32),
        "frontier_size": np.zeros(nq, np.uint32), "visited_count": np.zeros(nq, np.uint32),
        "dist_cmps": np.zeros(nq, np.uint32), "degree_sum": np.zeros(nq, np.uint32),
        "skipped": np.zeros(nq, np.uint32), "repeats": np.zeros(nq, np.uint32), "lookups": np.zeros(nq, np.uint32),
    }

    for qi in range(nq):
        self_id = int(query_ids[qi]) if query_ids is not None else -1
        qrow = points[self_id] if query_ids is not None else queries[qi]
        qptr = C.c_void_p(qrow.ctypes.data)

        def dist(a):
            return F(dist_fn(c_dt, c_m, C.c_void_p(pbase + a * pstride), qptr, c_d))

        table = {}                                       # slot -> id (hash_filter, :53)
        vtab = {}                                        # V: entry -> tag
        compared = set()

        victims = []                                     # ids H forgot while one row was filtered

        def v_insert(a):
            vtab[a & (v_n - 1)] = a >> vshift

        def v_flush():
            # the victims of a row enter V after the row's comparisons: a neighbour that a later neighbour of the SAME row
            # pushed out of H is compared further down in this row, not before it
            for a in victims:
                v_insert(a)
            victims.clear()

        def seen(a):                                     # has_been_seen (:54-59), with the victim's way towards V
            loc = slot_of[a]
            old = table.get(loc, -1)
            if old == a:
                return True
            table[loc] = a
            if use_v and insert == "victims" and old != -1:
                victims.append(old)
            return False

        frontier = []
        for s in starts:                                 # :66-70
            frontier.append((dist(s), s))
            compared.add(s)
            seen(s)
        v_flush()
        frontier.sort()
        unvisited = list(frontier)
        visited = []
        dist_cmps = len(starts)
        remain, num_visited, offset = len(frontier), 0, 0
        degree_sum = 0
        cand = []
        v_ok = True
        skipped = repeats = lookups = 0

        while remain > offset and num_visited < limit:   # :107
            cur = unvisited[offset]
            bisect.insort_right(visited, cur)
            num_visited += 1
            full = len(frontier) == beam                 # :115
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
            cutoff = frontier[-1][0] if full else BIG    # :150-152
            look = use_v and full and v_ok and cutoff <= BIG
            for a in pruned:
                if a in compared:
                    repeats += 1
                if look:
                    lookups += 1
                    if vtab.get(a & (v_n - 1), 0xFFFF) == a >> vshift:
                        assert a in compared             # V has no false positives
                        skipped += 1
                        inf = [e for e in frontier if e[1] == a]
                        inc = [e for e in cand if e[1] == a]
                        if inf:
                            if inf[0][0] < cutoff:
                                cand.append(inf[0])
                        elif inc:
                            cand.append(inc[0])
                        continue
                dv = dist(a)
                compared.add(a)
                if use_v and insert == "all":
                    v_insert(a)
                if dv >= cutoff:                         # :157
                    continue
                cand.append((dv, a))
            v_flush()
            if len(cand) == 0 or (limit >= 2 * beam and len(cand) < beam // 8 and offset + 1 < remain):   # :162-168
                offset += 1
                continue
            offset = 0
            cand.sort()                                  # :173
            uniq = []
            for c in cand:                               # std::unique by id (:174-175)
                if not uniq or uniq[-1][1] != c[1]:
                    uniq.append(c)
            merged = sorted(set(frontier) | set(uniq))   # :178-181
            cand = []
            msize = min(beam, len(merged))               # :185
            if cut_prunes and msize > k:                 # :190
                thr = (F(np.float64(cut) * np.float64(merged[k][0])), 0)
                ub = bisect.bisect_right(merged, thr, 0, msize)
                msize = max(ub, len(frontier))
                if msize <= k:
                    v_ok = False                         # entry k is gone: the next threshold may be a higher one
            frontier = merged[:msize]                    # :198-200
            vset = set(visited)
            unvisited = [e for e in frontier[:beam] if e not in vset]      # :203-208
            remain = len(unvisited)

        m = min(out_k, len(frontier))
        res["ids"][qi, :m] = [e[1] for e in frontier[:m]]
        res["dists"][qi, :m] = [e[0] for e in frontier[:m]]
        res["frontier_size"][qi] = len(frontier)
        res["visited_count"][qi] = len(visited)
        res["dist_cmps"][qi] = dist_cmps
        res["degree_sum"][qi] = degree_sum
        res["skipped"][qi], res["repeats"][qi], res["lookups"][qi] = skipped, repeats, lookups
    return res
