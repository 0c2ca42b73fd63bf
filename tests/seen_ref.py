"""CPU model of the beam-64 search with the second-sighting table V ("Second sightings"): the walk of
tests/beam_ref.py (filtered_beam_search, beamSearch.h:22-214, use_filtering == false), in which a neighbour that the lossy filter
H lets through a second time is NOT given a distance when V still knows it:

    V      v_n direct-mapped entries: entry id & (v_n - 1) holds id >> log2(v_n).  An id enters V when has_been_seen overwrites
           it in H with another id (victim policy); a match means "this query compared this id before".
    lookup for a neighbour that H kept (it is counted in dist_cmps as ever), while the frontier is full, the cutoff is at most
           the reference's BIG, and no cut-prune has left the frontier at or below k entries.  On a match the outcome comes
           from the state: in the frontier with dist < cutoff -> that (dist, id) joins the candidates; else among the pending
           candidates -> the same pair joins them again; else nothing.

Every other line is the reference's, so ids, dists and all counters must equal oracle.batch_search: that is the exactness
claim of the kernel, checked here where every step can be read.  `insert="all"` puts every compared id into V instead
(the policy the measurement in DESIGN.md compares the victims with); the start points do not enter V under either policy.

Returns the plain search's outputs ("dist_cmps" is the reference's counter: a neighbour that V settles is still counted) and,
per query, "skipped" (distances not computed), "repeats" (comparisons of an id this query compared before: what a V without
misses would skip once the frontier is full) and "lookups" (neighbours looked up).
"""
import numpy as np

import beam_ref
from beam_ref import BIG


class SecondSightings(beam_ref.Variant):
    def __init__(self, w, v_n, cut, insert):
        self.w, self.v_n, self.vshift = w, v_n, v_n.bit_length() - 1
        use_v = v_n != 0 and (not w.cut_prunes or cut >= 0.0)           # make_plan's conditions
        self.insert = insert if use_v else None
        self.vtab = {}                                   # V: entry -> tag
        self.compared = set()
        self.victims = []                                # ids H forgot while one row was filtered
        self.v_ok = True
        self.skipped = self.repeats = self.lookups = 0

    def v_insert(self, a):
        self.vtab[a & (self.v_n - 1)] = a >> self.vshift

    def on_evict(self, old):
        if self.insert == "victims":
            self.victims.append(old)

    def after_row(self):
        # the victims of a row enter V after the row's comparisons: a neighbour that a later neighbour of the SAME row
        # pushed out of H is compared further down in this row, not before it
        for a in self.victims:
            self.v_insert(a)
        self.victims.clear()

    def settle(self, a, cutoff, full):
        w = self.w
        if a in self.compared:
            self.repeats += 1
        if not (self.insert and full and self.v_ok and cutoff <= BIG):
            return False
        self.lookups += 1
        if self.vtab.get(a & (self.v_n - 1), 0xFFFF) != a >> self.vshift:
            return False
        assert a in self.compared                        # V has no false positives
        self.skipped += 1
        inf = [e for e in w.frontier if e[1] == a]
        inc = [e for e in w.cand if e[1] == a]
        if inf:
            if inf[0][0] < cutoff:
                w.cand.append(inf[0])
        elif inc:
            w.cand.append(inc[0])
        return True

    def on_distance(self, a, dist, cutoff):
        self.compared.add(a)
        if self.insert == "all" and cutoff is not None:
            self.v_insert(a)

    def after_cut_prune(self, msize):
        if msize <= self.w.k:
            self.v_ok = False                            # entry k is gone: the next threshold may be a higher one

    def end(self):
        return {"skipped": np.uint32(self.skipped), "repeats": np.uint32(self.repeats), "lookups": np.uint32(self.lookups)}


def seen_batch_search(points, graph, queries=None, query_ids=None, k=10, beam=64, cut=1.35, limit=None, degree_limit=None,
                      starts=(0,), metric="l2", out_k=None, v_n=512, insert="victims"):
    assert v_n == 0 or (v_n & (v_n - 1)) == 0
    assert v_n == 0 or len(points) <= 0xFFFF << (v_n.bit_length() - 1)         # every tag below the empty value
    res = beam_ref.batch_search(points, graph, queries, query_ids, k, beam, cut, limit, degree_limit, starts, metric, out_k,
                                variant=lambda w: SecondSightings(w, v_n, cut, insert))
    res["dist_cmps"] = res["pruned_cmps"]
    return {f: res[f] for f in ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum", "skipped", "repeats", "lookups")}
