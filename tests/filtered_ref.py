"""CPU checker of the two-level search: the walk of tests/beam_ref.py (filtered_beam_search, beamSearch.h:22-214) WITH the
reference's use_filtering branch (:98-100,117-123,139-146), which the C++ oracle does not have:

    while the frontier is full, a visit first adds the sketch distance of the frontier's last entry to a running mean -- the
    threshold (:119-123) -- and then keeps from a full distance every neighbour of `pruned` whose sketch distance is >= that
    threshold (:140-146).

Distances and the hash are the oracle's own; the threshold arithmetic is np.float32; sketch rows and sketch distances are
parlayann_amd.sketch's numpy reference.  With use_filtering=False the function must equal oracle.batch_search field for
field (tests/test_filtered_ref_cpu.py pins that before anything is compared against it).

Returns every pann_search_out field (visited lists in VISIT order, as the device writes them; "visited_sorted_ids" is the
reference's (dist, id) order; "dist_cmps" counts full distances, as the reference returns it, :213), "pruned_cmps" (the
reference's local dist_cmps) and "sketch_dropped": per query, how many neighbours the sketch kept from a full distance.
"""
import numpy as np

import beam_ref
from beam_ref import F
from parlayann_amd import sketch as sk


class Sketched(beam_ref.Variant):
    def __init__(self, w, on, sketches, sketch_queries, params):
        self.w, self.on, self.sketches, self.params = w, on, sketches, params
        if on:
            self.qq = sketches[w.self_id] if w.self_id >= 0 else sketch_queries[w.qi]
        self.fsum, self.fcount, self.fthr = F(0.0), 0, F(0.0)           # :98-100
        self.dropped = 0

    def sdist(self, ids):                                # Q_Points[a].distance(qp)
        return sk.sketch_distance_numpy(self.sketches[ids], self.qq, self.params)

    def before_distances(self, pruned, full):
        if not (self.on and full):
            return pruned
        last = self.w.frontier[-1][1]
        self.fsum = F(self.fsum + F(self.sdist(slice(last, last + 1))[0]))             # :119-123
        self.fcount += 1
        self.fthr = F(self.fsum / F(self.fcount))
        sd = self.sdist(pruned) if pruned else []                                      # :140-146
        kept = [a for a, v in zip(pruned, sd) if not (F(v) >= self.fthr)]
        self.dropped += len(pruned) - len(kept)
        return kept

    def end(self):
        return {"sketch_dropped": np.uint32(self.dropped)}


def filtered_batch_search(points, graph, queries=None, query_ids=None, k=10, beam=64, cut=1.35, limit=None, degree_limit=None,
                          starts=(0,), metric="l2", out_k=None, visited_cap=0, use_filtering=False, sketches=None,
                          sketch_queries=None, sketch_params=None):
    if use_filtering:
        assert sketches is not None and sketch_params is not None
        assert (queries is None) == (sketch_queries is None)
    res = beam_ref.batch_search(points, graph, queries, query_ids, k, beam, cut, limit, degree_limit, starts, metric, out_k, visited_cap,
                                variant=lambda w: Sketched(w, use_filtering, sketches, sketch_queries, sketch_params))
    return {f: v for f, v in res.items() if f not in ("frontier_ids", "frontier_dists", "final_frontier")}
