"""CPU checker of the steered masked search (DESIGN.md "Steered masked search"): tests/masked_ref.py's checker -- the walk of
tests/beam_ref.py (filtered_beam_search, beamSearch.h:22-214, use_filtering == false) and the masked result rule -- with ONE
change: how the list `pruned` of a visited vertex is made (:128-137):

    direct pass   for the first min(size, degree_limit) neighbours a of cur, in row order: seen(a) or a == self -> skipped;
                  allowed -> pruned; otherwise -> bridges
    two-hop pass  for each bridge b in order: stop when len(pruned) >= fill (a bridge's row is taken whole or not at all); for
                  the first min(size(b), degree_limit) neighbours c of b: not allowed -> skipped WITHOUT touching the hash filter;
                  seen(c) or c == self -> skipped; otherwise -> pruned

fill: 1..deg_eff, deg_eff = min(degree_limit, max_deg); 0 means deg_eff, a larger value is clamped.  Everything else -- the
cutoff, the distances, the skip rule, the merge, the cut-prune, the visited list, the result rule -- is masked_ref's, word for word.
Start points are compared whether allowed or not; degree_sum counts the visited vertices' rows only.

Returns the dictionary of masked_ref.masked_batch_search plus per query

    bridge_rows   bridge rows expanded
    hop2_cmps     entries the two-hop pass appended to pruned
    max_pruned    the longest `pruned` of any visit (diagnostic; bound: fill - 1 + deg_eff)
"""
import numpy as np

import beam_ref
import masked_ref


def effective_fill(fill, degree_limit, maxdeg):
    deg_eff = max(min(int(degree_limit), int(maxdeg)), 0)
    return deg_eff if fill == 0 or fill > deg_eff else int(fill)


class Steered(masked_ref.Masked):
    def __init__(self, w, allow, hook, fill):
        super().__init__(w, allow, hook)
        self.fill = fill
        self.bridge_rows = self.hop2_cmps = self.max_pruned = 0

    def after_direct_pass(self, direct):
        w, ok = self.w, self.ok
        pruned = [a for a in direct if ok[a]]
        for b in (a for a in direct if not ok[a]):       # ---- two-hop pass: the bridges have passed seen(), so the hash filter holds them ----
            if len(pruned) >= self.fill:
                break
            self.bridge_rows += 1
            for c in w.row(b):
                if not ok[c]:                            # the hash filter is neither consulted nor written: no third hop
                    continue
                if w.seen(c) or c == w.self_id:
                    continue
                pruned.append(c)
                self.hop2_cmps += 1
        self.max_pruned = max(self.max_pruned, len(pruned))
        return pruned

    def end(self):
        return dict(super().end(), bridge_rows=np.uint32(self.bridge_rows), hop2_cmps=np.uint32(self.hop2_cmps),
                    max_pruned=np.uint32(self.max_pruned))


def steered_batch_search(points, graph, allow, fill=0, queries=None, query_ids=None, k=10, beam=64, cut=1.35, limit=None,
                         degree_limit=None, starts=(0,), metric="l2", out_k=None, visited_cap=0, on_distance=None):
    maxdeg = np.shape(graph)[1] - 1
    fill = effective_fill(fill, maxdeg if degree_limit is None else degree_limit, maxdeg)
    allow = masked_ref.unpack_allow(allow, len(points), len(queries) if queries is not None else len(query_ids))
    res = beam_ref.batch_search(points, graph, queries, query_ids, k, beam, cut, limit, degree_limit, starts, metric, out_k, visited_cap,
                                variant=lambda w: Steered(w, allow, on_distance, fill))
    return masked_ref.result_fields(res)
