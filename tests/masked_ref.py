"""CPU checker of the masked search: the walk of tests/beam_ref.py (filtered_beam_search, beamSearch.h:22-214, use_filtering ==
false) with the project's own result rule kept beside it (DESIGN.md "Masked search"):

    result of a query = the min(out_k, count) smallest (dist, id) keys among all ALLOWED points whose full distance the
    search computed -- the start points (:66-69) and every `a` of `filtered` (:153-155) whether or not dist < cutoff,
    candidates still unmerged at loop exit included, a point that was compared twice listed once.

The allow mask never reaches the loop: the traversal fields must equal oracle.batch_search for any mask
(tests/test_masked_ref_cpu.py pins that before anything is compared against this file).

Returns every pann_search_out field of the plain search ("frontier_ids" / "frontier_dists" are its ids / dists: the head of the
frontier; visited lists in VISIT order, as the device writes them), the masked result in "ids" / "dists" (padding 0xFFFFFFFF /
+inf), "result_count", "allowed_cmps" and three diagnostics per query:

    from_beyond_cutoff    result entries whose first comparison had dist >= cutoff (the plain search throws those away)
    from_unmerged         result entries that were still unmerged candidates when the loop ended
    recompared_in_result  result entries that were compared more than once (the hash filter is lossy)

on_distance(qi, a, dist): called for every full distance the loop computes, in order -- the hook of the independent statement
of the result in the tests.
"""
import numpy as np

import beam_ref
from beam_ref import BIG, F, FilterSlots, _slots  # noqa: F401  (importable from here as ever)


def unpack_allow(allow, n, nq):
    """boolean (n,) / (nq, n) or packed uint32 (W,) / (nq, W) -> boolean (nq, n) view; bits at positions >= n are dropped"""
    a = np.asarray(allow)
    if a.dtype != np.bool_:
        a = np.unpackbits(np.ascontiguousarray(a.astype("<u4")).view(np.uint8), axis=-1, bitorder="little")[..., :n].astype(bool)
    assert a.shape[-1] == n
    return np.broadcast_to(a, (nq, n))


class Masked(beam_ref.Variant):
    """keeps every full distance of an allowed point; the walk itself is untouched"""

    def __init__(self, w, allow, hook):
        self.w, self.ok, self.hook = w, allow[w.qi], hook
        self.cmp = {}                                    # id -> [dist, times compared, first comparison was beyond the cutoff]
        self.allowed_cmps = 0

    def on_distance(self, a, dist, cutoff):
        if self.hook is not None:
            self.hook(self.w.qi, a, dist)
        if self.ok[a]:
            self.allowed_cmps += 1
            e = self.cmp.get(a)
            if e is None:
                self.cmp[a] = [dist, 1, cutoff is not None and bool(dist >= cutoff)]
            else:
                e[1] += 1

    def end(self):
        out_k, cmp = self.w.out_k, self.cmp
        keys = sorted((e[0], a) for a, e in cmp.items())[:out_k]
        unmerged = {a for _, a in self.w.cand}
        ids, dists = np.full(out_k, 0xFFFFFFFF, np.uint32), np.full(out_k, np.inf, np.float32)
        ids[:len(keys)] = [a for _, a in keys]
        dists[:len(keys)] = [v for v, _ in keys]
        return {"ids": ids, "dists": dists, "result_count": np.uint32(len(keys)), "allowed_cmps": np.uint32(self.allowed_cmps),
                "from_beyond_cutoff": np.uint32(sum(1 for _, a in keys if cmp[a][2])),
                "from_unmerged": np.uint32(sum(1 for _, a in keys if a in unmerged)),
                "recompared_in_result": np.uint32(sum(1 for _, a in keys if cmp[a][1] > 1))}


def masked_batch_search(points, graph, allow, queries=None, query_ids=None, k=10, beam=64, cut=1.35, limit=None,
                        degree_limit=None, starts=(0,), metric="l2", out_k=None, visited_cap=0, on_distance=None):
    allow = unpack_allow(allow, len(points), len(queries) if queries is not None else len(query_ids))
    res = beam_ref.batch_search(points, graph, queries, query_ids, k, beam, cut, limit, degree_limit, starts, metric, out_k, visited_cap,
                                variant=lambda w: Masked(w, allow, on_distance))
    return result_fields(res)


def result_fields(res):
    """what the masked and the steered checker return of the walk's fields: the final frontier stays (the post-filter baseline
    reads it); dist_cmps and pruned_cmps are one counter here, every neighbour of `pruned` gets its distance"""
    return {f: v for f, v in res.items() if f not in ("visited_sorted_ids", "pruned_cmps")}


def post_filter(res, allow, out_k):
    """The baseline a caller has without the masked search: the allowed entries of the plain search's FINAL FRONTIER, first out_k.
    -> (ids, dists) padded like the masked result."""
    nq = len(res["final_frontier"])
    allow = np.asarray(allow)
    assert allow.dtype == np.bool_                    # (n,) or (nq, n)
    allow = np.broadcast_to(allow, (nq, allow.shape[-1]))
    ids = np.full((nq, out_k), 0xFFFFFFFF, np.uint32)
    dists = np.full((nq, out_k), np.inf, np.float32)
    for qi, fr in enumerate(res["final_frontier"]):
        kept = [e for e in fr if allow[qi][e[1]]][:out_k]
        ids[qi, :len(kept)] = [e[1] for e in kept]
        dists[qi, :len(kept)] = [e[0] for e in kept]
    return ids, dists
