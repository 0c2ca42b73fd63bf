"""The refused calls of the 13 search and fused-rerank entry points that tests/filter_refusal_cases.py does not cover -- plain,
filtered, steered, steered labeled, grouped labeled and fused rerank, host and _dev, and the per-query-starts search, which has a
host form only -- shared by tests/test_search_refusals_gpu.py and tests/golden/make_search_refusals.py.

The table has the form of the filter table's: every entry has a CHAIN per form, its conditions in the order in which the library
tests them; a row is one call with one fault of the chain, or with two faults that are neighbours in it (the earlier one must
win).  Where two neighbours need the same argument the earlier one is paired with the next that does not.  The world is the filter
table's (N = 75, D = 16, NQ = 4) with a sketched handle and a few more buffers.  No row launches a kernel: a call is refused by the
entry point's own checks, or -- behind the host round trip's upload or the workspace's allocation -- by the launcher's, before its
first launch; or it has nothing to do (nq == 0).

The chains were read off the library of the commit that tests/golden/search_refusals_v1.json names.  Two things that they show:
the host and the _dev forms test the same conditions in different orders (a host call tests the queries' stride last, behind
nq == 0; a _dev call tests it before the launcher sees nq), and most messages name pann_batch_search whichever entry was called.

set_error sites of the search and rerank sections that no row reaches, and why:
  * "visited list longer than visited_cap", "internal dropped-list overflow": the status word of a launch says so;
  * "pann_batch_search: nq too large" (nq > 0xFFFFFFF0): the workspace of such a batch is sized and allocated first;
  * "workspace too small", "the sketch filter has no masked form", "labels, predicates of a known kind ...", "steering goes with a
    bitmap ...", the launcher's own "at least one start point" on the host path and "Q same size or smaller than k" of the masked
    entries: the entry points rule these out before the launcher runs, no C argument reaches them;
  * search_rerank_dev's "candidates per query" (beam == 0), "no sketch filter, k <= 64": ruled out by the entry's checks; its
    "rows of more than 16382 floats" and "rows too long for the rerank's LDS state" need a handle of that dimension, and the
    launcher's refusals inside a fused call (more starts than beam) come after the launch that prepares the queries;
  * on the _dev forms: a start id or a query id >= n and a table index out of range are not tested on the host at all (the
    grouped entry raises PANN_STATUS_BAD_GROUP on the device), and everything the launcher tests comes, for the grouped _dev
    entry, after the launch that gathers the rows;
  * every hip_fail and every Workspace::ensure failure."""
import ctypes as C

import numpy as np

import filter_refusal_cases as fr
from parlayann_amd import DeviceIndex, _capi, sketch

N, D, NQ, W, G = fr.N, fr.D, fr.NQ, fr.W, fr.G

FAULTS = {
    "null_idx": dict(idx=None), "null_qp": dict(qp=False), "null_out": dict(out=False), "k_gt_beam": dict(k=200),
    "beam_neg": dict(k=-1, beam=-1), "outk_gt_beam": dict(out_k=65), "outk_gt_64": dict(out_k=65, beam=128),
    "four_bit": dict(idx="four"), "no_sketch": dict(idx="full"), "sk_without_q": dict(q=False, qids="qids"), "q_without_sk": dict(sk=False),
    "sq_short": dict(sqstride=4), "null_starts": dict(starts=None), "nstarts0": dict(nstarts=0), "both_q": dict(qids="qids"),
    "neither_q": dict(q=False), "start_oor": dict(starts="bad_st"), "qid_oor": dict(q=False, qids="bad_qids"), "nq0": dict(nq=0),
    "short_qstride": dict(qstride=4 * D - 4), "nstarts_gt_beam": dict(nstarts=2, k=1, beam=1, out_k=1), "lds_too_large": dict(beam=9000),
    "no_labels": dict(idx="bare"), "bad_kind": dict(kind=5), "null_preds": dict(preds=False), "odd_preds": dict(preds_off=4),
    "bad_npreds": dict(npreds=2), "null_allow": dict(allow=False), "bad_stride": dict(stride=1),
    "G0": dict(npreds=0), "Gbig": dict(npreds=1 << 32), "null_group": dict(group=None), "bad_start_rows": dict(start_rows=2),
    "bad_index": dict(group="bad"),
    # fused rerank
    "null_quant": dict(quant=None), "null_qparams": dict(qparams=None), "null_ids": dict(ids=False), "null_dists": dict(dists=False),
    "k0": dict(k=0), "full_u8": dict(idx="quant"), "size_mismatch": dict(quant="short"), "bad_qkind": dict(qparams="badkind"),
    "qparams_misfit": dict(qparams="misfit"), "use_filter_4bit": dict(quant="four", qparams="u4", use_filter=1),
    "use_filter_no_sketch": dict(use_filter=1), "odd_qstride": dict(qstride=4 * D + 2), "beam_gt_4096": dict(beam=5000),
    "null_q": dict(q=False), "odd_q": dict(q_off=2),
}
OK_FAULTS = ("nq0",)

# what the launcher refuses (beam_search.hip), in its order; a host call is there behind its upload, a _dev call behind the workspace
_LAUNCHER = ["beam_neg", "nstarts0", "nstarts_gt_beam", "outk_gt_beam", "neither_q"]
# (a loop over nq entries finds nothing at nq == 0, so nq0 stands in front of the faults that such loops find)
_HOST_TAIL = ["null_starts", "both_q", "start_oor", "nq0", "qid_oor", "short_qstride"]
_PQS_TAIL = ["null_starts", "both_q", "nq0", "start_oor", "qid_oor", "short_qstride"]      # nq x nstarts starts
_MASK = ["outk_gt_beam", "null_allow", "bad_stride", "outk_gt_64"]
_LAB = ["no_labels", "bad_kind", "null_preds", "odd_preds", "bad_npreds"]
_TABLE = ["no_labels", "bad_kind", "null_preds", "odd_preds", "G0", "Gbig", "null_group", "bad_start_rows"]
_RERANK = ["null_idx", "null_qparams", "k0", "k_gt_beam", "full_u8", "size_mismatch", "bad_qkind", "qparams_misfit", "use_filter_4bit",
           "use_filter_no_sketch", "short_qstride", "null_starts", "beam_gt_4096", "null_q"]

# entry -> (family, host chain, _dev chain (None: no such form), further single rows of the host form, of the _dev form)
ENTRIES = {
    "pann_batch_search": ("plain",
                          ["null_idx", "null_qp", "null_out", "k_gt_beam"] + _HOST_TAIL + ["beam_neg", "nstarts_gt_beam", "outk_gt_beam"],
                          ["null_idx", "null_qp", "null_out", "k_gt_beam", "null_starts", "short_qstride", "nq0"] + _LAUNCHER,
                          ["nstarts0", "neither_q", "lds_too_large"], ["both_q", "lds_too_large"]),
    "pann_batch_search_per_query_starts": ("pqs",
                                           ["null_idx", "null_qp", "k_gt_beam"] + _PQS_TAIL + ["beam_neg", "nstarts_gt_beam", "outk_gt_beam"],
                                           None, ["null_out", "nstarts0", "neither_q"], []),
    "pann_batch_search_filtered": ("filtered",
                                   ["null_idx", "null_qp", "k_gt_beam", "four_bit", "no_sketch", "sk_without_q", "sq_short"] + _HOST_TAIL
                                   + ["beam_neg", "nstarts_gt_beam", "outk_gt_beam"],
                                   ["null_idx", "null_qp", "k_gt_beam", "four_bit", "null_starts", "short_qstride", "nq0"] + _LAUNCHER
                                   + ["no_sketch", "q_without_sk", "sq_short"],
                                   ["null_out", "q_without_sk", "nstarts0", "neither_q"], ["null_out", "both_q", "sk_without_q"]),
    "pann_batch_search_steered": ("steered", ["null_idx", "null_qp", "k_gt_beam"] + _MASK + _HOST_TAIL + ["nstarts_gt_beam"],
                                  ["null_idx", "null_qp", "k_gt_beam"] + _MASK + ["null_starts", "short_qstride", "nq0", "nstarts0",
                                                                                  "nstarts_gt_beam", "neither_q"],
                                  ["null_out", "nstarts0", "neither_q"], ["null_out", "both_q"]),
    "pann_batch_search_steered_labeled": ("steered_labeled",
                                          ["null_idx"] + _LAB + ["null_qp", "k_gt_beam", "outk_gt_beam", "outk_gt_64"] + _HOST_TAIL
                                          + ["nstarts_gt_beam"],
                                          ["null_idx"] + _LAB + ["null_qp", "k_gt_beam", "outk_gt_beam", "outk_gt_64", "null_starts",
                                                                 "short_qstride", "nq0", "nstarts0", "nstarts_gt_beam", "neither_q"],
                                          ["null_out", "nstarts0", "neither_q"], ["null_out", "both_q"]),
    "pann_batch_search_grouped_labeled": ("grouped",
                                          ["null_idx"] + _TABLE + ["null_qp", "k_gt_beam", "outk_gt_beam", "outk_gt_64", "null_starts", "both_q",
                                                                   "start_oor", "nq0", "bad_index", "qid_oor", "short_qstride"],
                                          ["null_idx"] + _TABLE + ["null_qp", "k_gt_beam", "outk_gt_beam", "outk_gt_64", "null_starts",
                                                                   "short_qstride"],
                                          ["null_out", "nstarts0", "neither_q"], ["null_out"]),
    "pann_batch_search_rerank": ("rerank", _RERANK + ["start_oor", "nq0"], _RERANK + ["nq0", "odd_q"],
                                 ["null_quant", "null_qp", "null_out", "null_ids", "null_dists", "odd_qstride", "nstarts0"],
                                 ["null_quant", "null_qp", "null_out", "null_ids", "null_dists", "odd_qstride", "nstarts0"]),
}
DEV_ONLY = {"odd_preds"}        # a host array of predicates needs no alignment


def rows():
    """[(row id, entry, dev, fault names)] -- the whole table, in a fixed order"""
    out = []
    for entry, (_, host_chain, dev_chain, host_singles, dev_singles) in ENTRIES.items():
        for dev, chain, singles in ((False, host_chain, host_singles), (True, dev_chain, dev_singles)):
            if chain is None:
                continue
            ch = [f for f in chain if dev or f not in DEV_ONLY]
            sets = [[f] for f in ch + singles]
            for i, f in enumerate(ch):
                nxt = next((g for g in ch[i + 1:] if not set(FAULTS[f]) & set(FAULTS[g])), None)
                if nxt:
                    sets.append([f, nxt])
            for s in sets:
                out.append((f"{entry}{'_dev' if dev else ''}:{'+'.join(s)}", entry, dev, s))
    return out


class World(fr.World):
    """the filter table's world, a handle with a sketch attached, and the buffers the further arguments need"""

    def __init__(self):
        super().__init__()
        torch = self.torch
        X = np.random.default_rng(11).standard_normal((N, D)).astype(np.float32)
        self.sk = DeviceIndex(X, max_degree=4)
        sketch.attach_sketch(self.sk, self.sk, sketch.sketch_params(self.sk, "euclid_bit"))
        self.handles["sk"] = self.sk
        bad_qids = np.arange(NQ, dtype=np.uint32); bad_qids[2] = N
        more = dict(st=np.zeros(8, np.uint32), bad_st=np.full(8, N, np.uint32), qids=np.arange(NQ, dtype=np.uint32),
                    bad_qids=bad_qids, skq=np.zeros((NQ, 16), np.uint8), steer=np.full((NQ, 2), 0x25A5A5A5, np.uint32),
                    pruned=np.full(NQ, 0x25A5A5A5, np.uint32))
        self.host.update(more)
        self.dev.update({k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in more.items()})
        self.outputs = self.outputs + ("steer", "pruned")
        qp = self.qparams
        variant = lambda **kw: _capi.QuantParams(**{**{f: getattr(qp, f) for f, _ in _capi.QuantParams._fields_}, **kw})
        self.qparams_of = dict(good=qp, badkind=variant(kind=99), misfit=variant(dims=D + 1), u4=variant(kind=_capi.PANN_QUANT_EUCLID_U4))
        torch.cuda.synchronize()

    def untouched(self):
        return super().untouched() and (self.host["steer"] == 0x25A5A5A5).all() and (self.host["pruned"] == 0x25A5A5A5).all()

    def call(self, entry, dev, faults):
        """-> (return code, pann_last_error() after the call); the error slot holds another text before it"""
        family = ENTRIES[entry][0]
        a = dict(idx="sk" if family == "filtered" else "full", quant="quant", qparams="good", q=True, q_off=0, qids=None, nq=NQ, qstride=4 * D,
                 k=10, beam=64, out_k=10, starts="st", nstarts=1, qp=True, out=True, ids=True, dists=True, sk=True, sqstride=16,
                 allow=True, stride=0, kind=_capi.PANN_PRED_RANGE, preds=True, preds_off=0, npreds=G if family == "grouped" else 1,
                 group="good", start_rows=1, use_filter=0)
        for f in faults:
            a.update(FAULTS[f])
        if family == "filtered" and not a["q"] and "sk_without_q" not in faults:
            a["sk"] = False      # sketch rows go with queries: a call without queries has none, unless that is its fault
        B = self.dev if dev else self.host

        def p(name, off=0):
            t = B[name] if isinstance(name, str) else name
            return C.c_void_p((t.data_ptr() if dev else t.ctypes.data) + off)
        opt = lambda name, off=0: None if name is None or name is False else p(name, off)
        h = lambda name: None if name is None else self.handles[name].handle
        lib = self.lib
        stream = [C.c_void_p(self.stream.cuda_stream)] if dev else []
        q, qids, starts = opt(a["q"] and "q", a["q_off"]), opt(a["qids"]), opt(a["starts"])
        qp = _capi.QueryParams(k=a["k"], beam=a["beam"], cut=1.35, limit=N, degree_limit=4, rerank_factor=100, pad=1.0)
        qp_ref = C.byref(qp) if a["qp"] else None
        ids, dists = opt(a["ids"] and "ids"), opt(a["dists"] and "dists")
        cnt = [p(B["cnt"][i]) for i in range(5)]
        assert lib.pann_index_set_option(self.full.handle, b"no-such-option", 0) == 1      # last error := another text
        if family == "rerank":
            ro = _capi.RerankOut(ids=ids, dists=dists, frontier_size=cnt[0], visited_count=cnt[1], dist_cmps=cnt[2], pruned_cmps=None,
                                 status=p("status"))
            qparams = None if a["qparams"] is None else C.byref(self.qparams_of[a["qparams"]])
            args = [h(a["idx"]), h(a["quant"]), qparams, q, a["nq"], a["qstride"], 0, a["use_filter"], starts, a["nstarts"], qp_ref,
                    C.byref(ro) if a["out"] else None]
        else:
            so = _capi.SearchOut(ids=ids, dists=dists, out_k=a["out_k"], frontier_size=cnt[0], visited_count=cnt[1], dist_cmps=cnt[2],
                                 degree_sum=None, visited_ids=None, visited_dists=None, visited_cap=0, status=p("status"))
            so_ref = C.byref(so) if a["out"] else None
            head = [h(a["idx"]), q, qids, a["nq"], a["qstride"]]
            preds = [a["kind"], opt(a["preds"] and "preds", a["preds_off"]), a["npreds"]]
            if family in ("plain", "pqs"):
                args = head + [starts, a["nstarts"], qp_ref, so_ref]
            elif family == "filtered":
                args = head + [opt(a["sk"] and "skq"), a["sqstride"], starts, a["nstarts"], qp_ref, so_ref, p("pruned")]
            elif family == "steered":
                args = head + [starts, a["nstarts"], qp_ref, opt(a["allow"] and "allow"), a["stride"], so_ref, cnt[3], cnt[4], 0, p("steer")]
            elif family == "steered_labeled":
                args = head + [starts, a["nstarts"], qp_ref] + preds + [so_ref, cnt[3], cnt[4], 0, p("steer")]
            else:
                args = head + [starts, a["nstarts"], a["start_rows"], qp_ref] + preds + [opt(a["group"]), so_ref, cnt[3], cnt[4], 1, 0, p("steer")]
        rc = getattr(lib, entry + ("_dev" if dev else ""))(*(args + stream))
        return int(rc), lib.pann_last_error().decode()
