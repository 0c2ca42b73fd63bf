"""The refused calls of the 18 filter-family entry points (masked / labeled search, fused rerank, exact kNN, grouped exact kNN,
the two label helpers), host and _dev, shared by tests/test_filter_refusals_gpu.py and tests/golden/make_filter_refusals.py.

Every entry has a CHAIN: its conditions in the order in which the library tests them.  A row of the table is one call with one
fault of the chain, or with two faults that are neighbours in it -- the earlier one must win, which pins the order.  Where two
neighbours need the same argument (a null and a misaligned pointer) the earlier one is paired with the next that does not.
Nothing here launches a kernel: every call is refused before its first launch, or has nothing to do (nq == 0)."""
import ctypes as C

import numpy as np

from parlayann_amd import DeviceIndex, _capi

N, D, NQ = 75, 16, 4
W = (N + 31) // 32
G = 3

# one fault = the keyword arguments that differ from a call that would be served
FAULTS = {
    "null_idx": dict(idx=None), "four_bit": dict(idx="four"), "no_labels": dict(idx="bare"), "nq0": dict(nq=0),
    "null_q": dict(q=False), "null_out": dict(out=False), "odd_out": dict(out_off=2), "short_qstride": dict(qstride=4 * D - 4),
    "null_starts": dict(starts=False), "k_gt_beam": dict(k=200), "outk_gt_beam": dict(out_k=65), "outk_gt_64": dict(out_k=65, beam=128),
    "null_allow": dict(allow=False), "bad_stride": dict(stride=1), "stride_w_minus_1": dict(stride=W - 1),
    "bad_kind": dict(kind=5), "null_preds": dict(preds=False), "odd_preds": dict(preds_off=4), "bad_npreds": dict(npreds=2),
    "k0": dict(k=0), "k65": dict(k=65, beam=128), "k65_rows": dict(k=65, stride=W), "k65_preds": dict(k=65, npreds=NQ), "k129": dict(k=129),
    "use_filter": dict(use_filter=1), "full_u8": dict(idx="quant"), "size_mismatch": dict(quant="short"),
    "G0": dict(G=0), "Gbig": dict(G=1 << 32), "null_group": dict(group=None), "bad_index": dict(group="bad"), "stride0_table": dict(stride=0),
    "npreds0": dict(npreds=0),
}
OK_FAULTS = ("nq0", "npreds0")      # not faults: nothing to do, PANN_OK

# entry -> (family, filter form, chain, further single rows, host/dev-only members)
_LAB = ["no_labels", "bad_kind", "null_preds", "odd_preds", "bad_npreds"]
ENTRIES = {
    "pann_batch_search_masked": ("search", "allow", ["null_idx", "k_gt_beam", "outk_gt_beam", "null_allow", "bad_stride", "outk_gt_64", "null_starts"],
                                 ["stride_w_minus_1"]),
    "pann_batch_search_labeled": ("search", "preds", ["null_idx"] + _LAB + ["k_gt_beam", "outk_gt_beam", "outk_gt_64", "null_starts"], []),
    "pann_batch_search_masked_rerank": ("rerank", "allow", ["null_idx", "null_out", "k0", "k_gt_beam", "full_u8", "size_mismatch", "short_qstride",
                                                            "null_starts", "null_q", "use_filter", "null_allow", "bad_stride", "k65", "nq0"],
                                        ["stride_w_minus_1"]),
    "pann_batch_search_labeled_rerank": ("rerank", "preds", ["null_idx", "null_out", "k0", "k_gt_beam", "null_starts", "null_q", "use_filter"] + _LAB
                                         + ["k65", "nq0"], []),
    "pann_bruteforce_knn_masked": ("knn", "allow", ["null_idx", "four_bit", "nq0", "null_q", "null_out", "null_allow", "bad_stride", "short_qstride",
                                                    "k0", "k129"], ["stride_w_minus_1", "k65_rows"]),
    "pann_bruteforce_knn_labeled": ("knn", "preds", ["null_idx", "four_bit", "nq0", "null_q", "null_out"] + _LAB + ["short_qstride", "k0", "k129"],
                                    ["k65_preds"]),
    "pann_bruteforce_knn_masked_grouped": ("grouped", "allow", ["null_idx", "four_bit", "nq0", "null_q", "null_out", "null_allow", "short_qstride", "k0",
                                                                "k129", "G0", "Gbig", "null_group", "stride_w_minus_1", "bad_index"],
                                           ["stride0_table"]),
    "pann_bruteforce_knn_labeled_grouped": ("grouped", "preds", ["null_idx", "four_bit", "nq0", "null_q", "null_out", "no_labels", "bad_kind", "null_preds",
                                                                 "odd_preds", "short_qstride", "k0", "k129", "G0", "Gbig", "null_group", "bad_index"], []),
    "pann_labels_to_allow": ("to_allow", "preds", ["null_idx", "null_out", "odd_out", "no_labels", "bad_kind", "null_preds", "odd_preds",
                                                   "stride_w_minus_1"], ["npreds0"]),
    "pann_label_count": ("count", "preds", ["null_idx", "null_out", "odd_out", "no_labels", "bad_kind", "null_preds", "odd_preds"], ["npreds0"]),
}
DEV_ONLY = {"odd_preds"}        # a host array of predicates needs no alignment
HOST_ONLY = {"bad_index"}       # the device entries find a bad table index on the device, after their launches
# the search entries test nothing after nq == 0 (host) or leave it to the launcher, which returns before its first launch (_dev):
# their nq == 0 row stands alone, outside the chain; the helpers have no host form
HOST_FORM = {e: ENTRIES[e][0] not in ("to_allow", "count") for e in ENTRIES}


def rows():
    """[(row id, entry, dev, fault names)] -- the whole table, in a fixed order"""
    out = []
    for entry, (family, _, chain, singles) in ENTRIES.items():
        for dev in (False, True):
            if not dev and not HOST_FORM[entry]:
                continue
            ch = [f for f in chain if f not in (HOST_ONLY if dev else DEV_ONLY)]
            sets = [[f] for f in ch + singles]
            if family == "search":
                sets.append(["nq0"])
            for i, f in enumerate(ch):
                nxt = next((g for g in ch[i + 1:] if not set(FAULTS[f]) & set(FAULTS[g])), None)
                if nxt:
                    sets.append([f, nxt])
            for s in sets:
                out.append((f"{entry}{'_dev' if dev else ''}:{'+'.join(s)}", entry, dev, s))
    return out


class World:
    """the handles and the buffers of the table, host and device"""

    def __init__(self):
        import torch
        self.torch = torch
        self.lib = _capi.load()
        rng = np.random.default_rng(7)
        X = rng.standard_normal((N, D)).astype(np.float32)
        self.full = DeviceIndex(X, max_degree=4)
        self.full.set_labels((np.arange(N) % 5).astype(np.uint32))
        self.quant, self.qparams = self.full.quantized("euclid_u8", copy_graph=False)
        self.bare = DeviceIndex(X, max_degree=4)
        self.four = DeviceIndex.from_packed(np.zeros((N, D // 2), np.uint8), D, "u4", max_degree=4)
        self.short = DeviceIndex(np.zeros((N - 1, D), np.uint8), max_degree=4)
        self.handles = dict(full=self.full, quant=self.quant, bare=self.bare, four=self.four, short=self.short)
        self.stream = torch.cuda.Stream()
        group = np.array([0, 1, 2, 0], np.uint32)
        bad = group.copy(); bad[2] = G
        host = dict(q=rng.standard_normal((NQ, D)).astype(np.float32), starts=np.zeros(1, np.uint32),
                    allow=np.full((NQ, W), 0xFFFFFFFF, np.uint32), preds=np.tile(np.array([[0, 4]], np.uint32), (NQ + 1, 1)),
                    good=group, bad=bad, ids=np.full((NQ, 129), 0x25A5A5A5, np.uint32), dists=np.full((NQ, 129), -7.0, np.float32),
                    cnt=np.full((5, NQ), 0x25A5A5A5, np.uint32), status=np.full(1, 0x25A5A5A5, np.uint32), rows=np.full((G, W) , 0x25A5A5A5, np.uint32))
        self.host = host
        self.dev = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in host.items()}
        self.outputs = ("ids", "dists", "cnt", "status", "rows")
        torch.cuda.synchronize()

    def close(self):
        for h in self.handles.values():
            h.close()

    def untouched(self):
        self.torch.cuda.synchronize()
        return all((self.dev[k].cpu().numpy().view(self.host[k].dtype) == self.host[k]).all() for k in self.outputs) and \
            (self.host["ids"] == 0x25A5A5A5).all() and (self.host["dists"] == -7.0).all() and (self.host["cnt"] == 0x25A5A5A5).all()

    def call(self, entry, dev, faults):
        """-> (return code, pann_last_error() after the call); the error slot holds another text before it"""
        family, form, _, _ = ENTRIES[entry]
        a = dict(idx="full", quant="quant", q=True, nq=NQ, qstride=4 * D, k=10, beam=64, out_k=10, starts=True, use_filter=0, allow=True,
                 stride=W if family in ("grouped", "to_allow") else 0, kind=_capi.PANN_PRED_RANGE, preds=True, preds_off=0,
                 npreds=G if family == "grouped" else 1, G=G, group="good", out=True, out_off=0)
        for f in faults:
            a.update(FAULTS[f])
        if family == "grouped" and "G" in {k for f in faults for k in FAULTS[f]}:
            a["npreds"] = a["G"]
        B = self.dev if dev else self.host

        def p(name, off=0):
            t = B[name] if isinstance(name, str) else name
            return C.c_void_p((t.data_ptr() if dev else t.ctypes.data) + off)
        h = lambda name: None if name is None else self.handles[name].handle
        lib = self.lib
        stream = [C.c_void_p(self.stream.cuda_stream)] if dev else []
        q, starts = (p("q") if a["q"] else None), (p("starts") if a["starts"] else None)
        allow, preds = (p("allow") if a["allow"] else None), (p("preds", a["preds_off"]) if a["preds"] else None)
        qp = _capi.QueryParams(k=a["k"], beam=a["beam"], cut=1.35, limit=N, degree_limit=4, rerank_factor=100, pad=1.0)
        ids, dists = (p("ids") if a["out"] else None), p("dists")
        cnt = [p(B["cnt"][i]) for i in range(5)]
        group = None if a["group"] is None else p(a["group"])
        assert lib.pann_index_set_option(self.full.handle, b"no-such-option", 0) == 1      # last error := another text
        if family == "search":
            so = _capi.SearchOut(ids=ids, dists=dists, out_k=a["out_k"], frontier_size=cnt[0], visited_count=cnt[1], dist_cmps=cnt[2],
                                 degree_sum=None, visited_ids=None, visited_dists=None, visited_cap=0, status=p("status"))
            filt = [allow, a["stride"]] if form == "allow" else [a["kind"], preds, a["npreds"]]
            args = [h(a["idx"]), q, None, a["nq"], a["qstride"], starts, 1, C.byref(qp)] + filt + [C.byref(so), cnt[3], cnt[4]]
        elif family == "rerank":
            ro = _capi.RerankOut(ids=ids, dists=dists, frontier_size=cnt[0], visited_count=cnt[1], dist_cmps=cnt[2], pruned_cmps=None,
                                 status=p("status"))
            filt = [allow, a["stride"]] if form == "allow" else [a["kind"], preds, a["npreds"]]
            args = [h(a["idx"]), h(a["quant"]), C.byref(self.qparams), q, a["nq"], a["qstride"], 0, a["use_filter"], starts, 1,
                    C.byref(qp)] + filt + [C.byref(ro), cnt[3], cnt[4]]
        elif family == "knn":
            filt = [allow, a["stride"]] if form == "allow" else [a["kind"], preds, a["npreds"]]
            args = [h(a["idx"]), q, a["nq"], a["qstride"], a["k"]] + filt + [ids, dists, cnt[0]]
        elif family == "grouped":
            filt = [allow, a["G"], a["stride"]] if form == "allow" else [a["kind"], preds, a["npreds"]]
            args = [h(a["idx"]), q, a["nq"], a["qstride"], a["k"]] + filt + [group, 0, ids, dists, cnt[0]]
        else:
            out = p("rows" if family == "to_allow" else "cnt", a["out_off"]) if a["out"] else None
            args = [h(a["idx"]), a["kind"], preds, a["npreds"], out] + ([a["stride"]] if family == "to_allow" else [])
        rc = getattr(lib, entry + ("_dev" if dev else ""))(*(args + stream))
        return int(rc), lib.pann_last_error().decode()
