"""The stream-ordering contract of the device-pointer entry points (include/pann.h: "launched on `stream`; no sync, no alloc"),
under the busy-stream harness of tests/stream_order.py (DESIGN.md "Stream order").

Every case enqueues, on ONE side stream and with no host step in between: a delay, the copy of the real inputs over decoys,
a poison fill of the outputs, and TWO calls of the entry point (64 queries, then 37, other inputs, separate outputs: the second
call lays its scratch over the first one's).  A launch, memset or copy that the library put on any other stream runs during the
delay, on decoys, and is poisoned over.  Expected values are the CPU references the entry points' own tests use (the oracle,
masked_ref, filtered_ref, numpy); where such a test has only the host entry point to compare with (normalize_first on the fused
rerank), the host entries run on a second, idle pair of handles.  Everything is integer-valued, so every comparison is bit for
bit.  Every case runs on each of two side streams that were probed to overtake each other (stream_order.independent_streams)."""
import ctypes as C

import numpy as np
import pytest
import torch

import delete_ref as dr
import filtered_ref
import masked_knn_cases as mkc
import masked_ref
import stream_order as so
import two_phase_cases as tp
from parlayann_amd import DeviceIndex, _capi, datasets, quantize
from parlayann_amd import distributed as dist
from parlayann_amd import sketch as sk
from parlayann_amd.index import allow_count, label_allow, pack_allow

pytestmark = pytest.mark.gpu

N, D, DM, K, R, L = 2000, 64, 100, 10, 16, 32
NQS = (64, 37)                         # the two calls behind one delay
WORDS = (N + 31) // 32
SENT = 0xFFFFFFFF
U32, F32 = np.uint32, np.float32
SEARCH_FIELDS = ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum")
STARTS = {1: ((0,), (7,)), 3: ((0, 500, 1500), (3, 900, 1999))}          # per number of starts: first call, second call
DECOY_STARTS = {1: (1,), 3: (11, 12, 13)}


def _dev():
    return torch.device("cuda", 0)


def _bytes(a, slack=0):
    """a numpy array as a flat uint8 device tensor (+ `slack` zero bytes: the kernels read query rows in 16-byte chunks)"""
    b = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    if slack:
        b = np.concatenate([b, np.zeros(slack, np.uint8)])
    return torch.from_numpy(b.copy()).to(_dev())


class Out:
    """an output array on the device"""

    def __init__(self, shape, dtype=U32):
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.t = torch.zeros(int(np.prod(shape)) * self.dtype.itemsize, dtype=torch.uint8, device=_dev())

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        return self.t.cpu().numpy().view(self.dtype).reshape(self.shape)


def _vp(t):
    """a device address for the C-ABI: of an Out, of a tensor, or the integer itself"""
    return C.c_void_p(t if isinstance(t, int) else t.ptr if isinstance(t, Out) else t.data_ptr())


class Plan:
    """the buffers, calls and expectations of one schedule"""

    def __init__(self):
        self.ins, self.outs, self.calls, self.expect = [], [], [], []
        self.after_warm_up = None

    def late(self, real, decoy, slack=0):
        """an input that reaches its buffer only behind the delay; until then the buffer holds the decoy -> the buffer"""
        real, decoy = np.ascontiguousarray(real), np.ascontiguousarray(decoy)
        assert real.shape == decoy.shape and real.dtype == decoy.dtype and not np.array_equal(real, decoy)
        buf = _bytes(decoy, slack)
        self.ins.append((buf, _bytes(real, slack), _bytes(decoy, slack)))
        return buf

    def out(self, shape, dtype=U32, expect=None, name=""):
        o = Out(shape, dtype)
        self.outs.append(o)
        if expect is not None:
            self.expect.append((name, o, expect))
        return o

    def want(self, name, o, expect):
        self.expect.append((name, o, expect))


def _run(stream, plan, early=True, label=""):
    """warm up with the real inputs (synchronised), put the decoys back, run the schedule, compare every output"""
    with torch.cuda.stream(stream):
        for buf, real, _ in plan.ins:
            buf.copy_(real)
    for call in plan.calls:
        call(stream)
    stream.synchronize()
    if plan.after_warm_up:
        plan.after_warm_up()
    with torch.cuda.stream(stream):
        for buf, _, decoy in plan.ins:
            buf.copy_(decoy)
    stream.synchronize()
    returned_early = so.run_behind_delay(stream, [(b, r) for b, r, _ in plan.ins], [o.t for o in plan.outs],
                                         [lambda c=c: c(stream) for c in plan.calls])
    so.HOST_MS[-1] = (so.HOST_MS[-1], early, label)
    for name, o, exp in plan.expect:
        got, exp = o.get(), np.ascontiguousarray(exp)
        assert got.dtype.itemsize == exp.dtype.itemsize and got.shape == exp.shape, name
        if got.tobytes() != exp.tobytes():                        # bit for bit; the typed comparison words the failure
            np.testing.assert_array_equal(got.view(exp.dtype), exp, err_msg=f"{label}: {name}")
            raise AssertionError(f"{label}: {name} differs in its bits")
    if early:
        assert returned_early, f"{label}: the call came back only after the delay had run out: it synchronised"


def _sp(stream):
    return C.c_void_p(stream.cuda_stream)


# ---- the table, built once ---------------------------------------------------------------------------------------------------

class Env:
    def __init__(self, oracle):
        self.o = oracle
        self.lib = _capi.load()
        X8 = datasets.sift_like(N, D, seed=1001, dtype=np.uint8)
        self.X = {"u8": X8, "f16": X8.astype(np.float16), "f32": X8.astype(F32),
                  "i8": (datasets.sift_like(N, DM, seed=1002, dtype=F32) - 128).clip(-127, 127).astype(np.int8)}
        self.metric = {"u8": "l2", "f16": "l2", "f32": "l2", "i8": "mips"}
        self.G = {}
        self.G["u8"] = self.G["f16"] = self.G["f32"] = oracle.vamana_build(X8, R, L, 1.2, num_passes=1, seed=5)[0]
        self.G["i8"] = oracle.vamana_build(self.X["i8"], R, L, 1.0, num_passes=1, seed=5, metric="mips")[0]
        self.ix = {t: DeviceIndex(self.X[t], self.G[t], metric="mips" if t == "i8" else "Euclidian") for t in self.X}
        rng = np.random.default_rng(77)
        self.labels = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(U32)
        for ix in self.ix.values():
            ix.set_labels(self.labels)
        self.streams = so.independent_streams(_dev())
        self._cache = {}
        self._extra = []

    def queries(self, t, which):
        """which: 0 / 1 = the queries of the first / second call, 2 = the decoys (64 rows)"""
        nq = NQS[which] if which < 2 else NQS[0]
        if t == "i8":
            return (datasets.sift_like(nq, DM, seed=3000 + which, dtype=F32) - 128).clip(-127, 127).astype(np.int8)
        return datasets.sift_like(nq, D, seed=2000 + which, dtype=np.uint8).astype(self.X[t].dtype)

    @staticmethod
    def query_ids(which):
        nq = NQS[which] if which < 2 else NQS[0]
        return np.array([((17, 5, 1)[which] + (331, 77, 1)[which] * i) % N for i in range(nq)], U32)

    def cached(self, key, fn):
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    def sketched(self):
        """the u8 handle with the one-bit Euclidean sketch of the f32 rows attached -> (handle, params, base sketch rows)"""
        def make():
            p = sk.sketch_params(self.ix["f32"], "euclid_bit")
            sk.attach_sketch(self.ix["u8"], self.ix["f32"], p)
            return self.ix["u8"], p, sk.sketch_rows_numpy(self.X["f32"], p)
        return self.cached("sketched", make)

    def rerank_pair(self, mips):
        """(full f32 handle, its one-byte copy, qparams) and a second, idle pair of the same (the host composition runs there)"""
        def make():
            pairs = []
            if mips:
                Xf = self.X["i8"].astype(F32)
                for _ in range(2):
                    full = DeviceIndex(Xf, self.G["i8"], metric="mips")
                    full.normalize()
                    pairs.append(full)
                kind = "mips_i8"
            else:
                pairs = [self.ix["f32"], DeviceIndex(self.X["f32"], self.G["f32"])]
                kind = "euclid_u8"
            quant, qparams = pairs[0].quantized(kind)
            quant2, _ = pairs[1].quantized(kind, params=qparams)
            sp = sk.sketch_params(pairs[0], "mips_2bit" if mips else "euclid_bit")
            sk.attach_sketch(quant, pairs[0], sp)
            sk.attach_sketch(quant2, pairs[1], sp)
            self._extra += [quant, quant2, pairs[1]] + ([pairs[0]] if mips else [])
            return pairs[0], quant, qparams, pairs[1], quant2, sp
        return self.cached(("rerank", mips), make)

    def close(self):
        for ix in list(self.ix.values()) + self._extra:
            ix.close()


@pytest.fixture(scope="module")
def env(oracle):
    e = Env(oracle)
    yield e
    asserted = sorted(h for h in so.HOST_MS if isinstance(h, tuple) and h[1])
    if asserted:                                                   # the figures DELAY_MS is chosen from (visible with -s)
        print(f"\nstream order: {len(so.HOST_MS)} schedules, delay {so.DELAY_MS} ms; host time from 'delay enqueued' to 'entry point "
              f"returned' where returned_early is asserted: median {asserted[len(asserted) // 2][0]:.3f} ms, largest three "
              + ", ".join(f"{h[0]:.3f} ms ({h[2]})" for h in asserted[-3:]))
    e.close()


@pytest.fixture(params=[0, 1], ids=["stream0", "stream1"])
def stream(request, env):
    if len(env.streams) < 2:
        pytest.skip(f"only {len(env.streams)} of torch's first 8 pool streams overtake a delayed stream on this machine: streams "
                    "that share a hardware queue run in submission order and would hide a wrong stream")
    return env.streams[request.param]


# ---- the harness's own control ------------------------------------------------------------------------------------------------

def test_harness_detects_a_wrong_stream(env, stream):
    """a stand-in library (one torch kernel: out = 2 * in) on the OTHER independent stream is reported as wrong; on the right
    stream it passes and reports returned_early"""
    other = env.streams[1 - env.streams.index(stream)]
    real = torch.arange(1, 4097, dtype=torch.int32, device=_dev())
    decoy = torch.full((4096,), 1000000, dtype=torch.int32, device=_dev())
    poisoned = np.full(4096, so.POISON_U32, U32)
    torch.mul(decoy, 2, out=torch.empty_like(decoy))             # the warm-up every case has: the first launch loads the kernel
    torch.cuda.synchronize(_dev())
    for where, right in ((stream, True), (other, False), (torch.cuda.default_stream(_dev()), False)):
        buf, out = decoy.clone(), torch.zeros(4096, dtype=torch.int32, device=_dev())

        def stand_in():
            with torch.cuda.stream(where):
                torch.mul(buf, 2, out=out)
        early = so.run_behind_delay(stream, [(buf, real)], [out], [stand_in])
        torch.cuda.synchronize(_dev())
        got = out.cpu().numpy()
        assert early
        if right:
            np.testing.assert_array_equal(got, 2 * np.arange(1, 4097))
        else:                                     # it ran during the delay: on the decoy, and was poisoned over
            assert np.array_equal(got.view(U32), poisoned) or np.array_equal(got, np.full(4096, 2000000))
            assert not np.array_equal(got, 2 * np.arange(1, 4097))


# ---- searches ---------------------------------------------------------------------------------------------------------------------

def _qp(beam, k=K, limit=N, rf=100):
    return _capi.QueryParams(k=k, beam=beam, cut=1.35, limit=limit, degree_limit=R, rerank_factor=rf, pad=1.0)


def _search_outs(plan, nq, exp, extra=()):
    """SearchOut over fresh outputs, every one of them expected from `exp`; extra: names of further nq-word outputs -> their Outs"""
    o = {f: plan.out((nq, K), F32 if f == "dists" else U32, exp[f], f) for f in ("ids", "dists")}
    for f in SEARCH_FIELDS[2:]:
        o[f] = plan.out((nq,), U32, exp[f], f)
    o["status"] = plan.out((1,), U32, np.zeros(1, U32), "status")
    more = [plan.out((nq,), U32, exp[f], f) for f in extra]
    so_ = _capi.SearchOut(ids=o["ids"].ptr, dists=o["dists"].ptr, out_k=K, frontier_size=o["frontier_size"].ptr,
                          visited_count=o["visited_count"].ptr, dist_cmps=o["dist_cmps"].ptr, degree_sum=o["degree_sum"].ptr,
                          visited_ids=None, visited_dists=None, visited_cap=0, status=o["status"].ptr)
    return so_, more


def _query_inputs(env, plan, t, form, which):
    """late queries or query ids of call `which` -> (d_queries, d_query_ids, stride, keyword for the references)"""
    if form == "ids":
        ids, decoy = env.query_ids(which), env.query_ids(2)[:NQS[which]]
        return None, _vp(plan.late(ids, decoy)), 0, dict(query_ids=ids)
    Q, decoy = env.queries(t, which), env.queries(t, 2)[:NQS[which]]
    return _vp(plan.late(Q, decoy, slack=16)), None, Q.shape[1] * Q.itemsize, dict(queries=Q)


def _starts(plan, nstarts, which):
    s = np.array(STARTS[nstarts][which], U32)
    return _vp(plan.late(s, np.array(DECOY_STARTS[nstarts], U32))), s


@pytest.mark.parametrize("t,beam,form,nstarts", [("u8", 32, "queries", 1), ("f16", 100, "ids", 3), ("f32", 32, "ids", 1),
                                                 ("i8", 100, "queries", 3)])
def test_batch_search_dev(env, stream, t, beam, form, nstarts):
    ix, plan = env.ix[t], Plan()
    for which, nq in enumerate(NQS):
        dq, dqi, stride, qkw = _query_inputs(env, plan, t, form, which)
        dst, starts = _starts(plan, nstarts, which)
        exp = env.cached(("plain", t, beam, form, nstarts, which), lambda: env.o.batch_search(
            env.X[t], env.G[t], k=K, beam=beam, starts=starts, metric=env.metric[t], **qkw))
        out, _ = _search_outs(plan, nq, exp)
        qp = _qp(beam)
        plan.calls.append(lambda s, a=(dq, dqi, nq, stride, dst, nstarts, qp, out): _capi.check(env.lib.pann_batch_search_dev(
            ix.handle, a[0], a[1], a[2], a[3], a[4], a[5], C.byref(a[6]), C.byref(a[7]), _sp(s))))
    _run(stream, plan, label=f"batch_search_dev {t} b{beam} {form}")


@pytest.mark.parametrize("beam,form", [(100, "queries"), (32, "ids")])
def test_batch_search_filtered_dev(env, stream, beam, form):
    """the sketch queries are a late input too"""
    ix, p, S = env.sketched()
    plan = Plan()
    for which, nq in enumerate(NQS):
        dq, dqi, stride, qkw = _query_inputs(env, plan, "u8", form, which)
        dst, starts = _starts(plan, 1, which)
        dsq, sq = None, None
        if form == "queries":
            sq = sk.sketch_rows_numpy(env.queries("f32", which), p)
            dsq = _vp(plan.late(sq, sk.sketch_rows_numpy(env.queries("f32", 2)[:nq], p)))
        exp = env.cached(("filtered", beam, form, which), lambda: filtered_ref.filtered_batch_search(
            env.X["u8"], env.G["u8"], k=K, beam=beam, starts=starts, use_filtering=True, sketches=S, sketch_queries=sq,
            sketch_params=p, **qkw))
        out, (pruned,) = _search_outs(plan, nq, exp, extra=("pruned_cmps",))
        qp = _qp(beam)
        plan.calls.append(lambda s, a=(dq, dqi, nq, stride, dsq, 0 if sq is None else sq.shape[1], dst, qp, out, pruned):
                          _capi.check(env.lib.pann_batch_search_filtered_dev(ix.handle, a[0], a[1], a[2], a[3], a[4], a[5], a[6], 1,
                                                                             C.byref(a[7]), C.byref(a[8]), _vp(a[9]), _sp(s))))
    _run(stream, plan, label=f"batch_search_filtered_dev b{beam} {form}")


def _mask(which, shared):
    """boolean allow mask of call `which`: one shared row, or one row per query (every row another half)"""
    rng = np.random.default_rng(500 + which + (10 if shared else 0))
    m = rng.random(N) < 0.4 if shared else rng.random((NQS[which], N)) < 0.5
    m[..., N - 3:] = (True, False, True)                    # ids in the last bitmap word, both verdicts
    return m


def _packed(m):
    """packed rows with the dead bits of the last word set (they must be ignored)"""
    w = pack_allow(m, N).copy()
    w[..., -1] |= U32((0xFFFFFFFF << (N & 31)) & 0xFFFFFFFF)
    return w


def _masked_ref(env, t, beam, allow, starts, out_k=K, **qkw):
    return masked_ref.masked_batch_search(env.X[t], env.G[t], allow, k=K, beam=beam, starts=starts, metric=env.metric[t],
                                          out_k=out_k, **qkw)


@pytest.mark.parametrize("t,beam,shared", [("f16", 32, False), ("u8", 100, True), ("f32", 32, True), ("i8", 100, False)])
def test_batch_search_masked_dev(env, stream, t, beam, shared):
    ix, plan = env.ix[t], Plan()
    for which, nq in enumerate(NQS):
        dq, dqi, stride, qkw = _query_inputs(env, plan, t, "queries", which)
        dst, starts = _starts(plan, 1, which)
        m = _mask(which, shared)
        dallow = _vp(plan.late(_packed(m), np.zeros_like(_packed(m))))
        exp = env.cached(("masked", t, beam, shared, which), lambda: _masked_ref(env, t, beam, m, starts, **qkw))
        out, (rc, ac) = _search_outs(plan, nq, exp, extra=("result_count", "allowed_cmps"))
        qp = _qp(beam)
        plan.calls.append(lambda s, a=(dq, nq, stride, dst, qp, dallow, 0 if shared else WORDS, out, rc, ac): _capi.check(
            env.lib.pann_batch_search_masked_dev(ix.handle, a[0], None, a[1], a[2], a[3], 1, C.byref(a[4]), a[5], a[6], C.byref(a[7]),
                                                 _vp(a[8]), _vp(a[9]), _sp(s))))
    _run(stream, plan, label=f"batch_search_masked_dev {t} b{beam} {'shared' if shared else 'rows'}")


def _preds(which, shared, decoy=False):
    """(kind name, kind code, predicates uint32 (m, 2)): one "any" predicate for the batch, or a "match" predicate per query"""
    if shared:
        bit = (0x10, 0x400)[which] if not decoy else 0x20
        return "any", _capi.PANN_PRED_ANY, np.array([[bit, 0]], U32)
    shift = (0, 1)[which] if not decoy else 2
    return "match", _capi.PANN_PRED_MATCH, np.array([[0x3, (q + shift) % 4] for q in range(NQS[which])], U32)


def _pred_allow(env, which, shared):
    kind, _, p = _preds(which, shared)
    return label_allow(env.labels, kind, p[0] if shared else p)


@pytest.mark.parametrize("t,beam,shared", [("f16", 32, False), ("u8", 100, True)])
def test_batch_search_labeled_dev(env, stream, t, beam, shared):
    """the predicates are a late input"""
    ix, plan = env.ix[t], Plan()
    for which, nq in enumerate(NQS):
        dq, dqi, stride, qkw = _query_inputs(env, plan, t, "queries", which)
        dst, starts = _starts(plan, 1, which)
        _, kind, p = _preds(which, shared)
        dp = _vp(plan.late(p, _preds(which, shared, decoy=True)[2]))
        exp = env.cached(("labeled", t, beam, shared, which),
                         lambda: _masked_ref(env, t, beam, _pred_allow(env, which, shared), starts, **qkw))
        out, (rc, ac) = _search_outs(plan, nq, exp, extra=("result_count", "allowed_cmps"))
        qp = _qp(beam)
        plan.calls.append(lambda s, a=(dq, nq, stride, dst, qp, kind, dp, len(p), out, rc, ac): _capi.check(
            env.lib.pann_batch_search_labeled_dev(ix.handle, a[0], None, a[1], a[2], a[3], 1, C.byref(a[4]), a[5], a[6], a[7],
                                                  C.byref(a[8]), _vp(a[9]), _vp(a[10]), _sp(s))))
    _run(stream, plan, label=f"batch_search_labeled_dev {t} b{beam} {'shared' if shared else 'per query'}")


# ---- fused quantised search + rerank ----------------------------------------------------------------------------------------------

def _rerank_rows(X, Q, cand, counts, k):
    """exact L2 distances of cand[i, :counts[i]] on integer-valued float rows (float64 is exact there), sorted by (dist, id), k
    kept, padded: what tests/masked_rerank_cases.rerank_rows computes with the oracle's distance"""
    ids, dists = np.full((len(Q), k), SENT, U32), np.full((len(Q), k), np.inf, F32)
    for i in range(len(Q)):
        c = np.asarray(cand[i][:int(counts[i])], U32)
        d = ((X[c].astype(np.float64) - Q[i].astype(np.float64)) ** 2).sum(1).astype(F32)
        order = np.lexsort((c, d))[:k]
        ids[i, :len(order)], dists[i, :len(order)] = c[order], d[order]
    return ids, dists


def _rerank_outs(plan, nq, exp, use_filter=False):
    o = {"ids": plan.out((nq, K), U32, exp["ids"], "ids"), "dists": plan.out((nq, K), F32, exp["dists"], "dists")}
    for f in ("frontier_size", "visited_count", "dist_cmps") + (("pruned_cmps",) if use_filter else ()):
        o[f] = plan.out((nq,), U32, exp[f], f)
    o["status"] = plan.out((1,), U32, np.zeros(1, U32), "status")
    return _capi.RerankOut(ids=o["ids"].ptr, dists=o["dists"].ptr, frontier_size=o["frontier_size"].ptr,
                           visited_count=o["visited_count"].ptr, dist_cmps=o["dist_cmps"].ptr,
                           pruned_cmps=o["pruned_cmps"].ptr if use_filter else None, status=o["status"].ptr)


def _float_queries(env, mips, which):
    return env.queries("i8" if mips else "f32", which).astype(F32)


@pytest.mark.parametrize("mips,beam,use_filter", [(False, 32, False), (False, 100, True), (True, 100, False), (True, 32, True)])
def test_batch_search_rerank_dev(env, stream, mips, beam, use_filter):
    """L2 without the filter: the oracle's search of the u8 rows (the quantiser of integer rows in 0..255 is the identity) and an
    exact rerank in numpy.  With the sketch filter, and on the MIPS table with normalize_first, the existing tests have only the
    composition of the host entry points (quantize_rows, batch_search[_filtered], rerank) to compare with: it runs here on a
    second, idle pair of handles."""
    full, quant, qparams, full2, quant2, sp = env.rerank_pair(mips)
    assert mips or qparams.identity
    plan = Plan()
    for which, nq in enumerate(NQS):
        Q = _float_queries(env, mips, which)
        dq = _vp(plan.late(Q, _float_queries(env, mips, 2)[:nq], slack=16))
        dst, starts = _starts(plan, 1, which)

        def reference():
            if not mips and not use_filter:
                r = env.o.batch_search(env.X["u8"], env.G["u8"], queries=Q.astype(np.uint8), k=K, beam=beam, starts=starts, out_k=beam)
                counts = np.minimum(r["frontier_size"], K * 100)
                r["ids"], r["dists"] = _rerank_rows(env.X["f32"], Q, r["ids"], counts, K)
                return r
            qq = quantize.device_quantize_rows(Q, qparams, normalize_first=mips)
            fq = quantize.normalize_rows(Q) if mips else Q
            if use_filter:
                r = quant2.batch_search_filtered(qq, sk.sketch_rows(fq, sp), k=K, beam=beam, out_k=beam, starts=starts)
            else:
                r = quant2.batch_search(qq, k=K, beam=beam, out_k=beam, starts=starts)
            counts = np.minimum(r["frontier_size"], K * 100).astype(U32)
            r["ids"], r["dists"] = full2.rerank(fq, r["ids"], counts, K, resort=True)
            return r
        exp = env.cached(("rerank", mips, beam, use_filter, which), reference)
        out = _rerank_outs(plan, nq, exp, use_filter)
        qp = _qp(beam)
        plan.calls.append(lambda s, a=(dq, nq, Q.shape[1] * 4, dst, qp, out): _capi.check(env.lib.pann_batch_search_rerank_dev(
            full.handle, quant.handle, C.byref(qparams), a[0], a[1], a[2], 1 if mips else 0, 1 if use_filter else 0, a[3], 1,
            C.byref(a[4]), C.byref(a[5]), _sp(s))))
    _run(stream, plan, label=f"batch_search_rerank_dev {'mips' if mips else 'l2'} b{beam} filter={use_filter}")


@pytest.mark.parametrize("labeled,beam,shared", [(False, 32, False), (False, 100, True), (True, 100, False), (True, 32, True)])
def test_batch_search_masked_and_labeled_rerank_dev(env, stream, labeled, beam, shared):
    """the rule restated on the CPU as tests/masked_rerank_cases.restate does: masked_ref on the u8 rows with a list of
    pool = min(k * rerank_factor, beam, 64) entries, every entry reranked exactly"""
    full, quant, qparams, *_ = env.rerank_pair(False)
    pool = min(K * 100, beam, 64)
    plan = Plan()
    for which, nq in enumerate(NQS):
        Q = _float_queries(env, False, which)
        dq = _vp(plan.late(Q, _float_queries(env, False, 2)[:nq], slack=16))
        dst, starts = _starts(plan, 1, which)
        if labeled:
            _, kind, p = _preds(which, shared)
            dmask = _vp(plan.late(p, _preds(which, shared, decoy=True)[2]))
            m = _pred_allow(env, which, shared)
        else:
            m = _mask(which, shared)
            dmask = _vp(plan.late(_packed(m), np.zeros_like(_packed(m))))

        def reference():
            r = _masked_ref(env, "u8", beam, m, starts, out_k=pool, queries=Q.astype(np.uint8))
            r["ids"], r["dists"] = _rerank_rows(env.X["f32"], Q, r["ids"], r["result_count"], K)
            return r
        exp = env.cached(("masked rerank", labeled, beam, shared, which), reference)
        out = _rerank_outs(plan, nq, exp)
        rc, ac = plan.out((nq,), U32, exp["result_count"], "result_count"), plan.out((nq,), U32, exp["allowed_cmps"], "allowed_cmps")
        qp = _qp(beam)
        if labeled:
            plan.calls.append(lambda s, a=(dq, nq, dst, qp, kind, dmask, len(p), out, rc, ac): _capi.check(
                env.lib.pann_batch_search_labeled_rerank_dev(full.handle, quant.handle, C.byref(qparams), a[0], a[1], D * 4, 0, 0, a[2], 1,
                                                             C.byref(a[3]), a[4], a[5], a[6], C.byref(a[7]), _vp(a[8]), _vp(a[9]),
                                                             _sp(s))))
        else:
            plan.calls.append(lambda s, a=(dq, nq, dst, qp, dmask, 0 if shared else WORDS, out, rc, ac): _capi.check(
                env.lib.pann_batch_search_masked_rerank_dev(full.handle, quant.handle, C.byref(qparams), a[0], a[1], D * 4, 0, 0, a[2], 1,
                                                            C.byref(a[3]), a[4], a[5], C.byref(a[6]), _vp(a[7]), _vp(a[8]), _sp(s))))
    _run(stream, plan, label=f"{'labeled' if labeled else 'masked'}_rerank_dev b{beam} {'shared' if shared else 'per query'}")


# ---- exact kNN under a mask, the counts and the bridge ------------------------------------------------------------------------------

def _knn_rows(which):
    """per-query rows of every density: an empty row, a full one, fewer than k, and random ones from 0.1 % to 90 %"""
    nq = NQS[which]
    rng = np.random.default_rng(900 + which)
    m = rng.random((nq, N)) < np.geomspace(0.001, 0.9, nq)[:, None]
    m[0], m[1] = False, True
    m[2] = False
    m[2, rng.choice(N, K - 1, replace=False)] = True
    return m


@pytest.mark.parametrize("t,labeled,shared", [("i8", False, False), ("u8", False, True), ("f16", True, False), ("f32", True, True)])
def test_bruteforce_knn_masked_and_labeled_dev(env, stream, t, labeled, shared):
    """per-query rows / predicates: no synchronisation.  One shared row or predicate: documented to synchronise the stream once
    (the allowed count sizes the launch), so only the results are asserted"""
    ix, plan = env.ix[t], Plan()
    for which, nq in enumerate(NQS):
        Q = env.queries(t, which)
        dq = _vp(plan.late(Q, env.queries(t, 2)[:nq], slack=16))
        if labeled:
            _, kind, p = _preds(which, shared)
            dmask = _vp(plan.late(p, _preds(which, shared, decoy=True)[2]))
            m = _pred_allow(env, which, shared)
        else:
            m = _mask(which, True) if shared else _knn_rows(which)
            dmask = _vp(plan.late(_packed(m), np.zeros_like(_packed(m))))
        ids, dists, counts = env.cached(("knn", t, labeled, shared, which),
                                        lambda: mkc.reference(env.o, env.X[t], Q, m, K, env.metric[t]))
        o = [plan.out((nq, K), U32, ids, "ids"), plan.out((nq, K), F32, dists, "dists"), plan.out((nq,), U32, counts, "counts")]
        stride = Q.shape[1] * Q.itemsize
        if labeled:
            plan.calls.append(lambda s, a=(dq, nq, stride, kind, dmask, len(p), o): _capi.check(env.lib.pann_bruteforce_knn_labeled_dev(
                ix.handle, a[0], a[1], a[2], K, a[3], a[4], a[5], _vp(a[6][0]), _vp(a[6][1]), _vp(a[6][2]), _sp(s))))
        else:
            plan.calls.append(lambda s, a=(dq, nq, stride, dmask, 0 if shared else WORDS, o): _capi.check(
                env.lib.pann_bruteforce_knn_masked_dev(ix.handle, a[0], a[1], a[2], K, a[3], a[4], _vp(a[5][0]), _vp(a[5][1]),
                                                       _vp(a[5][2]), _sp(s))))
    _run(stream, plan, early=not shared, label=f"bruteforce_knn_{'labeled' if labeled else 'masked'}_dev {t} {'shared' if shared else 'per query'}")


def test_allow_count_dev(env, stream):
    plan = Plan()
    for which, nq in enumerate(NQS):
        m = _knn_rows(which)
        da = _vp(plan.late(_packed(m), np.zeros_like(_packed(m))))
        o = plan.out((nq,), U32, allow_count(m, N).astype(U32), "counts")
        plan.calls.append(lambda s, a=(da, nq, o): _capi.check(env.lib.pann_allow_count_dev(a[0], N, a[1], WORDS, _vp(a[2]), _sp(s))))
    _run(stream, plan, label="allow_count_dev")


@pytest.mark.parametrize("fn", ["labels_to_allow", "label_count"])
def test_label_helpers_dev(env, stream, fn):
    ix, plan = env.ix["u8"], Plan()
    for which, nq in enumerate(NQS):
        _, kind, p = _preds(which, False)
        dp = _vp(plan.late(p, _preds(which, False, decoy=True)[2]))
        m = _pred_allow(env, which, False)
        if fn == "labels_to_allow":
            o = plan.out((nq, WORDS), U32, pack_allow(m, N), "allow")           # bits at positions >= n are written 0
            plan.calls.append(lambda s, a=(kind, dp, nq, o): _capi.check(env.lib.pann_labels_to_allow_dev(
                ix.handle, a[0], a[1], a[2], _vp(a[3]), WORDS, _sp(s))))
        else:
            o = plan.out((nq,), U32, m.sum(1).astype(U32), "counts")
            plan.calls.append(lambda s, a=(kind, dp, nq, o): _capi.check(env.lib.pann_label_count_dev(
                ix.handle, a[0], a[1], a[2], _vp(a[3]), _sp(s))))
    _run(stream, plan, label=f"{fn}_dev")


def test_merge_topk_dev(env, stream):
    """3 lists of k_in = 10 with sentinel-padded short lists, against distributed.merge_topk (numpy)"""
    plan = Plan()
    for which, nq in enumerate(NQS):
        def lists(seed):
            rng = np.random.default_rng(seed)
            ids = rng.integers(0, 1 << 31, (3, nq, K)).astype(U32)
            d = np.sort(rng.integers(0, 50, (3, nq, K)).astype(F32), axis=2)           # many ties: the id decides
            ids[0, ::5, K - 1], d[0, ::5, K - 1] = SENT, np.inf
            ids[2, 1::4, 3:], d[2, 1::4, 3:] = SENT, np.inf
            return ids, d
        (ids, d), (ids0, d0) = lists(40 + which), lists(50 + which)
        di, dd = _vp(plan.late(ids, ids0)), _vp(plan.late(d, d0))
        ei, ed = dist.merge_topk(ids, d, K)
        oi, od = plan.out((nq, K), U32, ei, "ids"), plan.out((nq, K), F32, ed, "dists")
        plan.calls.append(lambda s, a=(di, dd, nq, oi, od): _capi.check(env.lib.pann_merge_topk_dev(
            a[0], a[1], 3, a[2], K, K, None, K, _vp(a[3]), _vp(a[4]), _sp(s))))
    _run(stream, plan, label="merge_topk_dev")


# ---- quantiser and sketches -------------------------------------------------------------------------------------------------------

def _quant_rows(which):
    """float rows with fractions of every sign (64 or 37 rows of 100 floats): the roundings and both clamps are exercised"""
    rng = np.random.default_rng(700 + which)
    return (rng.standard_normal((NQS[which] if which < 2 else NQS[0], DM)) * 90 + 20).astype(F32)


def _quantised_numpy(x, kind, normalize_first):
    """the numpy quantiser of parlayann_amd/quantize.py -> (QuantParams for the device, expected rows)"""
    if normalize_first:
        x = quantize.normalize_rows(x)
    if kind == "euclid_u8":
        p = quantize.EuclidParams(-300.0, 350.0, DM)
        return quantize.device_params(kind, DM, slope=p.slope, offset=p.offset), quantize.euclid_u8_translate(x, p)
    mv = F32(0.25 if normalize_first else 200.0)
    return quantize.device_params(kind, DM, max_val=mv), quantize.mips_i8_translate(x, mv)


@pytest.mark.parametrize("kind,normalize_first", [("euclid_u8", False), ("mips_i8", False), ("mips_i8", True)])
def test_quantize_rows_dev(env, stream, kind, normalize_first):
    plan = Plan()
    for which, nq in enumerate(NQS):
        x = _quant_rows(which)
        p, exp = _quantised_numpy(x, kind, normalize_first)
        dx = _vp(plan.late(x, _quant_rows(2)[:nq]))
        o = plan.out((nq, DM), np.uint8, exp.view(np.uint8), "rows")
        plan.calls.append(lambda s, a=(p, dx, nq, o): _capi.check(env.lib.pann_quantize_rows_dev(
            C.byref(a[0]), a[1], a[2], DM * 4, 1 if normalize_first else 0, _vp(a[3]), DM, _sp(s))))
    _run(stream, plan, label=f"quantize_rows_dev {kind} normalize={normalize_first}")


def test_quantize_params_dev(env, stream):
    """documented to synchronise the stream (a handful of words come back before the parameters can be formed): only the results
    are asserted, against the numpy generate_parameters of parlayann_amd/quantize.py"""
    plan = Plan()
    got = [_capi.QuantParams(), _capi.QuantParams()]
    xs = [_quant_rows(0), np.abs(_quant_rows(1))]
    for which, nq in enumerate(NQS):
        dx = _vp(plan.late(xs[which], _quant_rows(2)[:nq] * F32(0.5)))
        kind = (_capi.PANN_QUANT_MIPS_I8, _capi.PANN_QUANT_EUCLID_U8)[which]
        plan.calls.append(lambda s, a=(dx, nq, kind, got[which]): _capi.check(env.lib.pann_quantize_params_dev(
            a[0], a[1], DM, DM * 4, a[2], 1, C.byref(a[3]), _sp(s))))
    _run(stream, plan, early=False, label="quantize_params_dev")
    assert F32(got[0].max_val) == quantize.mips_i8_max_val(xs[0], trim=True)
    e = quantize.euclid_u8_params(xs[1])
    assert (F32(got[1].slope), int(got[1].offset)) == (e.slope, int(e.offset))


@pytest.mark.parametrize("kind", ["euclid_bit", "mips_2bit"])
def test_sketch_rows_dev(env, stream, kind):
    """against the numpy packer of parlayann_amd/sketch.py, the reference of tests/test_sketch_gpu.py"""
    p = sk.make_params(kind, DM, median=20, cut=35.0)
    rb = sk.row_bytes(kind, DM)
    plan = Plan()
    for which, nq in enumerate(NQS):
        x = _quant_rows(which)
        dx = _vp(plan.late(x, _quant_rows(2)[:nq]))
        o = plan.out((nq, rb), np.uint8, sk.sketch_rows_numpy(x, p), "sketch rows")
        plan.calls.append(lambda s, a=(dx, nq, o): _capi.check(env.lib.pann_sketch_rows_dev(
            C.byref(p), a[0], a[1], DM * 4, _vp(a[2]), rb, _sp(s))))
    _run(stream, plan, label=f"sketch_rows_dev {kind}")


# ---- chains: producer and consumer with no host step between them -----------------------------------------------------------------

def test_chain_labels_to_allow_into_masked_search(env, stream):
    ix, plan = env.ix["f16"], Plan()
    beam = 32
    for which, nq in enumerate(NQS):
        dq, _, stride, qkw = _query_inputs(env, plan, "f16", "queries", which)
        dst, starts = _starts(plan, 1, which)
        _, kind, p = _preds(which, False)
        dp = _vp(plan.late(p, _preds(which, False, decoy=True)[2]))
        allow = plan.out((nq, WORDS), U32)                       # the intermediate: poisoned like an output (any bits are a valid bitmap)
        exp = env.cached(("labeled", "f16", beam, False, which),
                         lambda: _masked_ref(env, "f16", beam, _pred_allow(env, which, False), starts, **qkw))
        out, (rc, ac) = _search_outs(plan, nq, exp, extra=("result_count", "allowed_cmps"))
        qp = _qp(beam)

        def call(s, a=(kind, dp, nq, allow, dq, stride, dst, qp, out, rc, ac)):
            _capi.check(env.lib.pann_labels_to_allow_dev(ix.handle, a[0], a[1], a[2], _vp(a[3]), WORDS, _sp(s)))
            _capi.check(env.lib.pann_batch_search_masked_dev(ix.handle, a[4], None, a[2], a[5], a[6], 1, C.byref(a[7]), _vp(a[3]), WORDS,
                                                             C.byref(a[8]), _vp(a[9]), _vp(a[10]), _sp(s)))
        plan.calls.append(call)
    _run(stream, plan, label="labels_to_allow_dev -> batch_search_masked_dev")


def test_chain_quantize_rows_into_search(env, stream):
    """float queries -> pann_quantize_rows_dev -> pann_batch_search_dev on the one-byte copy of the f32 handle (integer rows in
    0..255: the quantiser is the identity, the copy holds the u8 table, and the oracle's search of it is the reference)"""
    _, quant, qparams, *_ = env.rerank_pair(False)
    plan, beam = Plan(), 100
    for which, nq in enumerate(NQS):
        Q = _float_queries(env, False, which)
        dq = _vp(plan.late(Q, _float_queries(env, False, 2)[:nq]))
        dst, starts = _starts(plan, 1, which)
        rows = plan.out((nq * D + 16,), np.uint8)                # the intermediate (any bytes are valid rows) + the read slack
        exp = env.cached(("plain", "u8", beam, "queries", 1, which), lambda: env.o.batch_search(
            env.X["u8"], env.G["u8"], queries=Q.astype(np.uint8), k=K, beam=beam, starts=starts))
        out, _ = _search_outs(plan, nq, exp)
        qp = _qp(beam)

        def call(s, a=(dq, nq, rows, dst, qp, out)):
            _capi.check(env.lib.pann_quantize_rows_dev(C.byref(qparams), a[0], a[1], D * 4, 0, _vp(a[2]), D, _sp(s)))
            _capi.check(env.lib.pann_batch_search_dev(quant.handle, _vp(a[2]), None, a[1], D, a[3], 1, C.byref(a[4]), C.byref(a[5]), _sp(s)))
        plan.calls.append(call)
    _run(stream, plan, label="quantize_rows_dev -> batch_search_dev")


def test_chain_sketch_rows_into_filtered_search(env, stream):
    ix, p, S = env.sketched()
    rb = sk.row_bytes("euclid_bit", D)
    plan, beam = Plan(), 100
    for which, nq in enumerate(NQS):
        dq, _, stride, qkw = _query_inputs(env, plan, "u8", "queries", which)
        Qf = env.queries("f32", which)
        dqf = _vp(plan.late(Qf, env.queries("f32", 2)[:nq]))
        dst, starts = _starts(plan, 1, which)
        sq = plan.out((nq, rb), np.uint8)                        # the intermediate (any bits are valid sketches)
        exp = env.cached(("filtered", beam, "queries", which), lambda: filtered_ref.filtered_batch_search(
            env.X["u8"], env.G["u8"], k=K, beam=beam, starts=starts, use_filtering=True, sketches=S,
            sketch_queries=sk.sketch_rows_numpy(Qf, p), sketch_params=p, **qkw))
        out, (pruned,) = _search_outs(plan, nq, exp, extra=("pruned_cmps",))
        qp = _qp(beam)

        def call(s, a=(dqf, nq, sq, dq, stride, dst, qp, out, pruned)):
            _capi.check(env.lib.pann_sketch_rows_dev(C.byref(p), a[0], a[1], D * 4, _vp(a[2]), rb, _sp(s)))
            _capi.check(env.lib.pann_batch_search_filtered_dev(ix.handle, a[3], None, a[1], a[4], _vp(a[2]), rb, a[5], 1, C.byref(a[6]),
                                                               C.byref(a[7]), _vp(a[8]), _sp(s)))
        plan.calls.append(call)
    _run(stream, plan, label="sketch_rows_dev -> batch_search_filtered_dev")


# ---- entries that run on the handle's stream (pann_index_set_stream) --------------------------------------------------------------

class _on_stream:
    """the handle on the caller's stream for the duration; the private stream is restored whatever happens"""

    def __init__(self, ix, stream):
        self.ix, self.stream = ix, stream

    def __enter__(self):
        self.ix.set_stream(self.stream.cuda_stream)

    def __exit__(self, *exc):
        self.ix.set_stream(0, private=True)


def test_set_labels_dev_then_labeled_search(env, stream):
    """pann_index_set_labels_dev (handle stream, no synchronisation) followed at once by pann_batch_search_labeled_dev on the same
    stream: the labels are a late input, and both calls must come back while the delay runs"""
    ix = DeviceIndex(env.X["u8"], env.G["u8"])
    other_labels = np.random.default_rng(78).integers(0, 1 << 32, N, dtype=np.uint64).astype(U32)
    try:
        ix.set_labels(other_labels)                              # the label array exists: set_labels_dev allocates nothing
        plan, beam, nq = Plan(), 32, NQS[0]
        dl = _vp(plan.late(env.labels, other_labels))
        dq, _, stride, qkw = _query_inputs(env, plan, "u8", "queries", 0)
        dst, starts = _starts(plan, 1, 0)
        _, kind, p = _preds(0, False)
        dp = _vp(plan.late(p, _preds(0, False, decoy=True)[2]))
        exp = env.cached(("labeled", "u8", beam, False, 0), lambda: _masked_ref(env, "u8", beam, _pred_allow(env, 0, False), starts, **qkw))
        out, (rc, ac) = _search_outs(plan, nq, exp, extra=("result_count", "allowed_cmps"))
        qp = _qp(beam)

        def call(s):
            _capi.check(env.lib.pann_index_set_labels_dev(ix.handle, 0, dl, N))
            _capi.check(env.lib.pann_batch_search_labeled_dev(ix.handle, dq, None, nq, stride, dst, 1, C.byref(qp), kind, dp, nq,
                                                              C.byref(out), _vp(rc), _vp(ac), _sp(s)))
        plan.calls.append(call)
        plan.after_warm_up = lambda: ix.set_labels(other_labels)
        with _on_stream(ix, stream):
            _run(stream, plan, label="set_labels_dev -> batch_search_labeled_dev")
        np.testing.assert_array_equal(ix.labels(), env.labels)
    finally:
        ix.close()


def _fill(o, word):
    """a poison of the caller's choice for words that a later kernel uses as ids: 0xFFFFFFFF is the empty slot, never an index"""
    o.t.view(torch.int32).fill_(word)


def test_vamana_phases_on_the_handle_stream(env, stream):
    """pann_vamana_search_prune_dev + pann_vamana_apply_rows_dev, one batch of 200 ids (late), the rows handed from A to B on the
    stream: the graph equals oracle.vamana_insert_batch.  Both return after the stream has drained: only results are asserted"""
    X, G = env.X["u8"], env.G["u8"]
    ids = np.random.default_rng(31).choice(np.arange(1, N), 200, replace=False).astype(U32)
    decoy = np.random.default_rng(32).choice(np.arange(1, N), 200, replace=False).astype(U32)
    want = G.copy()
    env.o.vamana_insert_batch(X, want, ids, R, L, 1.2)
    rows_want = env.o.vamana_phase_a(X, G, ids, R, L, 1.2)
    ix = DeviceIndex(X, G)
    try:
        plan = Plan()
        dids = plan.late(ids, decoy)
        rows = Out((200, R), U32)                                 # A's output and B's input: pre-set to empty rows, not to poison
        plan.want("rows", rows, rows_want)

        def call(s):
            with torch.cuda.stream(s):
                _fill(rows, -1)                                   # behind the delay: rows written ahead of it would be lost
            ix.vamana_search_prune_dev(dids.data_ptr(), 200, R, L, 1.2, rows.ptr)
            ix.vamana_apply_rows_dev(dids.data_ptr(), 200, rows.ptr, R, 1.2)
        plan.calls.append(call)
        plan.after_warm_up = lambda: ix.set_graph(G)
        with _on_stream(ix, stream):
            _run(stream, plan, early=False, label="vamana_search_prune_dev -> vamana_apply_rows_dev")
        np.testing.assert_array_equal(tp.norm(ix.get_graph()), tp.norm(want))
    finally:
        ix.close()


def test_vamana_delete_batch_dev_on_the_handle_stream(env, stream):
    X, G = env.X["u8"], env.G["u8"]
    ids = np.random.default_rng(41).choice(np.arange(1, N), 100, replace=False).astype(U32)
    decoy = np.random.default_rng(42).choice(np.arange(1, N), 100, replace=False).astype(U32)
    want, _ = dr.delete_ref(env.o, X, G, ids, 1.2, R)
    ix = DeviceIndex(X, G)
    try:
        plan = Plan()
        dids = plan.late(ids, decoy)
        plan.calls.append(lambda s: ix.vamana_delete_batch_dev(dids.data_ptr(), 100, R, 1.2))
        plan.after_warm_up = lambda: ix.set_graph(G)
        with _on_stream(ix, stream):
            _run(stream, plan, early=False, label="vamana_delete_batch_dev")
        np.testing.assert_array_equal(ix.get_graph(), want)
    finally:
        ix.close()


def test_hcnng_phases_on_the_handle_stream(env, stream):
    """pann_hcnng_build_trees_dev + pann_hcnng_assemble_dev: 2 trees, cluster size 100, the slab handed over on the stream; slab
    and graph against the oracle as in tests/test_two_phase_build_gpu.py"""
    X, T, cs = env.X["u8"], 2, 100
    stride = T * tp.MST_DEG
    ix = DeviceIndex(X, max_degree=stride)
    try:
        plan = Plan()
        slab = plan.out((N, stride), U32, tp.oracle_tree_slabs(env.o, X, T, cs, tp.MST_DEG, tp.HCNNG_SEED, 1)[0], "slab")

        def call(s):
            _capi.check(env.lib.pann_hcnng_build_trees_dev(ix.handle, 0, 1, T, cs, tp.MST_DEG, tp.HCNNG_SEED, _vp(slab), stride, None))
            _capi.check(env.lib.pann_hcnng_assemble_dev(ix.handle, _vp(slab), 1, stride, T, tp.MST_DEG))
        plan.calls.append(call)
        plan.after_warm_up = ix.clear_graph
        with _on_stream(ix, stream):
            _run(stream, plan, early=False, label="hcnng_build_trees_dev -> hcnng_assemble_dev")
        np.testing.assert_array_equal(ix.get_graph(), env.o.hcnng_build(X, T, cs, tp.MST_DEG, seed=tp.HCNNG_SEED))
    finally:
        ix.close()
