"""The two seams of the multi-GPU builds, phase by phase against the oracle in ONE process on ONE GPU:

  pann_vamana_search_prune_dev (phase A) / pann_vamana_apply_rows_dev (phase B)   -- distributed.device_vamana_build_sharded
  pann_hcnng_build_trees_dev / pann_hcnng_assemble_dev                            -- distributed.device_hcnng_build_tree_parallel

W ranks are played by calling phase A on the W slices of every batch (and build_trees once per rank); the all-gather is the
pad-and-cut of distributed.all_gather_rows without the collective.  After EVERY batch the m x R words phase A wrote (padding
included, into a buffer prefilled with POISON) and the graph phase B left are compared with the oracle's on the same graph
state, so a mismatch names a batch and a phase.  tests/two_phase_cases.py holds the cases and the oracle-side drivers,
tests/test_two_phase_cases_cpu.py shows on the CPU that they contain what they are there for.  tests/test_sharded_gpu.py keeps
covering the real collective.  Integer-valued data: every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import two_phase_cases as tp
from parlayann_amd import DeviceIndex, _capi, datasets

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
BAD_ARG = _capi.PANN_ERR_BAD_ARG
_single = {}


def _dev():
    return torch.device("cuda", 0)


def _to_dev(a):
    """uint32 numpy array -> int32 device tensor of the same bits"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(_dev())


def _to_host(t):
    return t.cpu().numpy().view(np.uint32)


def _stats(n):
    st = _capi.BuildStats()
    vis, dc = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    st.per_point_visited = vis.ctypes.data_as(C.c_void_p)
    st.per_point_dist_cmps = dc.ctypes.data_as(C.c_void_p)
    return st, vis, dc


def _sync(side):
    """the handle runs on its own stream unless it was given the caller's: torch's work on the ids and rows must have finished
    before a phase reads them.  On the caller's stream the order of the stream is enough (no host synchronisation)."""
    if side is None:
        torch.cuda.synchronize()


def _phase_a(ix, ids, W, R, L, a, start, stats, side=None):
    """phase A on the W slices of the batch, into ONE [m, R] tensor prefilled with POISON"""
    m = ids.numel()
    rows = torch.full((m, R), POISON, dtype=torch.int32, device=ids.device)
    _sync(side)
    for s0, s1 in tp.slices(m, W):
        if s1 > s0:
            ix.vamana_search_prune_dev(ids[s0:s1].data_ptr(), s1 - s0, R, L, a, rows[s0:s1].data_ptr(), start=start, stats=stats)
    return rows


def _gather(rows, W):
    """what distributed.all_gather_rows hands to phase B: every rank's block padded to `per` rows of -1, concatenated, cut to m"""
    m, R = rows.shape
    per = (m + W - 1) // W
    blocks = []
    for s0, s1 in tp.slices(m, W):
        blk = rows[s0:s1]
        if s1 - s0 < per:
            blk = torch.cat([blk, torch.full((per - (s1 - s0), R), -1, dtype=rows.dtype, device=rows.device)], 0)
        blocks.append(blk)
    return torch.cat(blocks, 0)[:m].contiguous()


def _phase_b(ix, ids, rows, R, a, stats, side=None):
    _sync(side)
    ix.vamana_apply_rows_dev(ids.data_ptr(), ids.numel(), rows.data_ptr(), R, a, stats=stats)


def _drive(oracle, ix, name, W, start=0, stats=None, mix=None, side=None, every_batch=True):
    """The build of a case as W ranks, on the device, in step with tp.oracle_two_phase_build.
    mix = None         : device A, device B; rows and graphs compared with the oracle's after every batch of the first pass
    mix = "oracle_rows": device B on the ORACLE's rows (no device A)
    mix = "device_rows": device A and B; the ORACLE's phase B applies the DEVICE's rows to its own graph
    Returns the oracle's graph before the final sort (the device's is still unsorted too)."""
    X, metric, R, max_deg, L, alpha, passes, _ = tp.vamana_case(name)
    sched = tp.schedule(len(X), tp.SEED, passes, alpha)
    nfirst = len(sched) // passes
    d_perm = _to_dev(np.concatenate([ids for ids, _ in sched[:nfirst]]))
    ref = tp.oracle_two_phase_build(oracle, X, R, L, alpha, passes, tp.SEED, W, metric, max_degree=max_deg, start=start)
    Gmix = np.zeros((len(X), max_deg + 1), np.uint32)
    lo = 0
    for b, (h_ids, a) in enumerate(sched):
        m = len(h_ids)
        if b % nfirst == 0:
            lo = 0
        ids = d_perm[lo:lo + m].clone()                    # made by a torch kernel, as device_vamana_build_sharded's slices are
        lo += m
        o_ids, o_rows, o_G = next(ref)
        assert np.array_equal(o_ids, h_ids)
        if mix == "oracle_rows":
            rows = _to_dev(o_rows)
        else:
            rows = _phase_a(ix, ids, W, R, L, a, start, stats, side)
            if mix is None and (every_batch or b == len(sched) - 1):
                np.testing.assert_array_equal(_to_host(rows), o_rows, err_msg=f"phase A rows of batch {b} (m = {m})")
        _phase_b(ix, ids, _gather(rows, W), R, a, stats, side)
        if mix == "device_rows":
            oracle.vamana_phase_b(X, Gmix, h_ids, _to_host(rows), R, a, metric=metric)
            o_G = Gmix
        if (every_batch and b < nfirst) or b == len(sched) - 1:
            np.testing.assert_array_equal(tp.norm(ix.get_graph()), tp.norm(o_G), err_msg=f"graph after batch {b} (m = {m})")
    return o_G


def _single_handle_build(name):
    """(BuildStats, per-point visited, per-point comparisons) of pann_vamana_build on a handle of its own, once per case"""
    if name not in _single:
        X, metric, R, max_deg, L, alpha, passes, _ = tp.vamana_case(name)
        ix = DeviceIndex(X, max_degree=max_deg, metric=metric)
        ps = (np.zeros(len(X), np.uint32), np.zeros(len(X), np.uint32))
        st = ix.vamana_build(R, L, alpha, num_passes=passes, seed=tp.SEED, point_stats=ps)
        ix.close()
        _single[name] = (st.search_dist_cmps, st.prune_dist_cmps, st.visited_total, ps[0], ps[1])
    return _single[name]


def _check_code_searches(oracle, ix, X, metric):
    """beam-100 searches go through the filter codes when they are valid: a code phase B forgot changes dist_cmps first"""
    G = ix.get_graph()
    qids = np.arange(0, len(X), 13, dtype=np.uint32)
    g = ix.batch_search(query_ids=qids, k=10, beam=100)
    o = oracle.batch_search(X, G, query_ids=qids, k=10, beam=100, metric=metric)
    for f in ("ids", "dists", "dist_cmps", "visited_count"):
        np.testing.assert_array_equal(g[f], o[f], err_msg=f)


@pytest.mark.parametrize("name,W", tp.VAMANA_PAIRS, ids=[f"{a}-W{b}" for a, b in tp.VAMANA_PAIRS])
def test_two_phase_build_equals_oracle_batch_by_batch(oracle, name, W):
    X, metric, R, max_deg, L, alpha, passes, _ = tp.vamana_case(name)
    ix = DeviceIndex(X, max_degree=max_deg, metric=metric)
    st, vis, dc = _stats(len(X))
    try:
        _drive(oracle, ix, name, W, stats=st)
        if name in tp.CODE_CASES:
            assert ix.get_option("filter_codes") == 1             # maintained by phase B, not dropped
            _check_code_searches(oracle, ix, X, metric)
        ix.vamana_sort_neighbors()
        Go, so, (ovis, odc) = tp.vamana_oracle_build(oracle, name)
        np.testing.assert_array_equal(tp.norm(ix.get_graph()), tp.norm(Go))
        # the split calls add up to the single-call build's statistics, whatever W; and to the oracle's
        s_search, s_prune, s_vis, p_vis, p_dc = _single_handle_build(name)
        assert (st.search_dist_cmps, st.prune_dist_cmps, st.visited_total) == (s_search, s_prune, s_vis)
        np.testing.assert_array_equal(vis, p_vis)
        np.testing.assert_array_equal(dc, p_dc)
        assert (st.search_dist_cmps, st.prune_dist_cmps, st.visited_total) == (int(so[0]), int(so[1]), int(so[2]))
        np.testing.assert_array_equal(vis, ovis)
        np.testing.assert_array_equal(dc, odc)
    finally:
        ix.close()


def test_filter_codes_switched_off_give_the_same_graph(oracle):
    name, W = "f16_L100", 3
    X, metric, *_ = tp.vamana_case(name)
    ix = DeviceIndex(X, max_degree=32, metric=metric)
    ix.set_option("filter_codes", 0)
    try:
        _drive(oracle, ix, name, W)
        assert ix.get_option("filter_codes") == 0
        _check_code_searches(oracle, ix, X, metric)
        ix.vamana_sort_neighbors()
        np.testing.assert_array_equal(tp.norm(ix.get_graph()), tp.norm(tp.vamana_oracle_build(oracle, name)[0]))
    finally:
        ix.close()


@pytest.mark.parametrize("name,W,mix", [("u8_L48", 2, "oracle_rows"), ("f16_L100", 3, "device_rows")])
def test_phases_mixed_with_the_oracle(oracle, name, W, mix):
    """device B on the oracle's rows, and the oracle's B on the device's rows: a pair of errors in A and B that cancel on the
    device cannot survive both"""
    X, metric, R, max_deg, *_ = tp.vamana_case(name)
    ix = DeviceIndex(X, max_degree=max_deg, metric=metric)
    try:
        _drive(oracle, ix, name, W, mix=mix)
        ix.vamana_sort_neighbors()
        np.testing.assert_array_equal(tp.norm(ix.get_graph()), tp.norm(tp.vamana_oracle_build(oracle, name)[0]))
    finally:
        ix.close()


def test_start_other_than_zero(oracle):
    name = "i8_L70"
    X, metric, R, max_deg, *_ = tp.vamana_case(name)
    ix = DeviceIndex(X, max_degree=max_deg, metric=metric)
    try:
        Go = _drive(oracle, ix, name, 3, start=5)
        assert not np.array_equal(tp.norm(Go), tp.norm(tp.vamana_oracle_build(oracle, name, sort_neighbors=False)[0]))
    finally:
        ix.close()


def test_on_the_callers_stream(oracle):
    """the handle on torch's side stream: ids cloned by a torch kernel on that stream, phases, pad-and-cut, all ordered by the
    stream alone (no host synchronisation between torch's kernels and the phases), as device_vamana_build_sharded runs them"""
    name, W = "u8_L48", 3
    X, metric, R, max_deg, *_ = tp.vamana_case(name)
    ix = DeviceIndex(X, max_degree=max_deg, metric=metric)
    side = torch.cuda.Stream(device=_dev())
    try:
        with torch.cuda.stream(side):
            ix.set_stream(side.cuda_stream)
            try:
                _drive(oracle, ix, name, W, side=side, every_batch=False)
            finally:
                ix.set_stream(0, private=True)
        ix.vamana_sort_neighbors()
        np.testing.assert_array_equal(tp.norm(ix.get_graph()), tp.norm(tp.vamana_oracle_build(oracle, name)[0]))
    finally:
        ix.close()


@pytest.mark.parametrize("locality", [0, 2])
def test_full_wide_rows_and_launch_order(oracle, locality):
    """ONE batch of 500 ids on the oracle's finished R = 96 graph at L = 200, three slices of 167, 167 and 166 ids:
    - rows of 96 picks, which the one-pass R = 96 build never produces (tests/test_two_phase_cases_cpu.py);
    - locality_order = 2 launches the searches of a call of 64 ids or more sorted by locality cell.  No batch of the n = 3000
      schedule is that long (the longest has 60 ids).  Row i of a slice must still belong to id i of the slice: the rows of this
      batch are pairwise different, so a row left at its launch slot is seen."""
    W = 3
    X, metric, G, h_ids, want, R, L, alpha = tp.full_wide_batch(oracle)
    ix = DeviceIndex(X, G, metric=metric)
    ix.set_option("locality_order", locality)
    try:
        ids = _to_dev(h_ids)
        rows = _phase_a(ix, ids, W, R, L, alpha, 0, None)
        assert ix.get_option("locality_order") == (1 if locality else 0)      # 1: the cells exist, the launches were reordered
        np.testing.assert_array_equal(_to_host(rows), want)
        _phase_b(ix, ids, _gather(rows, W), R, alpha, None)
        oracle.vamana_phase_b(X, G, h_ids, want, R, alpha, metric=metric)
        np.testing.assert_array_equal(tp.norm(ix.get_graph()), tp.norm(G))
    finally:
        ix.close()


# ---- HCNNG -------------------------------------------------------------------------------------------------------------------

def _build_slabs(ix, T, cs, W, stride, seed=tp.HCNNG_SEED):
    """every rank's build_trees call into its slab of ONE [W, n, stride] tensor prefilled with POISON"""
    slabs = torch.full((W, ix.n, stride), POISON, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    for r in range(W):
        _capi.check(ix._lib.pann_hcnng_build_trees_dev(ix.handle, r, W, len(range(r, T, W)), cs, tp.MST_DEG, seed,
                                                       C.c_void_p(slabs[r].data_ptr()), stride, None))
    return slabs


def _assemble(ix, slabs, T):
    W, _, stride = slabs.shape
    _capi.check(ix._lib.pann_hcnng_assemble_dev(ix.handle, C.c_void_p(slabs.data_ptr()), W, stride, T, tp.MST_DEG))


@pytest.mark.parametrize("name,W,forest", tp.HCNNG_TRIPLES, ids=[f"{a}-W{b}-{f[0]}x{f[1]}" for a, b, f in tp.HCNNG_TRIPLES])
def test_tree_slabs_and_assembly_equal_oracle(oracle, name, W, forest):
    T, cs = forest
    X, metric = tp.hcnng_points(name)
    ix = DeviceIndex(X, max_degree=T * tp.MST_DEG, metric=metric)
    try:
        empty = ix.get_graph()
        assert not empty.any()
        for stride in (tp.slab_stride(T, W, tp.MST_DEG), tp.slab_stride(T, W, tp.MST_DEG) + 5):
            slabs = _build_slabs(ix, T, cs, W, stride)
            want = tp.oracle_tree_slabs(oracle, X, T, cs, tp.MST_DEG, tp.HCNNG_SEED, W, metric, stride=stride)
            np.testing.assert_array_equal(_to_host(slabs), want, err_msg=f"stride {stride}")
            np.testing.assert_array_equal(ix.get_graph(), empty)          # build_trees does not touch the handle's graph
        _assemble(ix, slabs, T)                                            # (the slabs with 5 spare columns per row)
        np.testing.assert_array_equal(ix.get_graph(), oracle.hcnng_build(X, T, cs, tp.MST_DEG, seed=tp.HCNNG_SEED, metric=metric))
    finally:
        ix.close()


def test_forest_group_does_not_change_the_slabs(oracle):
    (T, cs), W = tp.HCNNG_FORESTS[1], 2
    X, metric = tp.hcnng_points("u8")
    want = tp.oracle_tree_slabs(oracle, X, T, cs, tp.MST_DEG, tp.HCNNG_SEED, W, metric)
    ix = DeviceIndex(X, max_degree=T * tp.MST_DEG)
    try:
        for group in (1, 0):                                               # one tree per forest pass; all of the call's trees together
            ix.set_option("forest_group", group)
            np.testing.assert_array_equal(_to_host(_build_slabs(ix, T, cs, W, want.shape[2])), want, err_msg=f"forest_group {group}")
    finally:
        ix.close()


@pytest.mark.parametrize("room", ["for_both", "rows_fill_up"])
def test_assemble_appends_after_the_current_neighbours(oracle, room):
    """a second forest assembled onto a handle that holds a first one: current neighbours first, then the trees in order.  With
    max_deg below the sum of both (rows_fill_up) a row takes edges while it has room and stops at max_deg -- the kernel bounds
    every store by max_deg, the row's stride is never passed -- exactly as the oracle's initial-graph entry does."""
    X, metric = tp.hcnng_points("u8")
    (T1, cs1), (T2, cs2) = tp.HCNNG_FORESTS[1], tp.HCNNG_FORESTS[0]
    max_deg = (T1 + T2) * tp.MST_DEG if room == "for_both" else T1 * tp.MST_DEG + 2
    ix = DeviceIndex(X, max_degree=max_deg)
    try:
        ix.hcnng_build(T1, cs1, tp.MST_DEG, seed=tp.HCNNG_SEED)
        first = ix.get_graph()
        np.testing.assert_array_equal(first[:, :T1 * tp.MST_DEG + 1], oracle.hcnng_build(X, T1, cs1, tp.MST_DEG, seed=tp.HCNNG_SEED))
        slabs = _build_slabs(ix, T2, cs2, 2, tp.slab_stride(T2, 2, tp.MST_DEG), seed=tp.HCNNG_SEED + 100)
        np.testing.assert_array_equal(ix.get_graph(), first)
        _assemble(ix, slabs, T2)
        want = tp.wide_cases.hcnng_oracle_append(X, first.copy(), T2, cs2, tp.MST_DEG, tp.HCNNG_SEED + 100, oracle=oracle)
        got = ix.get_graph()
        np.testing.assert_array_equal(got, want)
        assert got[:, 0].max() <= max_deg and (got[:, 0] > first[:, 0]).any()
        if room == "rows_fill_up":
            assert (got[:, 0] == max_deg).sum() >= 100
    finally:
        ix.close()


# ---- argument checks ------------------------------------------------------------------------------------------------------------

def test_statuses(oracle):
    """every refusal returns its code with a message of its own and leaves the graph and the output buffers as they were"""
    lib = _capi.load()
    n, d, max_deg, R, L, m = 1000, 32, 16, 16, 32, 8
    X = datasets.sift_like(n, d, seed=3)
    ix = DeviceIndex(X, max_degree=max_deg)
    try:
        ix.vamana_build(R, L, 1.2, num_passes=1, seed=5)
        G = ix.get_graph()
        h = ix.handle
        ids = _to_dev(np.arange(10, 10 + m, dtype=np.uint32))
        rows = torch.full((m, 2 * R), POISON, dtype=torch.int32, device=_dev())       # room for the R > max_deg calls too
        slab = torch.full((n, 8), POISON, dtype=torch.int32, device=_dev())
        torch.cuda.synchronize()
        p = lambda t: C.c_void_p(t.data_ptr())

        def refused(what, fn, code=BAD_ARG):
            assert lib.pann_index_set_option(h, b"no-such-option", 0) == 1              # last error := another text
            rc = fn()
            msg = lib.pann_last_error().decode()
            assert rc == code and msg and "no-such-option" not in msg, (what, rc, msg)
            assert (_to_host(rows) == POISON).all() and (_to_host(slab) == POISON).all(), what
            np.testing.assert_array_equal(ix.get_graph(), G, err_msg=what)

        A, B = lib.pann_vamana_search_prune_dev, lib.pann_vamana_apply_rows_dev
        refused("A: null ids", lambda: A(h, None, m, 0, R, L, 1.2, p(rows), None))
        refused("A: null rows", lambda: A(h, p(ids), m, 0, R, L, 1.2, None, None))
        refused("A: L = 0", lambda: A(h, p(ids), m, 0, R, 0, 1.2, p(rows), None))
        refused("A: start = n", lambda: A(h, p(ids), m, n, R, L, 1.2, p(rows), None))
        refused("A: R = 0", lambda: A(h, p(ids), m, 0, 0, L, 1.2, p(rows), None))
        refused("A: R > max_deg", lambda: A(h, p(ids), m, 0, max_deg + 1, L, 1.2, p(rows), None))
        refused("B: null ids", lambda: B(h, None, m, p(rows), R, 1.2, None))
        refused("B: null rows", lambda: B(h, p(ids), m, None, R, 1.2, None))
        refused("B: R = 0", lambda: B(h, p(ids), m, p(rows), 0, 1.2, None))
        refused("B: R > max_deg", lambda: B(h, p(ids), m, p(rows), max_deg + 1, 1.2, None))
        T_, S_ = lib.pann_hcnng_build_trees_dev, lib.pann_hcnng_assemble_dev
        refused("trees: mst_deg = 0", lambda: T_(h, 0, 1, 2, 100, 0, 1, p(slab), 8, None))
        refused("trees: tree_step = 0", lambda: T_(h, 0, 0, 2, 100, 3, 1, p(slab), 8, None))
        refused("trees: null slab", lambda: T_(h, 0, 1, 2, 100, 3, 1, None, 8, None))
        refused("assemble: null slabs", lambda: S_(h, None, 1, 8, 2, 3))
        refused("assemble: ntrees * mst_deg > max_deg", lambda: S_(h, p(slab), 1, 18, 6, 3))
        # m = 0 is no error and writes nothing
        st = _capi.BuildStats()
        assert A(h, p(ids), 0, 0, R, L, 1.2, p(rows), C.byref(st)) == 0 and B(h, p(ids), 0, p(rows), R, 1.2, C.byref(st)) == 0
        assert (_to_host(rows) == POISON).all() and st.visited_total == 0
        np.testing.assert_array_equal(ix.get_graph(), G)
        # the handle still works: one more batch through both phases equals the oracle's
        out = torch.full((m, R), POISON, dtype=torch.int32, device=_dev())
        torch.cuda.synchronize()
        ix.vamana_search_prune_dev(ids.data_ptr(), m, R, L, 1.2, out.data_ptr())
        h_ids = np.arange(10, 10 + m, dtype=np.uint32)
        want = oracle.vamana_phase_a(X, G, h_ids, R, L, 1.2)
        np.testing.assert_array_equal(_to_host(out), want)
        ix.vamana_apply_rows_dev(ids.data_ptr(), m, out.data_ptr(), R, 1.2)
        oracle.vamana_phase_b(X, G, h_ids, want, R, 1.2)
        np.testing.assert_array_equal(tp.norm(ix.get_graph()), tp.norm(G))
    finally:
        ix.close()
