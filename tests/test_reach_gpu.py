"""pann_graph_reach* / pann_graph_degrees* on the device against the numpy restatement of the rule (tests/reach_ref.py), field
for field and exactly: levels, bitmap words, the id list and every statistic but the time.  The shapes are the smallest at which
each mechanism can go wrong: a path (one level per vertex: the level loop must not round-trip per level), many parents of the
same targets (exactly-once discovery under races), a frontier wider than one expand launch, rows wider than a wavefront."""
import ctypes as C
import time

import numpy as np
import pytest

import delete_ref
import reach_ref as rr
import stream_order as so
from parlayann_amd import DeviceIndex, PannError, _capi, graph_index, io
from parlayann_amd.index import pack_allow

pytestmark = pytest.mark.gpu

BAD_ARG, OVERFLOW = _capi.PANN_ERR_BAD_ARG, _capi.PANN_ERR_OVERFLOW
U32 = np.uint32
_made = {}


def points(n, d=8):
    return (np.arange(n * d, dtype=np.int64).reshape(n, d) * 37 % 251).astype(np.uint8)      # anything: points are never read


def index_of(name, make):
    """the handle over a case's graph and its graph, made once"""
    if name not in _made:
        G = make()
        _made[name] = (DeviceIndex(points(len(G)), G), G)
    return _made[name]


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    for ix, _ in _made.values():
        ix.close()
    _made.clear()


def check(ix, G, starts=(0,), consider=None, max_rounds=0):
    got, ref = ix.reachability(starts, consider, max_rounds), rr.reach_ref(G, starts, consider, max_rounds)
    rr.same_fields(got, ref)
    assert got["seconds"] > 0
    return got


def _vp(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def _poisoned(words):
    import torch
    t = torch.empty(max(int(words), 1), dtype=torch.int32, device="cuda:0")
    so.poison(t)
    return t


def _host(t, words):
    return t.cpu().numpy().view(U32)[:words]


def reach_dev(ix, starts, consider=None, max_rounds=0, cap=None, level=True, reached=True, ids=True):
    """pann_graph_reach_dev on device arrays full of poison -> (status, stats, level, reached, ids), the arrays as they are after
    the call (whole, poison where nothing was written)"""
    import torch
    n, w = ix.n, (ix.n + 31) // 32
    lib = _capi.load()
    d_s = torch.from_numpy(np.ascontiguousarray(starts, U32).view(np.int32)).to("cuda:0")
    d_c = None if consider is None else torch.from_numpy(pack_allow(consider, n).view(np.int32)).to("cuda:0")
    cap = n if cap is None else cap
    d_l, d_r, d_i = (_poisoned(n) if level else None), (_poisoned(w) if reached else None), (_poisoned(cap) if ids else None)
    torch.cuda.synchronize()
    st = _capi.ReachStats()
    rc = lib.pann_graph_reach_dev(ix.handle, _vp(d_s), len(d_s), _vp(d_c), max_rounds, _vp(d_l), _vp(d_r), _vp(d_i), cap, C.byref(st))
    return (rc, st, None if d_l is None else _host(d_l, n), None if d_r is None else _host(d_r, w),
            None if d_i is None else _host(d_i, cap))


def same_stats(st, ref):
    assert (st.reached, st.unreached, st.levels, st.max_frontier, bool(st.truncated)) == \
        (ref["reached_count"], ref["unreached_count"], ref["levels"], ref["max_frontier"], ref["truncated"])


# ---- the level loop ---------------------------------------------------------------------------------------------------------

def test_path():
    """3 000 levels of one vertex; then max_rounds = 10: levels 0 .. 10 and truncated"""
    ix, G = index_of("path", lambda: rr.path_graph(3000))
    got = check(ix, G)
    assert got["levels"] == 3000 and got["max_frontier"] == 1 and got["unreached_count"] == 0
    t0 = time.perf_counter()
    ix.reachability(levels=False, ids=False)
    print(f"\npath of 3000 levels: {1e3 * (time.perf_counter() - t0):.1f} ms host time")
    got = check(ix, G, max_rounds=10)
    assert got["truncated"] and got["levels"] == 11 and (got["level"][:11] == np.arange(11)).all() and (got["level"][11:] == rr.NONE).all()
    for r in (1, 7, 8, 9, 16, 2999, 3000):                       # around the group size, and the round that empties the frontier
        check(ix, G, max_rounds=r)
    check(ix, G, starts=(2990, 5, 2990))


def test_many_parents():
    """2 000 vertices discover the same 64 targets in one round: each enters the next queue once"""
    ix, G = index_of("parents", rr.many_parents_graph)
    for _ in range(3):                                           # the race has many schedules; the answer has one
        got = check(ix, G)
        assert got["max_frontier"] == rr.MP_PARENTS and got["levels"] == 4 and got["reached_count"] == len(G) - rr.MP_LOOSE
    check(ix, G, starts=tuple(range(1 + rr.MP_FAN, 1 + rr.MP_FAN + rr.MP_PARENTS)))      # the parents as starts: 64 targets in round 1


@pytest.mark.parametrize("n", [40000, 40001])
def test_wide_frontier(n):
    """level populations beyond the 8 192 waves of one expand launch (grid-stride), n no multiple of 64 / the bitmap tail"""
    ix, G = index_of(("wide", n), lambda: rr.random_graph(n, 16, 7))
    got = check(ix, G)
    assert got["max_frontier"] > 8192
    live = np.random.default_rng(3).random(n) < 0.7
    check(ix, G, starts=(n - 1, 17), consider=live)


@pytest.mark.parametrize("max_deg", [64, 80])
def test_wide_rows(max_deg):
    """gstride 64 (one pass) and 80 (two passes): self loops, repeated neighbours, every degree 0 .. max_deg"""
    ix, G = index_of(("ragged", max_deg), lambda: rr.ragged_graph(3000, max_deg, 40 + max_deg))
    got = check(ix, G)
    assert 0 < got["unreached_count"] < 3000
    check(ix, G, starts=(2999, 1500), max_rounds=2)


# ---- degenerate cases -------------------------------------------------------------------------------------------------------

def test_single_vertex_and_empty_rows():
    ix, G = index_of("one", lambda: rr.host_rows([[0]], 4))
    check(ix, G)
    ix, G = index_of("empty", lambda: np.zeros((100, 5), U32))
    got = check(ix, G, starts=(7,))
    assert got["reached_count"] == 1 and got["unreached_count"] == 99 and got["levels"] == 1


def test_every_vertex_a_start_and_duplicate_starts():
    ix, G = index_of(("ragged", 64), lambda: rr.ragged_graph(3000, 64, 104))
    got = check(ix, G, starts=np.arange(3000))
    assert got["levels"] == 1 and got["max_frontier"] == 3000 and got["unreached_count"] == 0
    check(ix, G, starts=np.random.default_rng(5).integers(0, 40, 500))      # 500 starts, 40 distinct ids


def test_consider_with_bits_beyond_n():
    ix, G = index_of("parents", rr.many_parents_graph)
    n = len(G)
    cons = np.random.default_rng(9).random(n) < 0.5
    cons[-rr.MP_LOOSE:] = [True, False, True]
    packed = pack_allow(cons, n).copy()
    packed[-1] |= U32(0xFFFFFFFF << (n & 31) & 0xFFFFFFFF)                 # n = 2100: 20 live bits in the last word
    wide = np.concatenate([packed, np.full(3, 0xFFFFFFFF, U32)])         # and whole words past ceil(n / 32)
    for c in (cons, packed, wide):
        got = check(ix, G, consider=c)
        assert got["unreached_ids"].tolist() == [n - 3, n - 1]


def test_bad_start_writes_nothing():
    ix, G = index_of("parents", rr.many_parents_graph)
    n = len(G)
    for starts in ((n,), (0, 5, n + 7, 3), (0xFFFFFFFF,)):
        with pytest.raises(PannError) as e:
            ix.reachability(starts)
        assert e.value.code == BAD_ARG
        rc, st, level, reached, ids = reach_dev(ix, starts)
        assert rc == BAD_ARG
        for a in (level, reached, ids):
            assert (a == so.POISON_U32).all()
    lib = _capi.load()
    st = _capi.ReachStats()
    one = np.zeros(1, U32)
    assert lib.pann_graph_reach(ix.handle, None, 1, None, 0, None, None, None, 0, C.byref(st)) == BAD_ARG
    assert lib.pann_graph_reach(ix.handle, one.ctypes.data_as(C.c_void_p), 0, None, 0, None, None, None, 0, C.byref(st)) == BAD_ARG
    assert lib.pann_graph_reach(None, one.ctypes.data_as(C.c_void_p), 1, None, 0, None, None, None, 0, C.byref(st)) == BAD_ARG
    import torch
    d = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert lib.pann_graph_reach_dev(ix.handle, C.c_void_p(d.data_ptr() + 2), 1, None, 0, None, None, None, 0, C.byref(st)) == BAD_ARG
    assert lib.pann_graph_degrees_dev(ix.handle, C.c_void_p(d.data_ptr() + 1), None, None) == BAD_ARG
    assert lib.pann_graph_degrees_dev(ix.handle, None, None, None) == BAD_ARG
    assert lib.pann_graph_degrees(None, one.ctypes.data_as(C.c_void_p), None) == BAD_ARG


def test_device_form_and_overflow():
    """the _dev form equals the rule; a list one entry short is PANN_ERR_OVERFLOW with the list untouched and the rest valid;
    every output is optional"""
    ix, G = index_of(("ragged", 80), lambda: rr.ragged_graph(3000, 80, 120))
    n, lib = len(G), _capi.load()
    live = np.random.default_rng(4).random(n) < 0.8
    ref = rr.reach_ref(G, (0, 9), live)
    u = ref["unreached_count"]
    assert u > 1
    rc, st, level, reached, ids = reach_dev(ix, (0, 9), live)
    assert rc == 0
    same_stats(st, ref)
    np.testing.assert_array_equal(level, ref["level"]); np.testing.assert_array_equal(reached, ref["reached"])
    np.testing.assert_array_equal(ids[:u], ref["unreached_ids"])
    assert (ids[u:] == so.POISON_U32).all()                               # entries past stats.unreached are not written
    rc, st, level, reached, ids = reach_dev(ix, (0, 9), live, cap=u)      # exactly enough
    assert rc == 0
    np.testing.assert_array_equal(ids, ref["unreached_ids"])
    rc, st, level, reached, ids = reach_dev(ix, (0, 9), live, cap=u - 1)
    assert rc == OVERFLOW and (ids == so.POISON_U32).all()
    same_stats(st, ref)
    np.testing.assert_array_equal(level, ref["level"]); np.testing.assert_array_equal(reached, ref["reached"])
    # the host form: the same convention
    s, c = np.array([0, 9], U32), pack_allow(live, n)
    level, reached, ids = np.full(n, 7, U32), np.full((n + 31) // 32, 7, U32), np.full(u - 1, 7, U32)
    st = _capi.ReachStats()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.pann_graph_reach(ix.handle, p(s), 2, p(c), 0, p(level), p(reached), p(ids), u - 1, C.byref(st)) == OVERFLOW
    same_stats(st, ref)
    assert (ids == 7).all()
    np.testing.assert_array_equal(level, ref["level"]); np.testing.assert_array_equal(reached, ref["reached"])
    # optional outputs: stats alone, and each array alone
    rc, st, *_ = reach_dev(ix, (0, 9), live, level=False, reached=False, ids=False)
    assert rc == 0
    same_stats(st, ref)
    rc, st, level, reached, ids = reach_dev(ix, (0, 9), live, level=False, ids=False)
    np.testing.assert_array_equal(reached, ref["reached"])
    got = ix.reachability((0, 9), live, levels=False, ids=False)
    assert got["level"] is None and got["unreached_ids"] is None and got["unreached_count"] == u
    np.testing.assert_array_equal(got["reached"], ref["reached"])


def test_four_bit_handle_gives_the_same_answer():
    ix8, G = index_of(("ragged", 64), lambda: rr.ragged_graph(3000, 64, 104))
    ix4 = DeviceIndex.from_packed(points(len(G), 4), 8, "u4", graph=G)
    try:
        a, b = ix8.reachability((0, 11)), ix4.reachability((0, 11))
        rr.same_fields(b, rr.reach_ref(G, (0, 11)))
        rr.same_fields(b, a)
        for x, y in zip(ix8.degrees(), ix4.degrees()):
            np.testing.assert_array_equal(x, y)
    finally:
        ix4.close()


# ---- on a built graph -------------------------------------------------------------------------------------------------------

def test_built_graph_after_deletions():
    """the 3 000 x 16 quality case built and consolidated on the device: reachability equals the rule on get_graph(); the subset
    of what is live AND reached has no unreached vertex from the image of vertex 0"""
    X, n = rr.quality_points(), rr.Q_N
    ix = DeviceIndex(X, max_degree=rr.Q_R)
    ix.vamana_build(rr.Q_R, rr.Q_L, rr.Q_ALPHA, num_passes=1, seed=rr.Q_BUILD_SEED)
    check(ix, ix.get_graph())
    D = delete_ref.seeded_ids(n, rr.Q_FRACTION, 1, keep=(0,))
    ix.vamana_delete_batch(D, rr.Q_R, rr.Q_ALPHA)
    live = rr.live_bitmap(n, D)
    G = ix.get_graph()
    got = check(ix, G, consider=live)
    assert got["unreached_count"] >= 1 and not np.isin(got["unreached_ids"], D).any()
    keep = got["reached"] & live
    sub, n2o, o2n = ix.subset(keep)
    s = sub.reachability((int(o2n[0]),))
    assert s["unreached_count"] == 0 and s["reached_count"] == sub.n == n - len(D) - got["unreached_count"]
    rr.same_fields(s, rr.reach_ref(sub.get_graph(), (int(o2n[0]),)))
    sub.close(); ix.close()


def test_reconnect_equals_the_composition_on_the_oracle(oracle):
    X, n = rr.quality_points(), rr.Q_N
    G0 = oracle.vamana_build(X, rr.Q_R, rr.Q_L, rr.Q_ALPHA, num_passes=1, seed=rr.Q_BUILD_SEED)[0]
    D = delete_ref.seeded_ids(n, rr.Q_FRACTION, 2, keep=(0,))
    G1 = delete_ref.delete_ref(oracle, X, G0, D, rr.Q_ALPHA, rr.Q_R)[0]
    live = rr.live_bitmap(n, D)
    Gr, ref = rr.reconnect_ref(oracle, X, G1, rr.Q_R, rr.Q_L, rr.Q_ALPHA, 0, live, 3)
    ix = DeviceIndex(X, G1)
    got = ix.reconnect(rr.Q_R, rr.Q_L, rr.Q_ALPHA, 0, live, 3)
    print(f"\nreconnect: unreached per round {got['unreached']}")
    assert got["unreached"] == ref["unreached"] and len(ref["unreached"]) >= 2 and ref["unreached"][0] >= 1
    np.testing.assert_array_equal(got["remaining_ids"], ref["remaining_ids"])
    np.testing.assert_array_equal(delete_ref.normalized(ix.get_graph()), delete_ref.normalized(Gr))
    with pytest.raises(ValueError):
        ix.reconnect(rr.Q_R, rr.Q_L, rr.Q_ALPHA, int(D[0]), live)          # the start is not considered
    # nothing unreached: no round, nothing changed
    full = DeviceIndex(points(64), rr.host_rows([[(v + 1) % 64] for v in range(64)], 4))
    assert full.reconnect(4, 8, 1.2)["unreached"] == [0]
    full.close(); ix.close()


def test_graph_index_pass_throughs(tmp_path, oracle):
    X = rr.quality_points()[:600]
    G = oracle.vamana_build(X, 8, 16, 1.2, num_passes=1, seed=3)[0]
    io.write_bin(tmp_path / "b.bin", X); io.write_graph(tmp_path / "g", G)
    gi = graph_index.UInt8EuclidianIndex(str(tmp_path / "b.bin"), str(tmp_path / "g"))
    rr.same_fields(gi.reachability(), rr.reach_ref(G, (0,)))
    Gr, ref = rr.reconnect_ref(oracle, X, G, 8, 16, 1.2, 0, None, 2)
    assert gi.reconnect(8, 16, 1.2, max_rounds=2)["unreached"] == ref["unreached"]
    np.testing.assert_array_equal(delete_ref.normalized(gi.index.get_graph()), delete_ref.normalized(Gr))
    io.write_bin(tmp_path / "f.bin", X.astype(np.float32))
    gf = graph_index.FloatEuclidianIndex(str(tmp_path / "f.bin"), str(tmp_path / "g"))
    rr.same_fields(gf.reachability(), rr.reach_ref(G, (0,)))
    with pytest.raises(ValueError, match="copy_graph=True"):
        gf.reconnect(8, 16, 1.2)


# ---- degrees ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["ragged64", "ragged80", "parents", "wide16"])
def test_degrees(case):
    ix, G = {"ragged64": lambda: index_of(("ragged", 64), lambda: rr.ragged_graph(3000, 64, 104)),
             "ragged80": lambda: index_of(("ragged", 80), lambda: rr.ragged_graph(3000, 80, 120)),
             "parents": lambda: index_of("parents", rr.many_parents_graph),
             "wide16": lambda: index_of(("wide", 40001), lambda: rr.random_graph(40001, 16, 7))}[case]()
    out_deg, in_deg = ix.degrees()
    ro, ri = rr.degrees_ref(G)
    np.testing.assert_array_equal(out_deg, ro); np.testing.assert_array_equal(in_deg, ri)
    assert int(in_deg.sum()) == int(out_deg.sum())
    lib, n = _capi.load(), len(G)
    only = np.full(n, 7, U32)
    assert lib.pann_graph_degrees(ix.handle, None, only.ctypes.data_as(C.c_void_p)) == 0      # either output alone
    np.testing.assert_array_equal(only, ri)
    assert lib.pann_graph_degrees(ix.handle, only.ctypes.data_as(C.c_void_p), None) == 0
    np.testing.assert_array_equal(only, ro)


def test_degrees_dev_on_a_busy_stream():
    """pann_graph_degrees_dev behind a delay on the caller's stream: the outputs are poisoned AFTER the delay, so a zero-fill
    of d_in_deg (or a kernel) that the library put on another stream is overwritten and the sums come out wrong; and the call
    must come back while the delay runs.  (The graph is the handle's: there is no input to stage late.)"""
    import torch
    ix, G = index_of("parents", rr.many_parents_graph)
    n, lib = len(G), _capi.load()
    streams = so.independent_streams(torch.device("cuda", 0), want=1)
    if not streams:
        pytest.skip("none of torch's first 8 pool streams is overtaken by the null stream on this machine")
    s = streams[0]
    d_out, d_in = torch.zeros(n, dtype=torch.int32, device="cuda:0"), torch.zeros(n, dtype=torch.int32, device="cuda:0")
    call = lambda: _capi.check(lib.pann_graph_degrees_dev(ix.handle, _vp(d_out), _vp(d_in), C.c_void_p(s.cuda_stream)))
    call()                                                        # warm-up: the first launch loads the kernel
    s.synchronize()
    early = so.run_behind_delay(s, [], [d_out, d_in], [call])
    ro, ri = rr.degrees_ref(G)
    np.testing.assert_array_equal(_host(d_out, n), ro); np.testing.assert_array_equal(_host(d_in, n), ri)
    assert early, "pann_graph_degrees_dev came back only after the delay had run out: it synchronised"
