"""CPU-only: the reachability rule (tests/reach_ref.py) on graphs whose levels are written out by hand, the four new C-ABI
names in the ctypes table, and the quality table of DESIGN.md "Graph reachability" on the oracle."""
import ctypes as C

import numpy as np
import pytest

import delete_ref
import reach_ref as rr

NONE = rr.NONE


def _levels(G, starts, **kw):
    return rr.reach_ref(G, starts, **kw)


def test_path_by_hand():
    r = _levels(rr.path_graph(5), (0,))
    assert r["level"].tolist() == [0, 1, 2, 3, 4]
    assert (r["reached_count"], r["unreached_count"], r["levels"], r["max_frontier"], r["truncated"]) == (5, 0, 5, 1, False)
    assert r["reached"].tolist() == [0b11111] and r["unreached_ids"].tolist() == []
    r = _levels(rr.path_graph(5), (2,))
    assert r["level"].tolist() == [NONE, NONE, 0, 1, 2] and r["unreached_ids"].tolist() == [0, 1]
    assert r["reached"].tolist() == [0b11100] and r["levels"] == 3


def test_cycle_by_hand():
    G = rr.host_rows([[1], [2], [3], [0]], 2)
    assert _levels(G, (2,))["level"].tolist() == [2, 3, 0, 1]
    assert _levels(G, (2,))["levels"] == 4


def test_two_components_and_consider():
    G = rr.host_rows([[1, 2], [2], [], [4], [3], []], 2)            # {0, 1, 2} | {3, 4} | {5}
    r = _levels(G, (0,))
    assert r["level"].tolist() == [0, 1, 1, NONE, NONE, NONE]
    assert r["unreached_ids"].tolist() == [3, 4, 5] and (r["reached_count"], r["levels"], r["max_frontier"]) == (3, 2, 2)
    cons = np.array([1, 1, 0, 1, 0, 1], bool)
    r = _levels(G, (0,), consider=cons)
    assert r["unreached_ids"].tolist() == [3, 5] and r["unreached_count"] == 2 and r["reached_count"] == 3      # the walk is not steered
    assert r["level"][2] == 1                                          # ... it went through the vertex that is not considered
    packed = np.array([0b101011 | 0xFFFFFFC0], np.uint32)             # the same, packed, with bits set beyond n
    assert _levels(G, (0,), consider=packed)["unreached_ids"].tolist() == [3, 5]
    r = _levels(G, (0, 3))
    assert r["level"].tolist() == [0, 1, 1, 0, 1, NONE] and r["max_frontier"] == 3


def test_self_loops_and_duplicate_slots():
    G = rr.host_rows([[0, 1, 1, 1], [1, 2, 2, 0], [2], []], 4)
    r = _levels(G, (0,))
    assert r["level"].tolist() == [0, 1, 2, NONE] and r["max_frontier"] == 1 and r["levels"] == 3
    out_deg, in_deg = rr.degrees_ref(G)
    assert out_deg.tolist() == [4, 4, 1, 0] and in_deg.tolist() == [2, 4, 3, 0]


def test_empty_graph_and_repeated_start():
    G = np.zeros((4, 3), np.uint32)
    r = _levels(G, (1, 1, 1))
    assert r["level"].tolist() == [NONE, 0, NONE, NONE] and (r["reached_count"], r["levels"], r["max_frontier"]) == (1, 1, 1)
    assert r["unreached_ids"].tolist() == [0, 2, 3] and not r["truncated"]
    r = _levels(G, (0, 1, 2, 3, 0))
    assert r["level"].tolist() == [0, 0, 0, 0] and r["max_frontier"] == 4 and r["unreached_count"] == 0
    with pytest.raises(ValueError):
        _levels(G, (4,))
    with pytest.raises(ValueError):
        _levels(G, ())


def test_max_rounds_by_hand():
    G = rr.path_graph(5)
    r = _levels(G, (0,), max_rounds=1)
    assert r["level"].tolist() == [0, 1, NONE, NONE, NONE] and r["truncated"] and r["levels"] == 2 and r["unreached_count"] == 3
    r = _levels(G, (0,), max_rounds=2)
    assert r["level"].tolist() == [0, 1, 2, NONE, NONE] and r["truncated"] and r["levels"] == 3
    r = _levels(G, (0,), max_rounds=4)                                 # the level-4 frontier {4} is not empty: truncated
    assert r["level"].tolist() == [0, 1, 2, 3, 4] and r["truncated"] and r["unreached_count"] == 0
    r = _levels(G, (0,), max_rounds=5)                                 # the fifth round finds nothing: the walk ended by itself
    assert r["level"].tolist() == [0, 1, 2, 3, 4] and not r["truncated"] and r["levels"] == 5
    r = _levels(rr.host_rows([[1], [], []], 1), (0,), max_rounds=1)    # level 1 = {1} is not empty, whatever its row holds
    assert r["truncated"] and r["level"].tolist() == [0, 1, NONE]


def test_case_builders():
    G = rr.many_parents_graph()
    r = _levels(G, (0,))
    assert len(G) == 2100 and r["levels"] == 4 and r["max_frontier"] == rr.MP_PARENTS and r["unreached_count"] == rr.MP_LOOSE
    assert (r["level"][-rr.MP_LOOSE - rr.MP_TARGETS:-rr.MP_LOOSE] == 3).all()
    assert rr.degrees_ref(G)[1][-rr.MP_LOOSE - 1] == rr.MP_PARENTS
    r = _levels(rr.path_graph(3000), (0,), max_rounds=10)
    assert r["truncated"] and r["levels"] == 11 and r["reached_count"] == 11
    for md in (64, 80):
        G = rr.ragged_graph(3000, md, 40 + md)
        assert set(G[:, 0]) == set(range(md + 1))
        r = _levels(G, (0,))
        assert 0 < r["unreached_count"] < 3000 and r["levels"] >= 3
    r = _levels(rr.random_graph(40000, 16, 7), (0,))
    assert r["max_frontier"] > 8192                                    # more frontier vertices than waves of one expand launch


def test_the_four_names_are_bound():
    from parlayann_amd import _capi
    arity = {"pann_graph_reach_dev": 10, "pann_graph_reach": 10, "pann_graph_degrees_dev": 4, "pann_graph_degrees": 3}
    for name, n_args in arity.items():
        assert name in _capi.SIGNATURES, name
        res, args = _capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, name
    assert C.sizeof(_capi.ReachStats) == 40
    assert _capi.ReachStats.levels.offset == 24 and _capi.ReachStats.t_s.offset == 32
    assert hasattr(_capi.load(), "pann_graph_reach_dev")


def test_quality_table(oracle):
    """The table of DESIGN.md "Graph reachability": unreached vertices from vertex 0 of a small-R build over clustered points,
    straight after the build and after deleting 30 %, and what rounds of re-insertion (reconnect_ref) leave.  Asserted: there IS
    something unreached after every consolidation (otherwise this shows nothing) and reconnect strictly reduces it.  The counts
    themselves are printed (pytest -s) and recorded in DESIGN.md, not asserted."""
    X = rr.quality_points()
    n = rr.Q_N
    G0 = oracle.vamana_build(X, rr.Q_R, rr.Q_L, rr.Q_ALPHA, num_passes=1, seed=rr.Q_BUILD_SEED)[0]
    fresh = rr.reach_ref(G0, (0,))
    _, rec = rr.reconnect_ref(oracle, X, G0, rr.Q_R, rr.Q_L, rr.Q_ALPHA, 0, None, 3)
    print(f"\nfresh build R={rr.Q_R}: unreached {fresh['unreached_count']} of {n}, levels {fresh['levels']}, largest level "
          f"{fresh['max_frontier']}; reconnect rounds {rec['unreached']}")
    for seed in rr.Q_SEEDS:
        D = delete_ref.seeded_ids(n, rr.Q_FRACTION, seed, keep=(0,))
        G1 = delete_ref.delete_ref(oracle, X, G0, D, rr.Q_ALPHA, rr.Q_R)[0]
        live = rr.live_bitmap(n, D)
        before = rr.reach_ref(G1, (0,), live)
        G2, rec = rr.reconnect_ref(oracle, X, G1, rr.Q_R, rr.Q_L, rr.Q_ALPHA, 0, live, 3)
        print(f"delete seed {seed}: {len(D)} deleted, unreached live {before['unreached_count']}, levels {before['levels']}; "
              f"reconnect rounds {rec['unreached']}")
        assert before["unreached_count"] >= 1
        assert rec["unreached"][0] == before["unreached_count"] and rec["unreached"][-1] < rec["unreached"][0]
        assert len(rec["remaining_ids"]) == rec["unreached"][-1]
        assert not np.isin(rec["remaining_ids"], D).any()
        G2 = delete_ref.normalized(G2)
        assert (G2[D, 0] == 0).all() and not np.isin(rr.neighbours(G2, np.arange(n)), D).any()      # no deleted id came back
