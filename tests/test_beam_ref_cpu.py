"""CPU-only: the one walk behind the four Python checkers (tests/beam_ref.py) and what the checkers return.

* every row of tests/golden/beam_ref_v1.txt -- digests of what tests/masked_ref.py, tests/steered_ref.py, tests/filtered_ref.py
  and tests/seen_ref.py returned while each carried its own copy of the walk (tests/golden/make_beam_ref_digests.py) -- is
  recomputed and compared;
* the walk with no variant equals the C++ oracle field for field;
* each checker in its "off" setting returns the plain walk's plain fields.
"""
import os

import numpy as np
import pytest

import beam_ref
import filtered_ref
import masked_ref
import seen_ref
import steered_ref
import test_filtered_ref_cpu as tf
from golden import make_beam_ref_digests as rec

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_ref_v1.txt")
FIELDS = ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum")
PIN_IDS = [f"{np.dtype(c[0]).name}-{c[1]}-b{c[2]}-k{c[3]}-{i}" for i, c in enumerate(tf.PIN_CASES)]
_plain = {}


def plain(i):
    """the plain walk on PIN_CASES[i], computed once and never changed -> (X, G, keywords, result)"""
    if i not in _plain:
        X, G, kw = rec.filtered_pin_case(tf.PIN_CASES[i])
        _plain[i] = (X, G, kw, beam_ref.batch_search(X, G, **kw))
    return _plain[i]


@pytest.mark.parametrize("group", list(rec.GROUPS))
def test_checkers_return_what_they_returned_with_a_walk_each(oracle, group):
    with open(TABLE) as f:
        want = [l.rstrip("\n") for l in f if l.startswith(group + " ")]
    assert want and rec.lines(group) == want


@pytest.mark.parametrize("i", range(len(tf.PIN_CASES)), ids=PIN_IDS)
def test_plain_walk_equals_the_oracle(oracle, i):
    X, G, kw, g = plain(i)
    r = oracle.batch_search(X, G, **kw)
    assert r["rc"] == 0
    for f in FIELDS:
        assert np.array_equal(g[f], r[f]), f
    assert np.array_equal(g["pruned_cmps"], r["dist_cmps"])
    assert g["frontier_ids"] is g["ids"] and g["frontier_dists"] is g["dists"]
    for q in range(len(g["ids"])):
        v = int(r["visited_count"][q])
        assert np.array_equal(g["visited_ids"][q, :v], r["visit_order_ids"][q, :v])
        assert np.array_equal(g["visited_sorted_ids"][q, :v], r["visited_ids"][q, :v])
        srt = np.lexsort((g["visited_ids"][q, :v], g["visited_dists"][q, :v]))
        assert np.array_equal(g["visited_dists"][q, :v][srt], r["visited_dists"][q, :v])
        m = min(kw["out_k"], len(g["final_frontier"][q]))
        assert [e[1] for e in g["final_frontier"][q][:m]] == g["ids"][q, :m].tolist()


@pytest.mark.parametrize("i", range(len(tf.PIN_CASES)), ids=PIN_IDS)
def test_every_checker_switched_off_is_the_plain_walk(oracle, i):
    X, G, kw, want = plain(i)
    ones = np.ones(len(X), bool)
    no_cap = {a: b for a, b in kw.items() if a != "visited_cap"}
    runs = {"masked": masked_ref.masked_batch_search(X, G, ones, **kw),
            "steered": steered_ref.steered_batch_search(X, G, ones, fill=(0, 1, 3, 16, 40)[i % 5], **kw),
            "filtered": filtered_ref.filtered_batch_search(X, G, use_filtering=False, **kw),
            "seen": seen_ref.seen_batch_search(X, G, v_n=0, **no_cap)}
    for name, got in runs.items():
        head = ("frontier_ids", "frontier_dists") if name in ("masked", "steered") else ("ids", "dists")
        assert np.array_equal(got[head[0]], want["ids"]) and np.array_equal(got[head[1]], want["dists"]), name
        for f in FIELDS[2:]:
            assert np.array_equal(got[f], want[f]), (name, f)
        for f in ("visited_ids", "visited_dists", "visited_sorted_ids", "pruned_cmps"):
            if f in got:
                assert np.array_equal(got[f], want[f]), (name, f)
        if "final_frontier" in got:
            assert got["final_frontier"] == want["final_frontier"], name
    assert not runs["steered"]["bridge_rows"].any() and not runs["filtered"]["sketch_dropped"].any()
    assert not runs["seen"]["lookups"].any() and not runs["seen"]["skipped"].any()
