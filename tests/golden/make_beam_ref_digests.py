#!/usr/bin/env python3
"""Recorder of tests/golden/beam_ref_v1.txt: what the four Python restatements of the beam search (tests/masked_ref.py,
tests/steered_ref.py, tests/filtered_ref.py, tests/seen_ref.py) RETURNED at commit 8037fb3, the last one in which each of them
carried its own copy of the walk.  Run by hand; tests/test_beam_ref_cpu.py recomputes the same rows and compares.

The recorder imports the four public entry functions, the case modules and the pin tables of the three test_*_ref_cpu.py files,
and nothing else of the restatements, so the same text runs at 8037fb3 and at any later commit.  One line per (variant, case):
a SHA-256 digest over every field the function returned, in sorted key order -- an array as dtype, shape and bytes, None as a
marker, "final_frontier" as one float32 and one uint32 array per query.
usage: tests/golden/make_beam_ref_digests.py [--out FILE]"""
import argparse
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))) if p not in sys.path]

SEEN_ROWS = [          # second sightings on the fixture of tests/test_seen_ref_cpu.py, Q[:64]
    ("k10-cut1.35", dict(k=10, beam=64, cut=1.35)),
    ("k1-cut1.0-starts64", dict(k=1, beam=64, cut=1.0, starts=tuple(range(0, 64 * 311, 311)), out_k=10)),
    ("v256", dict(k=10, beam=64, cut=1.35, v_n=256)),
    ("insert-all", dict(k=10, beam=64, cut=1.35, insert="all")),
    ("b40-dl20", dict(k=10, beam=40, cut=1.35, degree_limit=20, out_k=40)),
]
SEEN_SKIPPED = [7623, 7689, 5835, 3962, 1896]      # sum of "skipped" over the 64 queries at 8037fb3: no row is vacuous
# the restate() keys tests/test_masked_rerank_cases_cpu.py asks for: (beam, k, rf, mask kind, query parameters)
RERANK_ROWS = [(64, 10, 100, "ones", {}), (64, 10, 100, "rand50", {}), (64, 10, 100, "zeros", {}), (64, 10, 100, "far_only", {}),
               (16, 10, 100, "rand5", {}), (16, 10, 100, "rand5", {"limit": 5}), (64, 2, 3, "rand50", {}), (64, 64, 100, "ones", {})]


def digest(res):
    h = hashlib.sha256()
    for key in sorted(res):
        v = res[key]
        h.update(key.encode() + b"\0")
        if v is None:
            h.update(b"<None>")
        elif key == "final_frontier":
            for fr in v:
                h.update(np.uint32(len(fr)).tobytes())
                h.update(np.array([e[0] for e in fr], np.float32).tobytes())
                h.update(np.array([e[1] for e in fr], np.uint32).tobytes())
        else:
            a = np.ascontiguousarray(v)
            h.update(f"{a.dtype.str}{a.shape}".encode())
            h.update(a.tobytes())
    return h.hexdigest()


def filtered_pin_case(case):
    """(X, G, keywords) of one PIN_CASES entry, as test_checker_without_filtering_equals_the_oracle builds them"""
    import filtered_cases as fc
    import test_filtered_ref_cpu as tf
    dtype, metric, beam, k, extra = case
    n, d, nq = 1200, 24, 10
    X, Q = tf._data(dtype, n, d, 11 + beam), tf._data(dtype, nq, d, 12 + beam)
    extra = dict(extra)
    kw = dict(k=k, beam=beam, metric=metric, out_k=beam, visited_cap=n)
    if extra.pop("query_ids", False):
        kw["query_ids"] = np.arange(3, 3 + 7 * nq, 7, dtype=np.uint32)
    else:
        kw["queries"] = Q
    kw.update(extra)
    return X, fc.random_graph(n, 16, 13 + beam), kw


def seen_fixture():
    import oracle_api
    import test_seen_ref_cpu as ts
    from parlayann_amd import datasets
    X = datasets.sift_like(ts.N, ts.D, seed=71, dtype=np.uint8)
    Q = datasets.sift_like(ts.NQ, ts.D, seed=72, dtype=np.uint8)
    G, _ = oracle_api.load().vamana_build(X, ts.R, ts.L, 1.15, num_passes=1, seed=3)
    return X, Q[:64], G


def masked_cases():
    import masked_cases as mc
    for case in mc.CASES:
        yield case[0], mc.case_reference(case)


def steered_cases():
    import steered_cases as sc
    for case in sc.CASES:
        yield case[0], sc.reference(case)


def filtered_cases():
    import filtered_cases as fc
    import filtered_ref
    for case in fc.CASES:
        c = fc.build_case(case)
        for on in (True, False):
            yield f"{case[0]}-{'sketch' if on else 'plain'}", filtered_ref.filtered_batch_search(**fc.checker_args(c, on))


def rerank_cases():
    import masked_rerank_cases as rc
    for name in rc.RESTATED:
        for beam, k, rf, mkind, qp in RERANK_ROWS:
            label = "-".join([name, f"b{beam}", f"k{k}", f"rf{rf}", mkind] + [f"{a}{b}" for a, b in qp.items()])
            yield label, rc.restate(name, beam, k, rf, mkind, **qp)


def masked_pins():
    import masked_ref
    import test_masked_ref_cpu as tm
    for dtype, metric, beam in tm.PIN:
        X, G, kw, allow = tm._pin_case(dtype, metric, beam)
        for mname, a in (("rand40", allow), ("ones", np.ones(tm.PIN_N, bool)), ("zeros", np.zeros(tm.PIN_N, bool))):
            yield f"{np.dtype(dtype).name}-{metric}-b{beam}-{mname}", masked_ref.masked_batch_search(X, G, a, **kw)


def steered_pins():
    import steered_ref
    import test_steered_ref_cpu as tsr
    for dtype, metric, beam in tsr.PIN:
        X, G, kw = tsr._case(dtype, metric, beam)
        tag = f"{np.dtype(dtype).name}-{metric}-b{beam}"
        for fill in (1, tsr.DEG // 2, 0):
            yield f"{tag}-ones-fill{fill}", steered_ref.steered_batch_search(X, G, np.ones(tsr.N, bool), fill=fill, **kw)
        for frac in (0.4, 0.05):
            allow = np.random.default_rng(24 + beam).random(tsr.N) < frac
            allow[5] = False
            for fill, dl in ((1, None), (tsr.DEG // 2, None), (0, None), (tsr.DEG + 5, None), (3, 11)):
                yield (f"{tag}-frac{frac}-fill{fill}-dl{dl}",
                       steered_ref.steered_batch_search(X, G, allow, fill=fill, degree_limit=dl, **kw))


def filtered_pins():
    import filtered_ref
    import test_filtered_ref_cpu as tf
    for i, case in enumerate(tf.PIN_CASES):
        X, G, kw = filtered_pin_case(case)
        yield f"{np.dtype(case[0]).name}-{case[1]}-b{case[2]}-k{case[3]}-{i}", filtered_ref.filtered_batch_search(X, G, use_filtering=False, **kw)


def seen_rows():
    import seen_ref
    X, Q, G = seen_fixture()
    for (label, kw), skipped in zip(SEEN_ROWS, SEEN_SKIPPED):
        r = seen_ref.seen_batch_search(X, G, queries=Q, **kw)
        assert int(r["skipped"].sum()) == skipped, (label, int(r["skipped"].sum()))
        yield label, r


GROUPS = {"masked_cases": masked_cases, "steered_cases": steered_cases, "filtered_cases": filtered_cases, "masked_rerank_cases": rerank_cases,
          "masked_pins": masked_pins, "steered_pins": steered_pins, "filtered_pins": filtered_pins, "seen": seen_rows}


def lines(group):
    return [f"{group} {label} {digest(res)}" for label, res in GROUPS[group]()]


def main():
    import time
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "beam_ref_v1.txt"))
    args = ap.parse_args()
    out = ["# group case sha256-of-every-returned-field"]
    for group in GROUPS:
        t0 = time.time()
        got = lines(group)
        print(f"{group}: {len(got)} rows, {time.time() - t0:.1f} s")
        out += got
    assert len({l.rsplit(" ", 1)[0] for l in out}) == len(out)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    sys.exit(main())
