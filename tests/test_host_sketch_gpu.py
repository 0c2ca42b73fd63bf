"""The two-level search of the C++ host mirror (parlayann_amd/host/sketch.h, beam_search.h, vamana/neighbors.h).
tests/host_sketch_check.cpp calls the three-range beam_search_rerank, the 10-argument qsearchAll and filtered_beam_search with
use_filtering on sketch ranges made by the translating PointRange constructor; every array it dumps is compared with the
Python composition (filtered search of the one-byte handle, then pann_rerank), run with hamming_as_written = 1 as the mirror
does.  The CLI with -graph_path and -quantize_mode 2 / 3 must print that composition's recall, and without a graph it must
leave through the documented abort."""
import os
import re
import subprocess

import numpy as np
import pytest

import filtered_cases as fc
from parlayann_amd import DeviceIndex, io, quantize
from parlayann_amd import sketch as sk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "parlayann_amd", "host")
N, NQ, K, BEAM, RF = 3000, 12, 10, 32, 3
CASES = [("l2", "bit", 100), ("mips", "bit", 100), ("mips", "2bit", 200)]


@pytest.fixture(scope="module")
def checker():
    subprocess.check_call(["make", "-C", HOST, "-s"])
    exe = os.path.join(ROOT, "tests", "host_sketch_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-Wno-sign-compare", "-o", exe,
                           os.path.join(ROOT, "tests", "host_sketch_check.cpp"), "-L" + os.path.join(ROOT, "parlayann_amd", "lib"),
                           "-lpann", "-Wl,-rpath," + os.path.join(ROOT, "parlayann_amd", "lib")])
    return exe


def _data(metric, d, seed):
    rng = np.random.default_rng(seed)
    if metric == "l2":
        return (rng.standard_normal((N, d)) * 30 + 120).astype(np.float32), (rng.standard_normal((NQ, d)) * 30 + 120).astype(np.float32)
    return rng.standard_normal((N, d)).astype(np.float32), rng.standard_normal((NQ, d)).astype(np.float32)


def _compose(X, Q, G, metric, level):
    """the Python path: one-byte copy searched with the sketch filter, exact rerank of the first min(k * rf, |frontier|)"""
    if metric == "l2":
        ep = quantize.euclid_u8_params(X)
        Xq, Qq = quantize.euclid_u8_translate(X, ep), quantize.euclid_u8_translate(Q, ep)
    else:
        mv = quantize.mips_i8_max_val(X, trim=True)
        Xq, Qq = quantize.mips_i8_translate(X, mv), quantize.mips_i8_translate(Q, mv)
    kind = "mips_2bit" if level == "2bit" else ("euclid_bit" if metric == "l2" else "mips_bit")
    src, qix = DeviceIndex(X, max_degree=4, metric=metric), DeviceIndex(Xq, G, metric=metric)
    try:
        p = sk.sketch_params(src, kind)
        p.hamming_as_written = 1
        sk.attach_sketch(qix, src, p)
        rows, sq = sk.download_sketch(qix), sk.sketch_rows(Q, p)
        r = qix.batch_search_filtered(Qq, sq, k=K, beam=BEAM, out_k=BEAM, visited_cap=2000)
        counts = np.minimum(r["frontier_size"], K * RF).astype(np.uint32)
        ids, dists = src.rerank(Q, r["ids"], counts, K, resort=True)
        one = qix.batch_search_filtered(Qq[2:3], sq[2:3], k=K, beam=BEAM, out_k=BEAM, visited_cap=2000)
        base = qix.batch_search_filtered(query_ids=[77], k=K, beam=BEAM, out_k=BEAM, visited_cap=2000)
    finally:
        src.close(); qix.close()
    return dict(p=p, rows=rows, sq=sq, r=r, ids=ids, dists=dists, one=one, base=base)


@pytest.mark.parametrize("metric,level,d", CASES)
def test_host_mirror_equals_the_python_composition(checker, tmp_path, metric, level, d):
    X, Q = _data(metric, d, 11 + d)
    G = fc.random_graph(N, 32, 5)
    io.write_bin(tmp_path / "b.fbin", X); io.write_bin(tmp_path / "q.fbin", Q); io.write_graph(tmp_path / "g.graph", G)
    out = tmp_path / "out"; out.mkdir()
    pr = subprocess.run([checker, str(tmp_path / "b.fbin"), str(tmp_path / "q.fbin"), str(tmp_path / "g.graph"), str(out), metric, level,
                         str(K), str(BEAM), str(RF)], capture_output=True, text=True)
    assert pr.returncode == 0 and "host_sketch_check done" in pr.stdout, pr.stdout[-3000:] + pr.stderr[-3000:]

    def ld(name, dt):
        return np.fromfile(out / (name + ".bin"), dtype=dt)
    c = _compose(X, Q, G, metric, level)
    # host types: parameters, num_bytes(), translated rows
    assert int(ld("qq_num_bytes", np.int32)[0]) == sk.row_bytes(c["p"].kind, d)
    if level == "2bit":
        assert ld("qq_cut", np.float32)[0] == np.float32(c["p"].cut)
    elif metric == "l2":
        assert int(ld("qq_median", np.int64)[0]) == c["p"].median
    np.testing.assert_array_equal(ld("qq_base_rows", np.uint8).reshape(N, -1), c["rows"])
    np.testing.assert_array_equal(ld("qq_query_rows", np.uint8).reshape(NQ, -1), c["sq"])
    assert (c["r"]["dist_cmps"] < c["r"]["pruned_cmps"]).any()           # the filter really dropped neighbours
    # three-range beam_search_rerank per query, and qsearchAll with a QQ range
    for name in ("rerank3", "qsearch3"):
        np.testing.assert_array_equal(ld(name + "_ids", np.uint32).reshape(NQ, K), c["ids"])
        np.testing.assert_array_equal(ld(name + "_dists", np.float32).reshape(NQ, K), c["dists"])
        np.testing.assert_array_equal(ld(name + "_visited", np.uint32), c["r"]["visited_count"])
        np.testing.assert_array_equal(ld(name + "_cmps", np.uint32), c["r"]["dist_cmps"])      # full_dist_cmps (:213)
    # filtered_beam_search(..., use_filtering = true): frontier, visited sorted by (dist, id), full_dist_cmps
    for name, g in (("fbs_ext", c["one"]), ("fbs_base", c["base"])):
        f, v = int(g["frontier_size"][0]), int(g["visited_count"][0])
        np.testing.assert_array_equal(ld(name + "_frontier_ids", np.uint32), g["ids"][0, :f])
        np.testing.assert_array_equal(ld(name + "_frontier_dists", np.float32), g["dists"][0, :f])
        vi, vd = g["visited_ids"][0, :v], g["visited_dists"][0, :v]
        srt = np.lexsort((vi, vd))
        np.testing.assert_array_equal(ld(name + "_visited_ids", np.uint32), vi[srt])
        np.testing.assert_array_equal(ld(name + "_visited_dists", np.float32), vd[srt])
        assert int(ld(name + "_cmps", np.uint64)[0]) == int(g["dist_cmps"][0])


def _cli(*args):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return subprocess.run([os.path.join(HOST, "vamana", "neighbors"), *[str(a) for a in args]], capture_output=True, text=True)


@pytest.mark.parametrize("metric,level,d", CASES)
def test_cli_with_a_prebuilt_graph_prints_the_python_recall(tmp_path, oracle, metric, level, d):
    X, Q = _data(metric, d, 31 + d)
    G = fc.random_graph(N, 32, 6)
    src = DeviceIndex(X, max_degree=4, metric=metric)
    gt, gd = src.bruteforce_knn(Q, 100)
    src.close()
    io.write_bin(tmp_path / "b.fbin", X); io.write_bin(tmp_path / "q.fbin", Q); io.write_graph(tmp_path / "g.graph", G)
    io.write_ibin(tmp_path / "gt.ibin", gt, gd)
    mode = 3 if level == "2bit" else 2
    r = _cli("-base_path", tmp_path / "b.fbin", "-query_path", tmp_path / "q.fbin", "-gt_path", tmp_path / "gt.ibin", "-graph_path",
             tmp_path / "g.graph", "-data_type", "float", "-dist_func", "Euclidian" if metric == "l2" else "mips", "-quantize_mode", mode,
             "-rerank_factor", RF, "-R", 32, "-L", 64, "-alpha", 1.2, "-k", K, "-Q", BEAM, "-verbose")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    c = _compose(X, Q, G, metric, level)
    rec = float(re.findall(r"recall=([0-9.]+)", r.stdout)[0])
    assert abs(rec - oracle.recall(c["ids"], gt, gd, K)) < 1e-6
    vis = int(re.findall(r"visited=([0-9]+)", r.stdout)[0])
    assert vis == int(c["r"]["visited_count"].astype(np.uint64).sum() // NQ)


@pytest.mark.parametrize("metric,mode", [("Euclidian", 2), ("mips", 3), ("Euclidian", 3), ("mips", 4)])
def test_cli_without_a_graph_or_with_an_unmirrored_mode_aborts(tmp_path, metric, mode):
    X, Q = _data("mips", 64, 3)
    io.write_bin(tmp_path / "b.fbin", X[:500]); io.write_bin(tmp_path / "q.fbin", Q)
    io.write_graph(tmp_path / "g.graph", fc.random_graph(500, 32, 6))
    args = ["-base_path", tmp_path / "b.fbin", "-query_path", tmp_path / "q.fbin", "-data_type", "float", "-dist_func", metric,
            "-quantize_mode", mode, "-R", 32, "-L", 64, "-alpha", 1.2, "-k", K, "-Q", BEAM]
    mirrored = mode == 2 or (mode == 3 and metric == "mips")
    if not mirrored:
        args += ["-graph_path", tmp_path / "g.graph"]        # even with a graph these modes are rejected
    r = _cli(*args)
    assert r.returncode != 0
    assert ("sketch-filtered builds are not mirrored" if mirrored else "is not mirrored; modes 0, 1, 2 and (mips) 3 are") in r.stdout
