"""Launch shapes of the beam search that no other test pins (beam_search.hip: launch_beam_search): persistent grids with more
queries than filter tables, and more than 48 KB of dynamic LDS.  u8 L2, n = 4096, d = 32, a random graph of degree 16,
base-point queries; ids, dists, visited_count and dist_cmps bit for bit against the CPU oracle (tests/oracle_api.py), the
masked case against the restatement tests/masked_ref.py."""
import numpy as np
import pytest

import masked_ref
from parlayann_amd import DeviceIndex, datasets

pytestmark = pytest.mark.gpu

N, D, DEG = 4096, 32, 16
NQ_PERSISTENT = 2200       # > 2048: the b128 kernel moves its filter to HBM, and the generic kernel has 2048 tables
DISTINCT = 128             # the 2200 queries repeat 128 base points: a query's result depends on nothing but its point (and
                           # the shared bitmap), so the Python restatement runs once per distinct point and every one of the
                           # 2200 device results is still compared


@pytest.fixture(scope="module")
def world():
    X = datasets.sift_like(N, D, seed=1234, dtype=np.uint8)
    rng = np.random.default_rng(99)
    G = np.empty((N, 1 + DEG), np.uint32)
    G[:, 0] = DEG
    G[:, 1:] = rng.integers(0, N, size=(N, DEG), dtype=np.uint32)
    base = rng.choice(N, size=DISTINCT, replace=False).astype(np.uint32)
    pick = rng.integers(0, DISTINCT, size=NQ_PERSISTENT)
    allow = rng.random(N) < 0.5                        # one shared bitmap, half the points
    ix = DeviceIndex(X, G)                             # no filter codes on this handle
    yield X, G, base, pick, allow, ix
    ix.close()


def _same(o, g):
    np.testing.assert_array_equal(o["ids"], g["ids"], err_msg="ids")
    np.testing.assert_array_equal(o["dists"].view(np.uint32), g["dists"].view(np.uint32), err_msg="dists")
    for f in ("visited_count", "dist_cmps"):
        np.testing.assert_array_equal(o[f], g[f], err_msg=f)


@pytest.mark.parametrize("nq,beam,k", [(NQ_PERSISTENT, 100, 10),    # b128 kernel, filter in HBM, 2200 blocks for 8192 tables
                                       (NQ_PERSISTENT, 200, 10),    # generic kernel, filter in HBM, 2048 blocks for 2200 queries
                                       (4, 3000, 10)])              # generic kernel, about 58 KB of dynamic LDS
def test_launch_shapes_equal_the_oracle(oracle, world, nq, beam, k):
    X, G, base, pick, _, ix = world
    qids = base[pick]
    o = oracle.batch_search(X, G, query_ids=qids[:nq], k=k, beam=beam, cut=1.35)
    g = ix.batch_search(query_ids=qids[:nq], k=k, beam=beam, cut=1.35)
    assert o["rc"] == 0
    _same(o, g)


def test_masked_persistent_grid_equals_the_restatement(world):
    X, G, base, pick, allow, ix = world
    kw = dict(k=10, beam=200, cut=1.35, out_k=10)
    once = masked_ref.masked_batch_search(X, G, allow, query_ids=base, **kw)
    ref = {f: once[f][pick] for f in ("ids", "dists", "visited_count", "dist_cmps", "result_count", "allowed_cmps")}
    g = ix.batch_search_masked(query_ids=base[pick], allow=allow, **kw)
    assert g["status"][0] == 0
    _same(ref, g)
    for f in ("result_count", "allowed_cmps"):
        np.testing.assert_array_equal(ref[f], g[f], err_msg=f)
