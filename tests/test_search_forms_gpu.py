"""The results of every form of the search family, as they were: each case of tests/search_form_cases.py -- the nine search forms
and the three fused-rerank forms, host and _dev, with every optional output and with ids and dists alone -- must give, bit for bit,
the return code, the status word and every output array that tests/golden/search_forms_v1.npz records, the poison of what a call
leaves unwritten included (the visited rows of a host call: up to visited_count, search_form_cases.settled says why).  The file
was written by tests/golden/make_search_forms.py from the library of the commit named in it (the last one before the request
descriptor); this test never regenerates it."""
import os

import numpy as np
import pytest

import search_form_cases as sf
from parlayann_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_forms_v1.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def world():
    w = sf.World()
    yield w
    w.close()


def test_the_record_names_the_cases_and_was_served(golden):
    assert len(bytes(golden["commit"])) >= 7
    want = {cid for cid, *_ in sf.cases()}
    assert {k.split("/")[0] for k in golden if k != "commit"} == want and len(want) == 46
    for cid in want:
        assert golden[cid + "/rc"][0] == _capi.PANN_OK, cid
        ids = golden[cid + "/ids"]
        assert ((ids < sf.N) | (ids == 0xFFFFFFFF)).all() and (ids[:, 0] < sf.N).all(), cid      # written, and no poison left
        if cid.endswith(":all"):
            assert golden[cid + "/status"][0] & ~np.uint32(_capi.PANN_STATUS_SHORT_FRONTIER) == 0, cid


@pytest.mark.parametrize("cid,form,dev,full", sf.cases(), ids=[c[0] for c in sf.cases()])
def test_results_equal_the_recorded_ones(world, golden, cid, form, dev, full):
    got = sf.settled(dev, world.run(form, dev, full))
    want = sf.settled(dev, {k.split("/")[1]: a for k, a in golden.items() if k.startswith(cid + "/")})
    assert set(got) == set(want)
    wrong = [n for n, a in got.items() if a.shape != want[n].shape or not np.array_equal(a, want[n])]
    assert not wrong, (cid, wrong)
