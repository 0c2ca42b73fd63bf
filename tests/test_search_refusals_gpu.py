"""What the plain, filtered, steered, grouped, per-query-starts and fused-rerank search entry points refuse, and in which order:
every row of tests/search_refusal_cases.py -- one fault, or two faults that are neighbours in the entry's check order -- must give
the return code AND the full pann_last_error() text that tests/golden/search_refusals_v1.json records.  The file was written by
tests/golden/make_search_refusals.py from the library of the commit named in it (the last one before the request descriptor);
this test never regenerates it.  No call here launches a kernel, so the outputs -- host and device -- still hold their fill at
the end."""
import json
import os

import pytest

import search_refusal_cases as sr
from parlayann_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_refusals_v1.json")


def test_codes_and_texts_equal_the_recorded_ones():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(golden["commit"]) >= 7
    table = sr.rows()
    assert sorted(golden["rows"]) == sorted(rid for rid, *_ in table)          # the table and the record name the same calls
    w = sr.World()
    try:
        wrong = []
        for rid, entry, dev, faults in table:
            rc, msg = w.call(entry, dev, faults)
            want = golden["rows"][rid]
            if (rc, msg) != (want["rc"], want["msg"]):
                wrong.append((rid, rc, msg, want))
            served = any(f in sr.OK_FAULTS for f in faults) and rc == _capi.PANN_OK      # nothing to do: the only call that is served
            assert served or (rc != _capi.PANN_OK and msg and "unknown option" not in msg), (rid, rc, msg)
        assert not wrong, wrong
        assert w.untouched()
    finally:
        w.close()


def test_every_entry_point_is_in_the_table():
    names = {entry + ("_dev" if dev else "") for _, entry, dev, _ in sr.rows()}
    assert len(names) == 13 and all(n in _capi.SIGNATURES for n in names)


def test_every_fault_is_used_and_every_chain_fault_is_known():
    used = {f for *_, faults in sr.rows() for f in faults}
    assert used == set(sr.FAULTS)
