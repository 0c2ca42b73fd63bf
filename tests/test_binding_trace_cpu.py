"""CPU-only: what parlayann_amd/index.py and parlayann_amd/graph_index.py ask of the C-ABI, and what they hand back.

Every row of tests/golden/binding_trace_v1.txt -- a digest of the C calls a method made (symbol, scalars, null / non-null
pointers, struct fields, the bytes of every input array) and of what it returned or raised, recorded by
tests/golden/make_binding_trace.py against a stand-in library while every method still spelled out its own filter arms -- is
recomputed on this tree and compared.  Nothing here computes: no libpann.so, no device.
"""
import os

import pytest

from golden import make_binding_trace as rec

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_trace_v1.txt")
with open(TABLE) as f:
    WANT = dict(l.split() for l in f if not l.startswith("#"))


def test_the_table_and_the_recorder_name_the_same_cases():
    assert list(WANT) == list(rec.CASES)


@pytest.mark.parametrize("case", list(rec.CASES))
def test_binding_asks_and_returns_what_it_did(case, tmp_path):
    text = rec.run(case, tmp_path)
    assert rec.hashlib.sha256(text.encode()).hexdigest() == WANT[case], text
