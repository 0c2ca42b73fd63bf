"""The label-aware build without a GPU: the new entries are declared to ctypes as the header declares them, and the CPU
restatement (tests/labeled_build_ref.py) with equal labels is its own plain prune."""
import os
import re

import numpy as np

import labeled_build_ref as lr
from parlayann_amd import _capi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pann.h")


def test_new_entries_match_the_header():
    text = open(HEADER).read()
    for name in ("pann_vamana_insert_batch_labeled", "pann_vamana_insert_batch_labeled_dev", "pann_vamana_build_labeled"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text).group(1)
        assert len(_capi.SIGNATURES[name][1]) == decl.count(",") + 1, name


def test_equal_labels_restate_the_plain_prune(oracle):
    n, R, L = 40, 4, 8
    rng = np.random.default_rng(3)
    X = rng.integers(0, 32, (n, 9)).astype(np.uint8)
    G = np.zeros((n, R + 1), np.uint32)
    G[:, 0] = 2
    G[:, 1:3] = [(v + 1 + rng.choice(n - 1, 2, replace=False)) % n for v in range(n)]
    table, batch, same = np.zeros((32, 1), np.uint32), rng.permutation(n)[:25].astype(np.uint32), np.full(n, 1 << 5, np.uint32)
    got, info = lr.insert_batch(oracle, X, G, same, batch, table, R, L, 1.2)
    want, _ = lr.insert_batch(oracle, X, G, same, batch, table, R, L, 1.2, filtered=False)
    np.testing.assert_array_equal(got, want)
    assert info["heavy"] and info["longest"] > R
