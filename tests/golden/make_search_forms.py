"""Writes tests/golden/search_forms_v1.npz: every output array, the status word and the return code of every case of
tests/search_form_cases.py, as the library of ONE commit computes them on a GPU machine.  The file is the record of that commit's
results; tests/test_search_forms_gpu.py compares later commits with it bit for bit and never regenerates it.

    PANN_LIBRARY=/path/to/that/commit's/libpann.so python tests/golden/make_search_forms.py --commit <hash> [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import search_form_cases as sf  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the loaded library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "search_forms_v1.npz"))
    a = ap.parse_args()
    w = sf.World()
    rec = sf.record(w)
    w.close()
    rec["commit"] = np.frombuffer(a.commit.encode(), np.uint8)
    np.savez_compressed(a.out, **rec)
    print(f"{len(rec) - 1} arrays of {len(sf.cases())} cases from {a.commit} -> {a.out}")


if __name__ == "__main__":
    main()
