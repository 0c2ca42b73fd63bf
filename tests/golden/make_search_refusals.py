"""Writes tests/golden/search_refusals_v1.json: the return code and the full pann_last_error() text of every row of
tests/search_refusal_cases.py, as the library of ONE commit answers them on a GPU machine.  The file is the record of that
commit's behaviour; tests/test_search_refusals_gpu.py compares later commits with it and never regenerates it.

    PANN_LIBRARY=/path/to/that/commit's/libpann.so python tests/golden/make_search_refusals.py --commit <hash> [--out FILE]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import search_refusal_cases as sr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the loaded library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "search_refusals_v1.json"))
    a = ap.parse_args()
    w = sr.World()
    table = {}
    for rid, entry, dev, faults in sr.rows():
        rc, msg = w.call(entry, dev, faults)
        table[rid] = {"rc": rc, "msg": msg}
    assert w.untouched(), "a refused call wrote to an output"
    w.close()
    with open(a.out, "w") as f:
        json.dump({"commit": a.commit, "rows": table}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(table)} rows from {a.commit} -> {a.out}")


if __name__ == "__main__":
    main()
