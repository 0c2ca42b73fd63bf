"""Cases shared by the label-predicate tests (DESIGN.md "Label predicates"): label arrays and predicates at the shapes of
tests/masked_cases.py -- N = 3001, so the last bitmap word has 25 live bits, and NQ = 8 queries.  Plain Python: nothing here needs
a GPU.  tests/test_label_cases_cpu.py asserts that every case is what it claims to be (so that no device test passes
vacuously); the device tests expand a case with label_allow and compare with tests/masked_ref.py on that mask, and with the
device's own bitmap entry points on the packed rows.

A case is (labels uint32 (N,), kind, preds): preds a pair (a, b) -- one predicate for the batch -- or an (NQ, 2) uint32 array.

    mask reproductions   random 32-bit labels whose bit 3 is a mask of masked_cases, searched with ANY a = 1 << 3: the results
                         are those of the existing masked cases, whose references apply unchanged
    tenant               low byte = a tenant in 0..3, bit 31 = a tombstone on about 10 % of the points, the bits between random;
                         MATCH a = 0x800000FF, b = q % 4: query q sees the live points of tenant q % 4
    match_all / none     MATCH a = 0, b = 0 allows everything; a = 0xFF, b = 0x1FF cannot hold (b has a bit outside a)
    any_zero             ANY a = 0 allows nothing
    range_*              labels uniform over the full unsigned range, with one label forced onto each bound of each window.
                         straddle: lo < 2^31 <= hi, so a signed compare answers differently; high: a window entirely above
                         2^31; empty: a > b; rows: eight different windows, each with lo < 2^31 <= hi
"""
import numpy as np

import masked_cases as mc

N, NQ = mc.N, mc.NQ
LAST_WORD = np.arange(N - 25, N)          # ids 2976..3000: the live bits of the last bitmap word
MASK_BIT = np.uint32(1 << 3)
MASK_KINDS = ["rand50", "rand5", "zeros", "ones", "only_start", "start_off"]

_cache = {}


def mask_labels(mkind, layout=mc.KIND_LAYOUT, starts=(0,)):
    """random labels whose bit 3 is mask(mkind): with ANY (1 << 3, 0) they reproduce the masked case"""
    m = mc.mask(mkind, layout, starts)
    assert m.ndim == 1
    rng = np.random.default_rng(100 + MASK_KINDS.index(mkind))
    lab = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    return np.where(m, lab | MASK_BIT, lab & ~MASK_BIT).astype(np.uint32)


MASK_PRED = (int(MASK_BIT), 0)


def tenant_labels():
    if "tenant" not in _cache:
        rng = np.random.default_rng(211)
        lab = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32) & np.uint32(0x7FFFFF00)
        lab |= rng.integers(0, 4, N).astype(np.uint32)
        lab |= (rng.random(N) < 0.1).astype(np.uint32) << np.uint32(31)
        lab[N - 5:] = [0x00000001, 0x00001200, 0x80000001, 0x00345602, 0x7FFFFF03]   # the last word: live points of tenants 0..3, a dead one
        _cache["tenant"] = lab
    return _cache["tenant"]


TENANT_PREDS = np.array([[0x800000FF, q % 4] for q in range(NQ)], np.uint32)

RANGE_STRADDLE = (0x60000000, 0xA0000000)
RANGE_HIGH = (0xC0000000, 0xF0000000)
RANGE_EMPTY = (0x90000000, 0x70000000)
RANGE_ROWS = np.array([[0x10000000 + 0x08000000 * q, 0x80000000 + 0x0C000000 * q] for q in range(NQ)], np.uint32)


def range_labels():
    """uniform over [0, 2^32); every bound of every window above is the label of some point, and the last word holds both
    verdicts of every window"""
    if "range" not in _cache:
        rng = np.random.default_rng(223)
        lab = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
        bounds = [*RANGE_STRADDLE, *RANGE_HIGH, *RANGE_EMPTY, *RANGE_ROWS.reshape(-1).tolist()]
        at = rng.choice(N - 25, len(bounds), replace=False)
        lab[at] = np.array(bounds, np.uint32)
        lab[N - 4:] = [0x00000005, 0x7FFFFFFF, 0x80000000, 0xFFFFFFF0]          # outside / inside every non-empty window
        lab[N - 6:N - 4] = [0xD0000000, 0x50000000]
        _cache["range"] = lab
    return _cache["range"]


# name -> (labels, kind, preds, claim); claim: "some" (a share strictly between 0 and 1 for every predicate), "all", "none"
def cases():
    c = {}
    for mk in MASK_KINDS:
        claim = {"zeros": "none", "ones": "all"}.get(mk, "some")
        c["mask-" + mk] = (mask_labels(mk), "any", MASK_PRED, claim)
    c["tenant"] = (tenant_labels(), "match", TENANT_PREDS, "some")
    c["tenant-shared"] = (tenant_labels(), "match", (0x800000FF, 2), "some")
    c["match-all"] = (tenant_labels(), "match", (0, 0), "all")
    c["match-none"] = (tenant_labels(), "match", (0xFF, 0x1FF), "none")
    c["any-zero"] = (tenant_labels(), "any", (0, 0), "none")
    c["range-straddle"] = (range_labels(), "range", RANGE_STRADDLE, "some")
    c["range-high"] = (range_labels(), "range", RANGE_HIGH, "some")
    c["range-empty"] = (range_labels(), "range", RANGE_EMPTY, "none")
    c["range-rows"] = (range_labels(), "range", RANGE_ROWS, "some")
    return c


CASES = cases()
# the cases whose every predicate has both verdicts among the ids of the last bitmap word
LAST_WORD_BOTH = ["mask-rand50", "mask-rand5", "tenant", "tenant-shared", "range-straddle", "range-high", "range-rows"]
# RANGE cases on which a signed compare selects another set.  range-high is not among them: a window entirely above 2^31 maps to
# negative numbers in the same order, so signed and unsigned agree there -- it is the control that the others differ by the sign alone
SIGNED_DIFFERS = ["range-straddle", "range-empty", "range-rows"]
PER_QUERY = [name for name, c in CASES.items() if np.asarray(c[2]).ndim == 2]


def loop_allow(labels, kind, a, b):
    """the table of the issue, one point at a time in Python integers"""
    out = np.zeros(len(labels), bool)
    for i, l in enumerate(labels.tolist()):
        if kind == "any":
            out[i] = (l & a) != 0
        elif kind == "match":
            out[i] = (l & a) == b
        else:
            out[i] = a <= l <= b
    return out


def signed_range_allow(labels, a, b):
    """what a kernel with a SIGNED compare would compute for a RANGE predicate"""
    s = np.asarray(labels, np.uint32).view(np.int32)
    sa, sb = np.array([a, b], np.uint32).view(np.int32)
    return (s >= sa) & (s <= sb)


def preds_rows(preds):
    """(a, b) or (NQ, 2) -> the NQ per-query predicates as an (NQ, 2) uint32 array"""
    p = np.asarray(preds, np.uint32)
    return np.ascontiguousarray(np.broadcast_to(p, (NQ, 2)))
