"""The label-predicate cases of tests/label_cases.py are what they claim to be, shown without a GPU: label_allow (the host helper
the device tests expand every case with) agrees with a plain loop over the table of the issue, the selected shares are what each
case says, the last bitmap word sees both verdicts, a signed compare would answer the RANGE cases differently, and per-query
predicates give pairwise different rows.  The mask reproductions select exactly the masks of tests/masked_cases.py."""
import numpy as np
import pytest

import label_cases as lc
import masked_cases as mc
from parlayann_amd.index import label_allow, label_preds, pred_kind

NAMES = list(lc.CASES)


def _rows(name):
    """the case's boolean rows, (NQ, N), one per query"""
    labels, kind, preds, _ = lc.CASES[name]
    return np.broadcast_to(label_allow(labels, kind, preds), (lc.NQ, lc.N))


@pytest.mark.parametrize("name", NAMES)
def test_label_allow_equals_a_plain_loop(name):
    labels, kind, preds, _ = lc.CASES[name]
    got = label_allow(labels, kind, preds)
    p = np.asarray(preds)
    assert got.dtype == np.bool_ and got.shape == ((lc.N,) if p.ndim == 1 else (lc.NQ, lc.N))
    for q, (a, b) in enumerate(p.reshape(-1, 2).tolist()):
        np.testing.assert_array_equal(got if p.ndim == 1 else got[q], lc.loop_allow(labels, kind, a, b), err_msg=f"{name} q{q}")
    # kind codes and names are the same thing
    np.testing.assert_array_equal(got, label_allow(labels, pred_kind(kind), preds))


@pytest.mark.parametrize("name", NAMES)
def test_selected_share_is_what_the_case_claims(name):
    claim = lc.CASES[name][3]
    cnt = _rows(name).sum(axis=1)
    if claim == "some":
        assert (cnt > 0).all() and (cnt < lc.N).all()
    elif claim == "all":
        assert (cnt == lc.N).all()
    else:
        assert claim == "none" and (cnt == 0).all()


@pytest.mark.parametrize("name", lc.LAST_WORD_BOTH)
def test_both_verdicts_occur_in_the_last_word(name):
    last = _rows(name)[:, lc.LAST_WORD]
    assert lc.LAST_WORD[0] == 2976 and lc.LAST_WORD[-1] == 3000 and lc.N % 32 == 25
    assert last.any(axis=1).all() and (~last).any(axis=1).all()


@pytest.mark.parametrize("mkind", lc.MASK_KINDS)
def test_mask_reproductions_select_the_masks_of_masked_cases(mkind):
    labels, kind, preds, _ = lc.CASES["mask-" + mkind]
    np.testing.assert_array_equal(label_allow(labels, kind, preds), mc.mask(mkind, mc.KIND_LAYOUT))
    assert len(np.unique(labels >> np.uint32(4))) > lc.N // 2          # the other bits are random, not copies of the mask


def test_tenant_labels_are_as_described():
    lab = lc.tenant_labels()
    assert set(np.unique(lab & np.uint32(0xFF)).tolist()) == {0, 1, 2, 3}
    dead = (lab >> np.uint32(31)).astype(bool)
    assert 0.05 < dead.mean() < 0.15
    rows = _rows("tenant")
    for q in range(lc.NQ):
        np.testing.assert_array_equal(rows[q], ((lab & np.uint32(0xFF)) == q % 4) & ~dead)
    assert rows[:, dead].sum() == 0


def test_range_cases_are_as_described():
    lab = lc.range_labels()
    windows = [lc.RANGE_STRADDLE, lc.RANGE_HIGH, lc.RANGE_EMPTY, *lc.RANGE_ROWS.tolist()]
    for a, b in windows:
        assert (lab == a).any() and (lab == b).any()                   # a label on each bound: the ends are inclusive
    for a, b in [lc.RANGE_STRADDLE, *lc.RANGE_ROWS.tolist()]:
        assert a < 2 ** 31 <= b
        sel = label_allow(lab, "range", (a, b))
        assert sel[lab == a].all() and sel[lab == b].all()
    assert lc.RANGE_HIGH[0] > 2 ** 31 and lc.RANGE_EMPTY[0] > lc.RANGE_EMPTY[1]
    assert (lab < 2 ** 31).mean() > 0.4 and (lab >= 2 ** 31).mean() > 0.4   # the full unsigned range is in use
    assert len({tuple(w) for w in lc.RANGE_ROWS.tolist()}) == lc.NQ


@pytest.mark.parametrize("name", lc.SIGNED_DIFFERS)
def test_a_signed_compare_selects_a_different_set(name):
    labels, kind, preds, _ = lc.CASES[name]
    assert kind == "range"
    for a, b in np.asarray(preds).reshape(-1, 2).tolist():
        assert (label_allow(labels, kind, (a, b)) != lc.signed_range_allow(labels, a, b)).any()


def test_the_window_above_2_31_is_the_control():
    """signed and unsigned order agree on labels >= 2^31 among themselves: the other RANGE cases differ by the sign alone"""
    labels, kind, preds, _ = lc.CASES["range-high"]
    sel = label_allow(labels, kind, preds)
    assert sel.any() and (labels[sel] >= 2 ** 31).all()
    np.testing.assert_array_equal(sel, lc.signed_range_allow(labels, *preds))


@pytest.mark.parametrize("name", lc.PER_QUERY)
def test_per_query_predicates_give_pairwise_different_rows(name):
    rows = _rows(name)
    want = 4 if name == "tenant" else lc.NQ                            # tenant: q and q + 4 share a tenant, on purpose
    assert len({r.tobytes() for r in rows}) == want
    p = lc.CASES[name][2]
    assert p.shape == (lc.NQ, 2) and len({tuple(x) for x in p.tolist()}) == want


def test_label_allow_argument_forms():
    lab = lc.tenant_labels()
    p, single = label_preds((1, 2))
    assert single and p.dtype == np.uint32 and p.shape == (1, 2) and p.flags.c_contiguous
    p, single = label_preds(np.array([[1, 2]], np.int64))
    assert not single and p.shape == (1, 2)
    assert label_allow(lab, "any", np.array([[1, 0]], np.uint32)).shape == (1, lc.N)
    with pytest.raises(ValueError):
        label_allow(lab, "between", (0, 1))
    with pytest.raises(ValueError):
        label_allow(lab, "any", (1, 2, 3))
    with pytest.raises(ValueError):
        label_allow(lab, "any", (-1, 0))
    with pytest.raises(ValueError):
        label_allow(lab, "any", (1 << 32, 0))
