"""CPU-side pieces of the range ground truth: the RangeGroundTruth file format (types.h:119-140, written by
compute_range_groundtruth.cpp:64-88), range recall (check_range_recall.h:37-53) and the no-fallback rule."""
import struct

import numpy as np
import pytest

from parlayann_amd import DeviceIndex, PannError, _capi, io
from parlayann_amd.recall import range_recall


def _hand_bytes(rows):
    """[n:i32][num_matches:i32][sizes: n x i32][ids: num_matches x i32], little endian, built field by field"""
    flat = [i for r in rows for i in r]
    b = struct.pack("<ii", len(rows), len(flat))
    b += b"".join(struct.pack("<i", len(r)) for r in rows)
    b += b"".join(struct.pack("<i", i) for i in flat)
    return b


def test_range_gt_file_round_trip_against_hand_built_bytes(tmp_path):
    rows = [[3, 9, 27], [], [0], [], [], [5, 6, 7, 8, 2000000000]]           # empty rows in the middle and in a run
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    ids = np.array([i for r in rows for i in r], np.uint32)
    io.write_range_gt(tmp_path / "a.gt", off, ids)
    assert (tmp_path / "a.gt").read_bytes() == _hand_bytes(rows)
    (tmp_path / "b.gt").write_bytes(_hand_bytes(rows))
    o, i = io.read_range_gt(tmp_path / "b.gt")
    assert o.dtype == np.uint64 and i.dtype == np.uint32
    np.testing.assert_array_equal(o, off); np.testing.assert_array_equal(i, ids)
    # nothing at all, and only empty rows
    io.write_range_gt(tmp_path / "e.gt", np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    assert (tmp_path / "e.gt").read_bytes() == struct.pack("<ii", 0, 0)
    io.write_range_gt(tmp_path / "z.gt", np.zeros(4, np.uint64), np.zeros(0, np.uint32))
    assert (tmp_path / "z.gt").read_bytes() == _hand_bytes([[], [], []])
    o, i = io.read_range_gt(tmp_path / "z.gt")
    assert list(o) == [0, 0, 0, 0] and len(i) == 0


def test_range_gt_file_refuses_what_the_32_bit_header_cannot_hold(tmp_path):
    off = np.array([0, 2 ** 31], np.uint64)                       # refused from the offsets alone, before the ids are looked at
    with pytest.raises(ValueError, match="32-bit"):
        io.write_range_gt(tmp_path / "h.gt", off, np.zeros(1, np.uint32))
    off = np.array([0, 5, 2 ** 31 - 1], np.uint64)                # the largest count the header holds gets past that check
    with pytest.raises(ValueError, match="ids given"):
        io.write_range_gt(tmp_path / "h.gt", off, np.zeros(1, np.uint32))
    assert not (tmp_path / "h.gt").exists()
    with pytest.raises(ValueError):
        io.write_range_gt(tmp_path / "m.gt", np.array([0, 2], np.uint64), np.array([1], np.uint32))      # offsets and ids disagree
    (tmp_path / "t.gt").write_bytes(_hand_bytes([[1, 2], [3]])[:-4])                                     # truncated
    with pytest.raises(ValueError):
        io.read_range_gt(tmp_path / "t.gt")


def test_range_recall_hand_cases():
    PAD = 0xFFFFFFFF
    gt_off = np.array([0, 4, 4, 6, 6], np.uint64)                 # truth sizes 4, 0, 2, 0
    gt_ids = np.array([1, 5, 9, 12, 7, 8], np.uint32)
    res = np.array([[9, 1, 100, PAD],                             # 2 of 4, plus an id outside the truth: not counted
                    [4, PAD, PAD, PAD],                           # empty truth: left out of the pointwise mean
                    [8, 7, PAD, PAD],                             # 2 of 2, BFS order
                    [PAD, PAD, PAD, PAD]], np.uint32)
    cnt = np.array([3, 1, 2, 0], np.uint32)
    r = range_recall(res, cnt, gt_off, gt_ids)
    assert r["nonzero"] == 2 and r["total"] == 6 and r["reported"] == 6
    assert r["pointwise"] == pytest.approx((2 / 4 + 2 / 2) / 2)
    assert r["cumulative"] == pytest.approx(4 / 6)                # hits / total
    # a repeated id counts once; entries past the count are ignored
    r = range_recall(np.array([[7, 7, 8, 1]], np.uint32), np.array([2], np.uint32), np.array([0, 2], np.uint64), np.array([7, 8], np.uint32))
    assert r["pointwise"] == pytest.approx(0.5) and r["cumulative"] == pytest.approx(0.5) and r["reported"] == 1
    # everything found: exactly 1, never above
    r = range_recall(np.array([[8, 7, 99]], np.uint32), np.array([3], np.uint32), np.array([0, 2], np.uint64), np.array([7, 8], np.uint32))
    assert r["pointwise"] == 1.0 and r["cumulative"] == 1.0
    with pytest.raises(ValueError):
        range_recall(res, cnt, gt_off[:-1], gt_ids)


def test_new_entry_points_fail_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = _capi.load()
    assert lib.pann_device_count() == 0
    ix = DeviceIndex.__new__(DeviceIndex)                          # no handle can exist without a device
    ix._lib, ix._h = lib, None
    ix.n, ix.d, ix.max_degree, ix.dtype, ix.metric = 16, 8, 4, np.dtype(np.uint8), 0
    Q = np.zeros((4, 8), np.uint8)
    for call in (lambda: ix.bruteforce_range(Q, 1.0), lambda: ix.range_query(Q, radius=1.0, beam=10, max_results=8)):
        with pytest.raises(PannError) as e:
            call()
        assert e.value.code == 3 and "no HIP device" in str(e.value)     # PANN_ERR_NO_DEVICE: no numpy fallback
