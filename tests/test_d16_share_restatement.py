"""The numpy restatement of the shared delta streams (tests/d16_share_restatement.py) pinned on the
CPU: the classes every case is there for, the format's invariants, and the decode through the
class addressing against the plain decode.  The device tests (tests/test_gpu_d16_share.py) compare
``spmv_layout()`` with the bytes restated here.
"""
import numpy as np
import pytest

import d16_share_restatement as D
import spmv_layout_restatement as R


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.id)
def test_format_invariants_and_decode(case):
    L, E, Sh = D.restated(case)
    ns = L.nslices
    Ls = np.diff(E.sptr) // 64
    assert L.d16 and len(Sh.C) == ns and len(Sh.cls) == ns * 64
    assert Sh.C.min() >= 1 and Sh.C.max() <= 64
    cls = Sh.cls.reshape(ns, 64).astype(np.int64)
    # ids 0..C-1, ordered by lowest member lane: lane 0 has class 0 and a lane's class is at most
    # one more than the largest before it
    assert np.all(cls[:, 0] == 0)
    assert np.all(cls.max(axis=1) + 1 == Sh.C)
    assert np.all(cls[:, 1:] <= np.maximum.accumulate(cls, axis=1)[:, :-1] + 1)
    assert np.array_equal(np.diff(Sh.dptr), Sh.C * Ls)
    assert np.all(Sh.dptr % 8 == 0)  # every pack is 16-B aligned
    assert Sh.bytes == L.bytes() - 2 * (L.stored - Sh.dstored) + 72 * ns + 8
    assert Sh.bytes_low == Sh.bytes - 4 * L.stored
    plain, shared = D.lane_columns(E), D.lane_columns(E, Sh)
    assert plain.keys() == shared.keys()
    for Lv in plain:
        assert np.array_equal(plain[Lv][1], shared[Lv][1])
    # two lanes of a slice are in one class exactly when their plain streams are equal
    for Lv, (S, d) in D._lane_streams(E).items():
        for i in range(0, len(S), max(1, len(S) // 16)):  # a sample of the slices, all pairs of lanes
            same_stream = (d[i][:, None, :] == d[i][None, :, :]).all(axis=2)
            same_class = cls[S[i]][:, None] == cls[S[i]][None, :]
            assert np.array_equal(same_stream, same_class)


@pytest.mark.parametrize("case", [c for c in D.CASES if c.expect_C], ids=lambda c: c.id)
def test_hand_built_classes(case):
    assert tuple(D.restated(case)[2].C) == case.expect_C


def test_all_class_matrix_is_the_plain_stream():
    """C = 64 with cls = lane is the plain stream: same deltas at the same places."""
    L, E, Sh = D.restated(D.BY_ID["classes-320"])
    base, dbase = int(E.sptr[4]), int(Sh.dptr[4])
    n = int(E.sptr[5] - E.sptr[4])
    assert Sh.C[4] == 64 and np.array_equal(Sh.cls[256:320], np.arange(64))
    assert np.array_equal(Sh.dls[dbase:dbase + n], E.dl[base:base + n])


def test_short_last_slice_shares_the_zero_class():
    """Rows 64..99 and 28 lanes without a row: the single-entry row 70 and the empty lanes hold
    the all-zero stream and share class 1; the last row (two entries) has a class of its own."""
    _, _, Sh = D.restated(D.BY_ID["short-last-slice"])
    c = Sh.cls[64:128]
    assert c[70 - 64] == 1 and np.all(c[36:] == 1)
    assert c[99 - 64] == 2 and np.all(np.delete(c[:35], 70 - 64) == 0)


def test_padded_twins_land_in_two_classes():
    _, E, Sh = D.restated(D.BY_ID["padded-twins"])
    assert np.array_equal(Sh.cls[:64], np.arange(64) % 2)
    # ... though their deltas agree as far as the shorter row goes
    d = D._lane_streams(E)[8][1][0]
    assert np.array_equal(d[0][:2], d[1][:2]) and d[0][2] == 1 and d[1][2] == 0


def test_synthetic_classes():
    """2-D N=24 (ns = nf = 4802, np = 625).  The s- and f-rows have fixed offset stencils in the s
    and f column blocks, but their pressure columns start at ns + nf + floor(i np / ns) + d: the
    step from the last f column to the first p column changes from row to row, and at this size
    it fits a 16-bit delta (it becomes a segment base, the same for every row, only above 65535:
    ns beyond that, as in the 3-D N=59 system).  So a slice's rows share a stream only in pairs
    that have the same floor: C between 50 and 64 on the lane-per-row slices, none at 1, few
    deltas saved.  The case is here for the irregular end of the format -- many classes, 8-lane
    pressure slices -- and "wide", "ramp" and "classes-320" cover the small C values."""
    L, _, Sh = D.restated(D.BY_ID["synthetic-2d-24"])
    lpr = L.plan.slpr
    print("slices", L.nslices, "lane-per-row", int((lpr == 1).sum()), "C histogram",
          dict(zip(*np.unique(Sh.C, return_counts=True))), "deltas", Sh.dstored, "of", L.stored)
    assert L.plan.rowmap is None
    one = Sh.C[lpr == 1]
    assert one.min() >= 50 and (one < 64).sum() >= 0.9 * len(one)
    assert (lpr == 8).any() and (Sh.C[lpr == 8] < 64).any() and (Sh.C[lpr == 8] > 1).all()
    assert 0.8 * L.stored < Sh.dstored < L.stored


def test_cases_reach_their_branch():
    """wide: 8 lanes per row, one class; sorted: a row map; bases-8: nsegs 8; ramp: 1..5 groups of 8."""
    L, _, Sh = D.restated(D.BY_ID["wide"])
    assert (L.plan.slpr == 8).any() and np.all(Sh.C[L.plan.slpr == 8] == 1)
    L, _, Sh = D.restated(D.BY_ID["sorted"])
    assert L.plan.rowmap is not None and (L.plan.slpr == 2).any() and Sh.shared_slices == L.nslices
    L, _, Sh = D.restated(D.BY_ID["bases-8"])
    assert L.nsegs == 8 and L.max_bases == 5 and Sh.shared_slices > 0
    L, E, Sh = D.restated(D.BY_ID["ramp"])
    assert tuple(np.diff(E.sptr) // 512) == (1, 2, 3, 4, 5) and np.all(Sh.C == 3)


def test_distinct_streams_save_nothing():
    """The matrix the auto rule declines: 64 classes, so the shared layout is 72 + 8 bytes larger."""
    L = R.layout(D.distinct_64(), {})
    Sh = D.share(L, L.encode())
    assert tuple(Sh.C) == (64,) and Sh.bytes == L.bytes() + 80


def test_a_wrong_class_changes_the_decode():
    """The decode check can fail: moving one lane of a C = 2 slice into the other class changes
    its columns."""
    _, E, Sh = D.restated(D.BY_ID["padded-twins"])
    bad = D.Shared(Sh.C, Sh.cls.copy(), Sh.dptr, Sh.dls, Sh.bytes, Sh.bytes_low)
    bad.cls[3] = 0
    assert not np.array_equal(D.lane_columns(E)[8][1], D.lane_columns(E, bad)[8][1])
