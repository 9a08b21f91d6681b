"""The phase rule of the reduced outer layout with wide reuse rows (tests/reuse_wide_restatement.py),
on the CPU: the hand-built systems are what the GPU tests take them for, every remaining entry of
a wide reuse row stays on the lane it has in A, phase 0 is the layout without the rule, and the
stored lengths follow from the lanes' entry counts.  tests/test_gpu_reuse_wide.py pins the same
numbers against the device layout's bytes().
"""
import numpy as np
import pytest

import reuse_wide_restatement as W
import spmv_layout_restatement as R

CASES = [1160, 1152]  # ns: A's 64-row groups cut 8 rows off M's, and the same cuts


def _ms(A, ns):
    return np.diff(A[:, :ns].tocsr().indptr)


@pytest.mark.parametrize("ns", CASES)
def test_every_remaining_entry_keeps_its_lane(ns):
    A, ns, nf, np_ = W.wide_system(ns)
    Rd = W.reduced(A, ns)
    rp = A.indptr.astype(np.int64)
    j_full = Rd.entry_idx - rp[Rd.entry_row]           # the entry's place in the full row
    lpr = Rd.lanes[Rd.entry_row]
    assert np.array_equal(Rd.entry_sub, j_full % lpr)
    # a lane's entries are every lpr-th of the row, in order: its places count up from 0
    order = np.lexsort((j_full, Rd.entry_sub, Rd.entry_row))
    r, s, k = Rd.entry_row[order], Rd.entry_sub[order], Rd.entry_k[order]
    new_lane = np.r_[True, (r[1:] != r[:-1]) | (s[1:] != s[:-1])]
    assert np.all(k[new_lane] == 0) and np.all(k[~new_lane] == k[np.nonzero(~new_lane)[0] - 1] + 1)
    # the stored lengths are the lanes' entry counts: count them from the full rows' lanes directly
    per_lane = {}
    for rr, ss in zip(Rd.entry_row.tolist(), Rd.entry_sub.tolist()):
        per_lane[(rr, ss)] = per_lane.get((rr, ss), 0) + 1
    _, plan = W.lanes_per_row(A, R.Options.from_pls(W.OPTIONS))
    longest = np.zeros(len(plan.slpr), dtype=np.int64)
    for (rr, ss), cnt in per_lane.items():
        sl = np.searchsorted(plan.sfirst, rr, side="right") - 1
        longest[sl] = max(longest[sl], cnt)
    assert np.array_equal(np.diff(Rd.sptr), 64 * ((longest + 7) & ~7))


@pytest.mark.parametrize("ns", CASES)
def test_phase_zero_is_the_plain_rule(ns):
    """Without wide reuse rows A' is the layout of the rows' remaining entries by entry j on lane
    j % lpr: spmv_layout_restatement's slice pointers for the matrix without those entries."""
    import scipy.sparse as sp
    A, ns, nf, np_ = W.wide_system(ns)
    Rd = W.reduced(A, ns, reuse_wide=False)
    assert Rd.wide_rows == 0 and Rd.lane_rows > 0
    keep = np.ones(A.nnz, dtype=bool)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    keep[(Rd.kind[rows] > 0) & (A.indices < ns)] = False
    B = sp.csr_matrix((A.data[keep], (rows[keep], A.indices[keep])), shape=A.shape)
    _, plan = W.lanes_per_row(A, R.Options.from_pls(W.OPTIONS))  # (A's plan, not B's)
    assert np.array_equal(Rd.sptr, R._slice_ptr(np.diff(B.indptr).astype(np.int64), plan))
    # and with them the wide rows store less
    assert W.reduced(A, ns).stored < Rd.stored


def test_the_offset_case_is_what_the_gpu_test_takes_it_for():
    A, ns, nf, np_ = W.wide_system(1160)
    o = R.Options.from_pls(W.OPTIONS)
    la, planA = W.lanes_per_row(A, o)
    lm, planM = W.lanes_per_row(A[ns:, :ns], o)
    assert ns % 64 == 8 and (A.shape[0] - ns) % 64 == 20
    fp = np.arange(A.shape[0] - ns)
    # M: wide groups 0, 1 and 3, a lane-per-row group between them and a final partial group
    assert np.array_equal(lm > 1, (fp < 128) | ((fp >= 192) & (fp < 256)))
    # A cuts its groups 8 rows earlier: fp rows 56..119 and 184..247 are wide there (the group of
    # the last s rows and fp rows 0..55 is not: its first columns do not rise)
    assert np.array_equal(la[ns:] > 1, ((fp >= 56) & (fp < 120)) | ((fp >= 184) & (fp < 248)))
    assert set(la[la > 1]) == {8} and set(lm[lm > 1]) == {8}
    Rd = W.reduced(A, ns)
    wide = ((fp >= 56) & (fp < 120)) | ((fp >= 192) & (fp < 248))
    assert np.array_equal(Rd.kind[ns:] == 2, wide) and Rd.wide_rows == 120
    assert np.array_equal(Rd.kind[ns:] == 1, ((fp >= 128) & (fp < 184)) | (fp >= 256)) and Rd.lane_rows == 76
    assert not Rd.kind[:ns].any()
    ms = _ms(A, ns)[ns:]
    assert set((ms[wide] % 8).tolist()) == set(range(8))          # every residue mod 8
    assert ms[60] == 0 and ms[70] == 3 and ms[80] == 8 and wide[[60, 70, 80, 100]].all()
    assert A.indptr[ns + 101] - A.indptr[ns + 100] == ms[100] > 0  # a row without fp columns
    assert Rd.max_bases <= 4 and Rd.nsegs == 4


def test_aligned_case_has_wide_rows_too():
    A, ns, nf, np_ = W.wide_system(1152)
    Rd = W.reduced(A, ns)
    assert ns % 64 == 0 and Rd.wide_rows == 192 and Rd.lane_rows == 84
