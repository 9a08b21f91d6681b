"""The reduced outer layout A' of the coupling reuse with wide reuse rows (option pls.reuse_wide;
csrc/runtime.cpp: build_coupling; csrc/kernels.hip: d16_first, k_d16_slice_len, k_d16_count,
k_d16_fill), restated in numpy on top of tests/spmv_layout_restatement.py.

The rules, as pinned here (A in field-major order, rows and columns [0, ns) the s field, sorted
columns; M = A[ns:, :ns] the block PC's coupling block):

* both matrices get their plain slice plans (d16_plan; a sorted plan anywhere: no reuse at all).
  lanes_A[r], lanes_M[r] are the lanes per row of the slice holding row r (M's rows shifted by ns).
* an fp row r >= ns is a lane-per-row reuse row when lanes_A[r] == lanes_M[r] == 1, and, with
  reuse_wide, a wide reuse row when lanes_A[r] == lanes_M[r] > 1.
* a reuse row of either kind loses its m_s leading entries (the columns < ns) in A'; every other
  row keeps all of its entries.
* phase rule: a row of lpr lanes that lost m entries has phase = m % lpr; lane ``sub`` takes the
  remaining entries j' = 0, 1, ... with (j' + phase) % lpr == sub, in order.  That is the lane
  entry m + j' has in the full row (entry j on lane j % lpr).
* A' keeps A's slice plan; a slice stores 64 * roundup8(the most entries one of its lanes holds);
  segment bases per lane by k_d16_count's rule (first entry, column gap above 65535).
* ``Reduced.bytes`` is DevSELL::bytes() of A' with a plain delta stream (pls.d16_share 0).

``wide_system(ns)`` builds the hand-made systems of the tests: fp rows whose s-part is a run of
consecutive s columns (wide 64-row groups where the runs start 5 columns apart, a lane-per-row
group where they start 1 apart), s-part lengths over every residue mod 8, one empty and two short
s-parts, one row without fp columns, and a final partial group.  OPTIONS (pls.d16_sigma 0) keeps
the plans plain whatever the padding: the sorted plan would end the reuse.
"""
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import spmv_layout_restatement as R

OPTIONS = {"pls.d16_sigma": "0"}


def _csr(A):
    A = sp.csr_matrix(A)
    if not A.has_sorted_indices:
        A = A.sorted_indices()
    return A


def lanes_per_row(M, o):
    """Lanes per row of M's plain plan (any CSR shape); None when the plan is a sorted one."""
    M = _csr(M)
    n = M.shape[0]
    plan = R.d16_plan(n, M.indptr.astype(np.int64), M.indices.astype(np.int64), o)
    if plan.rowmap is not None:
        return None, plan
    lanes = np.zeros(n, dtype=np.int64)
    for s, l in enumerate(plan.slpr):
        lanes[plan.sfirst[s]:min(plan.sfirst[s + 1], n)] = l
    return lanes, plan


@dataclass
class Reduced:
    kind: np.ndarray        # per row: 0 keeps its entries, 1 lane-per-row reuse row, 2 wide reuse row
    skip: np.ndarray        # per row: leading entries A' leaves out
    lanes: np.ndarray       # per row: lanes per row in A's plan
    entry_row: np.ndarray   # per remaining entry (CSR order): its row,
    entry_idx: np.ndarray   # its place in A's arrays,
    entry_sub: np.ndarray   # the lane of the row that holds it
    entry_k: np.ndarray     # and its place in that lane's stream
    sptr: np.ndarray        # slice pointers of A'
    max_bases: int
    nsegs: int
    nslices: int

    @property
    def stored(self):
        return int(self.sptr[-1])

    @property
    def wide_rows(self):
        return int((self.kind == 2).sum())

    @property
    def lane_rows(self):
        return int((self.kind == 1).sum())

    @property
    def bytes(self):
        # (as Layout.bytes() of a D16 layout without row map, triples or relabelling: the last 8 is
        # the empty triple part's slice pointer)
        return self.stored * 10 + self.nslices * (64 * 4 * self.nsegs + 20) + 8 + 8


def reduced(A, ns, options=None, reuse_wide=True):
    """A' of the square CSR matrix A (field-major, s first); None where no row is a reuse row."""
    o = options if isinstance(options, R.Options) else R.Options.from_pls(OPTIONS if options is None else options)
    A = _csr(A)
    n = A.shape[0]
    rp, ci = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    la, planA = lanes_per_row(A, o)
    lm_fp, _ = lanes_per_row(A[ns:, :ns], o)
    if la is None or lm_fp is None:
        return None
    lm = np.zeros(n, dtype=np.int64)
    lm[ns:] = lm_fp
    lens = np.diff(rp)
    row_of = np.repeat(np.arange(n), lens)
    ms = np.bincount(row_of[ci < ns], minlength=n)  # sorted columns: the s entries lead the row
    kind = np.where((la == 1) & (lm == 1), 1, np.where(reuse_wide & (la > 1) & (la == lm), 2, 0))
    kind[:ns] = 0
    if not kind.any():
        return None
    skip = np.where(kind > 0, ms, 0)
    phase = skip % la
    # the remaining entries, their lanes and places
    left = lens - skip
    erow = np.repeat(np.arange(n), left)
    jp = np.arange(len(erow)) - np.repeat(np.cumsum(left) - left, left)
    eidx = rp[erow] + skip[erow] + jp
    l = la[erow]
    sub = (jp + phase[erow]) % l
    first = (sub - phase[erow]) % l
    k = (jp - first) // l
    # slice lengths: the most entries one lane of the slice holds
    sl_of_row = np.searchsorted(planA.sfirst, np.arange(n), side="right") - 1
    nsl = len(planA.slpr)
    longest = np.zeros(nsl, dtype=np.int64)
    np.maximum.at(longest, sl_of_row[erow], k + 1)
    sptr = np.concatenate(([0], np.cumsum(64 * R._up8(longest)))).astype(np.int64)
    # segment bases per lane
    order = np.lexsort((k, sub, erow))
    r_, s_, k_, c_ = erow[order], sub[order], k[order], ci[eidx][order]
    gap = np.zeros(len(c_), dtype=np.int64)
    gap[1:] = c_[1:] - c_[:-1]
    newbase = (k_ == 0) | (gap > R.DELTA_MAX) | (gap <= 0)
    lane_id = r_ * 64 + s_
    bases = np.bincount(np.unique(lane_id, return_inverse=True)[1], weights=newbase) if len(c_) else np.zeros(1)
    h = int(bases.max())
    if h > R.D16_SEG_MAX:
        return None
    nsegs = R.D16_SEG if (h <= R.D16_SEG and o.d16_segs <= R.D16_SEG) else R.D16_SEG_MAX
    return Reduced(kind, skip, la, erow, eidx, sub, k, sptr, h, nsegs, nsl)


def wide_system(ns=1160, seed=3):
    """(A, ns, nf, np): the hand-built system.  276 fp rows; fp row i has the s columns
    start_i .. start_i + len_i - 1 and fp columns around its diagonal."""
    rng = np.random.default_rng(seed)
    nfp = 64 * 4 + 20
    n = ns + nfp
    rows, cols = [], []
    for r in range(ns):  # s rows: 8 entries around the diagonal, lane-per-row
        for c in range(r - 3, r + 5):
            if 0 <= c < ns:
                rows.append(r)
                cols.append(c)
    special_len = {60: 0, 70: 3, 80: 8, 90: 16, 200: 5, 210: 0}
    for i in range(nfp):
        if i < 128:
            start = 5 * i                      # wide in M: runs start 5 columns apart
        elif i < 192:
            start = 640 + (i - 128)            # lane-per-row in M: runs start 1 apart
        else:
            start = 700 + 5 * (i - 192)        # wide again, then the final partial group
        ln = special_len.get(i, 17 + i % 16)
        assert start + ln <= ns
        for c in range(start, start + ln):
            rows.append(ns + i)
            cols.append(c)
        if i == 100:                           # a row without fp columns
            continue
        w = 12 + (i * 7) % 17
        for c in range(max(0, i - w), min(nfp, i + w + 1)):
            rows.append(ns + i)
            cols.append(ns + c)
    rows, cols = np.array(rows), np.array(cols)
    vals = rng.standard_normal(len(rows))
    vals[rows == cols] = 4.0 + np.abs(vals[rows == cols])
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    nf = nfp // 2
    return A, ns, nf, nfp - nf
