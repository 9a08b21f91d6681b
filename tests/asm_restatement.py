"""PETSc's additive Schwarz (PCASM) on one rank, restated in numpy.

Subdomains: the non-overlapping sets are bjacobi's contiguous row ranges (what
PCASMCreateSubdomains gives without a graph partitioner); overlap k runs
MatIncreaseOverlap_SeqAIJ's round k times -- every column index stored in the rows the previous
round added joins the set (round 1: the rows of the range).  Growth follows the row structure
only: directed, stored zeros count.  Each set ends sorted ascending.

Local problems: A_b = M[I_b, I_b] (entries with a column outside I_b dropped), factored by
ILU(levels) in that order -- PCILUk of tests/iluk_restatement.py.

Application, with R_b selecting I_b and R_b0 the same with the non-owned rows zeroed:
restrict  y = sum_b R_b0^T A_b^-1 R_b x;  basic  R_b on both sides;  interpolate  R_b0 on the
input, R_b on the output;  none  R_b0 on both sides.  A row's contributions are summed from 0.0
in ascending block order.
"""
import numpy as np
import scipy.sparse as sp

from iluk_restatement import PCILUk, bjacobi_block_sizes

TYPES = ("restrict", "basic", "interpolate", "none")  # pls_get_asm_stats' type 0..3


def subdomains(M, nblocks, overlap):
    """(bounds of the owned ranges, [sorted int32 rows of I_b])."""
    M = sp.csr_matrix(M)
    n = M.shape[0]
    rp, ci = M.indptr, M.indices
    bounds = np.concatenate([[0], np.cumsum(bjacobi_block_sizes(n, nblocks))]).astype(np.int64)
    sets = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        inside = np.zeros(n, dtype=bool)
        inside[lo:hi] = True
        front = np.arange(lo, hi)
        for _ in range(int(overlap)):
            if front.size == 0:
                break
            cols = np.unique(np.concatenate([ci[rp[r]:rp[r + 1]] for r in front]))
            front = cols[~inside[cols]]
            inside[front] = True
        sets.append(np.flatnonzero(inside).astype(np.int32))
    return bounds, sets


class PCASM:
    type = "asm"

    def __init__(self, M, nblocks, overlap=1, asm_type="restrict", k=0, fast=False):
        M = sp.csr_matrix(M)
        M.sort_indices()
        n = M.shape[0]
        if not 1 <= int(nblocks) <= n:
            raise ValueError("pc_asm_blocks out of range")
        self.n, self.nblocks, self.overlap, self.asm_type = n, int(nblocks), int(overlap), asm_type
        self.mask_in = asm_type in ("interpolate", "none")
        self.mask_out = asm_type in ("restrict", "none")
        self.bounds, self.rows = subdomains(M, self.nblocks, self.overlap)
        self.own = [(r >= lo) & (r < hi) for r, lo, hi in zip(self.rows, self.bounds[:-1], self.bounds[1:])]
        self.subs = [PCILUk(M[r][:, r].tocsr(), k, fast) for r in self.rows]
        self.ptr = np.concatenate([[0], np.cumsum([r.size for r in self.rows])]).astype(np.int64)
        self.nnz = sum(s.nnz for s in self.subs)
        self.max_row = max(s.max_row for s in self.subs)
        self.writes = None  # contributions every row received in the last apply

    def stats(self, fused):
        return (self.nblocks, self.overlap, TYPES.index(self.asm_type), int(self.ptr[-1]),
                int(np.diff(self.ptr).max()), int(fused))

    def apply(self, x):
        x = np.asarray(x, dtype=np.float64)
        y = np.zeros(self.n, dtype=np.float64)
        writes = np.zeros(self.n, dtype=np.int64)
        for s, rows, own in zip(self.subs, self.rows, self.own):  # ascending block order
            xb = x[rows]
            if self.mask_in:
                xb = np.where(own, xb, 0.0)
            yb = s.apply(xb)
            sel = own if self.mask_out else np.ones(rows.size, dtype=bool)
            y[rows[sel]] = y[rows[sel]] + yb[sel]
            writes[rows[sel]] += 1
        self.writes = writes
        return y
