"""ILU(k) as PETSc defines it (MatILUFactorSymbolic_SeqAIJ, natural ordering), restated in numpy.

Symbolic phase, the row-merge form: stored entries (stored zeros included) have
level 0; row i is merged with the U parts of its pivot rows p < i in ascending
order, lev(i, j) = min over pivots p < min(i, j) of lev(i, p) + lev(p, j) + 1
(the sum rule), and an entry is kept when its level is <= k.  The numeric phase
is the IKJ factorization on the kept pattern, and the solves run in CSR order --
the operations of oracle/csrc/oracle.c's ILU(0) in the same order, so level 0
is oracle.native.ILU0 bitwise (tests/test_iluk_restatement.py).

The loops over rows are Python; everything inside a row is a numpy call.  That is quick on blocks
of a few hundred rows.  For blocks of thousands of rows with hundreds of entries per row (3-D)
``fast=True`` takes two shortcuts, both pinned equal to the plain path by
tests/test_iluk_restatement.py: the levels from the same recursion run over levels instead of
rows (sparse products, symbolic_products), and the numeric phase and the solves by
oracle.native.ILU0 on the filled matrix (zeros stored in the new places) -- ILU(0) of that
matrix is the IKJ factorization on the kept pattern.
"""
import heapq

import numpy as np
import scipy.sparse as sp

from oracle.petsc import bjacobi_block_sizes

BIG = np.iinfo(np.int32).max


def symbolic_rowmerge(M, k):
    """(indptr int64, indices int32 sorted, levels int32) of the ILU(k) pattern of M."""
    M = sp.csr_matrix(M)
    M.sort_indices()
    n = M.shape[0]
    rp, ci = M.indptr, M.indices
    lev = np.full(n, BIG, dtype=np.int64)
    ucols, ulevs = [None] * n, [None] * n
    out_c, out_l, out_p = [], [], [0]
    for i in range(n):
        cols = ci[rp[i]:rp[i + 1]]
        if i not in cols:
            raise RuntimeError(f"ILU({k}): missing diagonal in row {i}")
        lev[cols] = 0
        touched = [cols]
        heap = [int(c) for c in cols if c < i]
        heapq.heapify(heap)
        while heap:
            p = heapq.heappop(heap)
            cand = lev[p] + ulevs[p] + 1      # lev(i, p) + lev(p, j) + 1 for the j > p of row p
            jj = ucols[p]
            keep = (cand <= k) & (cand < lev[jj])
            if not keep.any():
                continue
            jj, cand = jj[keep], cand[keep]
            for j in jj[(lev[jj] == BIG) & (jj < i)]:
                heapq.heappush(heap, int(j))
            lev[jj] = cand
            touched.append(jj)
        row = np.unique(np.concatenate(touched))
        rl = lev[row]
        lev[row] = BIG
        up = row > i
        ucols[i], ulevs[i] = row[up], rl[up]
        out_c.append(row)
        out_l.append(rl)
        out_p.append(out_p[-1] + row.size)
    return (np.asarray(out_p, dtype=np.int64), np.concatenate(out_c).astype(np.int32),
            np.concatenate(out_l).astype(np.int32))


def symbolic_products(M, k):
    """symbolic_rowmerge's result from the recursion over levels: with E_a the entries of level
    exactly a, an entry is of level <= m when it is stored or in the pattern of
    strict_lower(E_a) @ strict_upper(E_b) for some a + b + 1 <= m -- the pivot p < min(i, j) of
    the rule is the product's inner index."""
    M = sp.csr_matrix(M)
    n = M.shape[0]
    E = [sp.csr_matrix((np.ones(M.nnz, dtype=np.float32), M.indices, M.indptr), shape=M.shape)]
    if np.any(E[0].diagonal() == 0):
        raise RuntimeError(f"ILU({k}): missing diagonal in row {int(np.flatnonzero(E[0].diagonal() == 0)[0])}")
    known = E[0].copy()
    lower = [sp.tril(E[0], -1, format="csr")]
    upper = [sp.triu(E[0], 1, format="csr")]
    for m in range(1, min(k, n) + 1):
        new = None
        for a in range(m):
            prod = lower[a] @ upper[m - 1 - a]
            new = prod if new is None else new + prod
        new.data[:] = 1.0
        new = (new - new.multiply(known)).tocsr()
        new.eliminate_zeros()
        E.append(new)
        lower.append(sp.tril(new, -1, format="csr"))
        upper.append(sp.triu(new, 1, format="csr"))
        known = known + new
    lev = sum((e * float(a + 1) for a, e in enumerate(E)), sp.csr_matrix(M.shape, dtype=np.float32)).tocsr()
    lev.sort_indices()
    return lev.indptr.astype(np.int64), lev.indices.astype(np.int32), (lev.data - 1).astype(np.int32)


def filled_values(M, rp, ci):
    """M's values in the pattern (rp, ci) -- which contains M's -- zeros elsewhere."""
    M = sp.csr_matrix(M)
    M.sort_indices()
    v = np.zeros(ci.size, dtype=np.float64)
    for i in range(M.shape[0]):
        a, b = M.indptr[i], M.indptr[i + 1]
        v[rp[i] + np.searchsorted(ci[rp[i]:rp[i + 1]], M.indices[a:b])] = M.data[a:b]
    return v


def numeric_ikj(rp, ci, v):
    """In-place IKJ factorization on the pattern: (lu, diag positions, 1 / pivots).  Row i lives in
    a dense work vector while its pivot rows are subtracted; updates outside the row's pattern are
    dropped."""
    n = rp.size - 1
    lu = np.array(v, dtype=np.float64, copy=True)
    diag = np.empty(n, dtype=np.int64)
    dinv = np.zeros(n, dtype=np.float64)
    w = np.zeros(n, dtype=np.float64)
    inrow = np.zeros(n, dtype=bool)
    for i in range(n):
        a, b = rp[i], rp[i + 1]
        cols = ci[a:b]
        diag[i] = a + np.searchsorted(cols, i)
        w[cols] = lu[a:b]
        inrow[cols] = True
        for r in cols[:diag[i] - a]:
            pc = w[r]
            if pc != 0.0:
                mult = pc * dinv[r]
                w[r] = mult
                u0, u1 = diag[r] + 1, rp[r + 1]
                uc = ci[u0:u1]
                m = inrow[uc]
                uc = uc[m]
                w[uc] = w[uc] - mult * lu[u0:u1][m]
        lu[a:b] = w[cols]
        piv = lu[diag[i]]
        if piv == 0.0:
            raise RuntimeError(f"ILU: zero pivot in row {i}")
        dinv[i] = 1.0 / piv
        inrow[cols] = False
    return lu, diag, dinv


def solve(rp, ci, lu, diag, dinv, b):
    """x = (LU)^-1 b, the sums in CSR order (subtract.reduce runs left to right)."""
    n = rp.size - 1
    x = np.empty(n, dtype=np.float64)
    for i in range(n):
        a, d = rp[i], diag[i]
        x[i] = np.subtract.reduce(np.concatenate(([b[i]], lu[a:d] * x[ci[a:d]])))
    for i in range(n - 1, -1, -1):
        d, e = diag[i] + 1, rp[i + 1]
        x[i] = np.subtract.reduce(np.concatenate(([x[i]], lu[d:e] * x[ci[d:e]]))) * dinv[i]
    return x


class PCILUk:
    type = "ilu"

    def __init__(self, M, k, fast=False):
        self.k, self.fast = int(k), fast
        self.rp, self.ci, self.lev = (symbolic_products if fast else symbolic_rowmerge)(M, self.k)
        self.nnz = int(self.ci.size)
        self.max_row = int(np.diff(self.rp).max())
        self._M, self._f, self._native = M, None, None

    def factors(self):
        """(lu, diag, dinv), factored on first use: the pattern alone is cheap."""
        if self._f is None:
            v = filled_values(self._M, self.rp, self.ci)
            if self.fast:
                from oracle import native
                n = self.rp.size - 1
                self._native = f = native.ILU0(sp.csr_matrix((v, self.ci, self.rp), shape=(n, n)))
                assert np.array_equal(f.rp, self.rp) and np.array_equal(f.ci, self.ci)  # zeros kept
                self._f = (f.lu, f.diag, f.dinv)
            else:
                self._f = numeric_ikj(self.rp, self.ci, v)
        return self._f

    lu = property(lambda self: self.factors()[0])
    diag = property(lambda self: self.factors()[1])
    dinv = property(lambda self: self.factors()[2])

    def apply(self, x):
        if self.fast:
            self.factors()
            return self._native.solve(np.asarray(x, dtype=np.float64))
        return solve(self.rp, self.ci, self.lu, self.diag, self.dinv, np.asarray(x, dtype=np.float64))


class PCBJacobi:
    """PCBJACOBI with ILU(k) blocks: PETSc's block sizes, each block's own truncated matrix."""
    type = "bjacobi"

    def __init__(self, M, nblocks, k, fast=False):
        M = sp.csr_matrix(M)
        n = M.shape[0]
        nblocks = max(1, min(int(nblocks), n))
        self.bounds = np.concatenate([[0], np.cumsum(bjacobi_block_sizes(n, nblocks))]).astype(np.int64)
        self.subs = [PCILUk(M[lo:hi, lo:hi].tocsr(), k, fast) for lo, hi in zip(self.bounds[:-1], self.bounds[1:])]
        self.nnz = sum(s.nnz for s in self.subs)
        self.max_row = max(s.max_row for s in self.subs)

    def apply(self, x):
        y = np.empty(x.size, dtype=np.float64)
        for s, lo, hi in zip(self.subs, self.bounds[:-1], self.bounds[1:]):
            y[lo:hi] = s.apply(x[lo:hi])
        return y
