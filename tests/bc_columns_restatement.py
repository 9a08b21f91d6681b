"""<prefix>pls_bc_columns restated in numpy: detection of the rows
dolfin's bc.apply replaced, the split K = K' + C and the lift b' = b - C b.  Works on the stored
arrays of a CSR block (explicit zeros count as stored), so that the device's lists, C and K' can
be compared entry for entry.  tests/test_bc_columns_restatement.py pins it on the CPU,
tests/test_gpu_bc_columns.py holds the device against it."""
import numpy as np
import scipy.sparse as sp


def _csr(K):
    K = sp.csr_matrix(K)
    if not K.has_sorted_indices:
        K = K.copy()
        K.sort_indices()
    return K


def block_of(P, rows):
    """P[rows][:, rows] with its stored zeros, columns ascending."""
    rows = np.asarray(rows)
    return _csr(sp.csr_matrix(P)[rows][:, rows])


def identity_rows(K):
    """Constrained rows, ascending: the diagonal is stored and equals 1.0 exactly, every other
    stored value of the row is 0.0 (tools/s_cg_attribution.py: identity_rows)."""
    K = _csr(K)
    n = K.shape[0]
    r = np.repeat(np.arange(n), np.diff(K.indptr))
    diag = r == K.indices
    bad = np.where(diag, K.data != 1.0, K.data != 0.0)
    nbad = np.bincount(r, weights=bad, minlength=n)
    ndiag = np.bincount(r, weights=diag, minlength=n)
    return np.flatnonzero((nbad == 0) & (ndiag > 0)).astype(np.int32)


def split(K):
    """(bc_rows, K', c_rp, c_ci, c_val).  K' has K's pattern, every stored value in a constrained
    column outside that column's own row set to 0.0.  C, CSR over all rows of K, holds the moved
    values that were nonzero, in stored (ascending column) order."""
    K = _csr(K)
    n = K.shape[0]
    bc = identity_rows(K)
    is_bc = np.zeros(n, dtype=bool)
    is_bc[bc] = True
    r = np.repeat(np.arange(n), np.diff(K.indptr))
    cons = is_bc[K.indices] & (r != K.indices)
    moved = cons & (K.data != 0.0)
    Kp = sp.csr_matrix((np.where(cons, 0.0, K.data), K.indices.copy(), K.indptr.copy()), shape=K.shape)
    c_rp = np.concatenate([[0], np.cumsum(np.bincount(r[moved], minlength=n))]).astype(np.int64)
    return bc, Kp, c_rp, K.indices[moved].astype(np.int32), K.data[moved].astype(np.float64)


def c_matrix(n, c_rp, c_ci, c_val):
    return sp.csr_matrix((c_val, c_ci, c_rp), shape=(n, n))


def lift(b, c_rp, c_ci, c_val):
    """b' = b - C b, each row's sum taken in stored order."""
    out = np.array(b, dtype=np.float64, copy=True)
    for i in np.flatnonzero(np.diff(c_rp)):
        s = 0.0
        for e in range(c_rp[i], c_rp[i + 1]):
            s += c_val[e] * b[c_ci[e]]
        out[i] = b[i] - s
    return out


def zero_bc_columns(P, index_sets):
    """P with the constrained columns zeroed inside each of the given diagonal blocks (index sets
    in P's numbering): what a CPU oracle is handed to express `drop`."""
    P = _csr(P).copy()
    n = P.shape[0]
    r = np.repeat(np.arange(n), np.diff(P.indptr))
    for rows in index_sets:
        rows = np.asarray(rows)
        bc = rows[identity_rows(block_of(P, rows))]
        in_block = np.zeros(n, dtype=bool)
        in_block[rows] = True
        is_bc = np.zeros(n, dtype=bool)
        is_bc[bc] = True
        hit = in_block[r] & is_bc[P.indices] & (r != P.indices)
        P.data[hit] = 0.0
    return P
