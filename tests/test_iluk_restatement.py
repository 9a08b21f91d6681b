"""tests/iluk_restatement.py pinned on the CPU: level 0 against oracle.native.ILU0 (bitwise), the
row-merge levels against a hand-worked nonsymmetric pattern, the two-search breadth-first
formulation the device kernels use (csrc/iluk.hip) against the row-merge, and ILU(n) = LU.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from iluk_restatement import PCBJacobi, PCILUk, symbolic_products, symbolic_rowmerge
from oracle import native
from oracle import synthetic as S
from oracle.blockpc import submatrix


# ------------------------------------------------------------ level 0 ----
@pytest.fixture(scope="module")
def blocks_2d6():
    spec = S.SynthSpec(2, 6)
    P = S.matrix(spec, 1)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    is_fp = np.concatenate([is_f, is_p])
    return submatrix(P, is_s, is_s), submatrix(P, is_fp, is_fp)


@pytest.mark.parametrize("which", [0, 1], ids=["s", "fp"])
def test_level_0_is_the_native_ilu0_bitwise(blocks_2d6, which):
    M = blocks_2d6[which]
    assert M.shape[0] == (338, 387)[which]
    f, g = native.ILU0(M), PCILUk(M, 0)
    assert np.array_equal(g.rp, f.rp) and np.array_equal(g.ci, f.ci)
    assert np.array_equal(g.lu, f.lu) and np.array_equal(g.dinv, f.dinv)
    x = np.random.default_rng(3).standard_normal(M.shape[0])
    assert np.array_equal(g.apply(x), f.solve(x))


def test_levels_change_the_pattern(blocks_2d6):
    """The issue's table: fill 2.96 / 4.39 on s, 3.48 / 4.57 on fp; longest rows 69 / 103, 176 / 264."""
    for M, fills, rows in zip(blocks_2d6, ((2.96, 4.39), (3.48, 4.57)), ((69, 103), (176, 264))):
        for k, fill, row in zip((1, 2), fills, rows):
            rp, ci, _ = symbolic_rowmerge(M, k)
            assert round(ci.size / M.nnz, 2) == fill and int(np.diff(rp).max()) == row


# ----------------------------------------------- the hand-worked pattern ----
# Structurally nonsymmetric 5 x 5 (x stored, 0 a stored zero):
#        0  1  2  3  4
#   0  [ x  .  .  x  . ]
#   1  [ .  x  .  .  x ]
#   2  [ 0  .  x  .  . ]      (2, 0) is a stored zero
#   3  [ .  x  .  x  . ]
#   4  [ .  .  x  x  x ]
# Level 1: (2, 3) through pivot 0 -- the stored zero (2, 0) counts as structure;
#          (3, 4) through pivot 1; (4, 3) is stored.
#          (4, 0)? the only path 4 -> 2 -> 0 has the intermediate 2 > 0: no fill at any level.
#          (1, 3)? path 1 -> 4 -> 3 runs through 4 > min(1, 3): no fill at any level.
# Level 2: (4, 4) is stored; no entry of level 2 appears: (4, 3) is stored, and (2, 4) would need
#          2 -> 0 -> 3 -> 4 with 3 > 2.
HAND = np.array([[1, 0, 0, 1, 0],
                 [0, 1, 0, 0, 1],
                 [1, 0, 1, 0, 0],
                 [0, 1, 0, 1, 0],
                 [0, 0, 1, 1, 1]])
HAND_VALUES = np.array([[4., 0, 0, 1, 0],
                        [0, 5., 0, 0, 2],
                        [0., 0, 3., 0, 0],   # (2, 0): stored zero
                        [0, 1., 0, 6., 0],
                        [0, 0, 2., 1., 7.]])


def _hand_matrix():
    r, c = np.nonzero(HAND)
    M = sp.csr_matrix((HAND_VALUES[r, c], (r, c)), shape=HAND.shape)
    assert M.nnz == 11  # the stored zero is kept
    return M


def _levels_dense(M, k):
    rp, ci, lev = symbolic_rowmerge(M, k)
    n = rp.size - 1
    D = np.full((n, n), -1)
    for i in range(n):
        D[i, ci[rp[i]:rp[i + 1]]] = lev[rp[i]:rp[i + 1]]
    return D


def test_hand_pattern_levels():
    M = _hand_matrix()
    assert np.array_equal(_levels_dense(M, 0), np.where(HAND, 0, -1))
    want = np.where(HAND, 0, -1)
    want[2, 3] = 1   # through the stored zero (2, 0)
    want[3, 4] = 1
    for k in (1, 2, 5):
        D = _levels_dense(M, k)
        assert np.array_equal(D, want), (k, D)
        assert D[4, 0] == -1 and D[1, 3] == -1  # paths through a vertex larger than the target


def test_missing_diagonal_raises():
    M = sp.csr_matrix(np.array([[1., 1], [1, 0]]))
    with pytest.raises(RuntimeError, match="missing diagonal in row 1"):
        symbolic_rowmerge(M, 1)


# ------------------------------------------- the two-search formulation ----
def _bfs_reach(adj_p, adj_i, i, k):
    """Vertices t > i first reached from i at depth <= k + 1 when only vertices < i are expanded."""
    seen = {i}
    out = {}
    frontier = [i]
    for d in range(k + 1):
        nxt = []
        for v in frontier:
            for t in adj_i[adj_p[v]:adj_p[v + 1]]:
                t = int(t)
                if t in seen:
                    continue
                seen.add(t)
                if t > i:
                    out[t] = d
                else:
                    nxt.append(t)
        frontier = nxt
    return out


def symbolic_two_searches(M, k):
    """U parts by searches on G(A), L parts by searches on G(A^T) transposed back; levels dense, -1 absent."""
    M = sp.csr_matrix(M)
    n = M.shape[0]
    T = sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape).T.tocsr()
    D = np.full((n, n), -1)
    for i in range(n):
        D[i, i] = 0
        for t, lev in _bfs_reach(M.indptr, M.indices, i, k).items():
            D[i, t] = lev
        for t, lev in _bfs_reach(T.indptr, T.indices, i, k).items():
            D[t, i] = lev
    return D


def _random_nonsymmetric(n, seed):
    rng = np.random.default_rng(seed)
    A = (rng.random((n, n)) < 0.06).astype(float)
    np.fill_diagonal(A, 1.0)
    assert np.any((A != 0) != (A.T != 0))
    return sp.csr_matrix(A)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_two_searches_equal_the_row_merge(k):
    for M in (_hand_matrix(), _random_nonsymmetric(60, 11)):
        assert np.array_equal(symbolic_two_searches(M, k), _levels_dense(M, k))


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_recursion_over_levels_equals_the_row_merge(k, blocks_2d6):
    """symbolic_products (fast=True, the 3-D blocks of tests/test_gpu_iluk.py) against the row-merge."""
    for M in (_hand_matrix(), _random_nonsymmetric(60, 11), _random_nonsymmetric(60, 12)) + tuple(blocks_2d6):
        if M.shape[0] > 60 and k == 3:
            continue  # (the 2-D blocks at levels 0, 1, 2: seconds)
        for a, b in zip(symbolic_products(M, k), symbolic_rowmerge(M, k)):
            assert np.array_equal(a, b)


def test_fast_path_is_the_plain_one_bitwise(blocks_2d6):
    """fast=True: oracle.native.ILU0 on the filled matrix is the IKJ factorization on the kept pattern."""
    M = blocks_2d6[0]
    f, g = PCILUk(M, 1, fast=True), PCILUk(M, 1)
    assert np.array_equal(f.ci, g.ci) and np.array_equal(f.lu, g.lu) and np.array_equal(f.dinv, g.dinv)
    x = np.random.default_rng(2).standard_normal(M.shape[0])
    assert np.array_equal(f.apply(x), g.apply(x))
    h = _hand_matrix()
    assert np.array_equal(PCILUk(h, 1, fast=True).apply(np.arange(5.0)), PCILUk(h, 1).apply(np.arange(5.0)))


def test_one_search_is_not_enough():
    """The L part read off the search on G(A) (every t < i it reaches) differs from the row-merge on
    the hand pattern: row 4 reaches 0 through 2, but (4, 0) is no fill entry."""
    M = _hand_matrix()
    seen = set()
    frontier = [4]
    for _ in range(2):
        nxt = []
        for v in frontier:
            for t in M.indices[M.indptr[v]:M.indptr[v + 1]]:
                if t not in seen and t < 4:
                    seen.add(int(t))
                    nxt.append(int(t))
        frontier = nxt
    assert 0 in seen and _levels_dense(M, 1)[4, 0] == -1


# ------------------------------------------------------------- numeric ----
def test_full_levels_are_the_exact_lu():
    rng = np.random.default_rng(5)
    n = 40
    A = (rng.random((n, n)) < 0.12) * rng.standard_normal((n, n))
    A += np.diag(np.abs(A).sum(axis=1) + 1.0)
    M = sp.csr_matrix(A)
    pc = PCILUk(M, n)
    b = rng.standard_normal(n)
    x = pc.apply(b)
    assert np.linalg.norm(A @ x - b) <= 1e-12 * np.linalg.norm(b)
    # and ILU(0) of the same matrix is not
    assert np.linalg.norm(A @ PCILUk(M, 0).apply(b) - b) > 1e-6 * np.linalg.norm(b)


def test_bjacobi_blocks_fill_separately(blocks_2d6):
    M = blocks_2d6[0]
    pc = PCBJacobi(M, 3, 1)
    assert list(np.diff(pc.bounds)) == [113, 113, 112]
    x = np.random.default_rng(1).standard_normal(M.shape[0])
    y = pc.apply(x)
    for s, lo, hi in zip(pc.subs, pc.bounds[:-1], pc.bounds[1:]):
        assert np.array_equal(y[lo:hi], PCILUk(M[lo:hi, lo:hi], 1).apply(x[lo:hi]))
    assert pc.nnz < PCILUk(M, 1).nnz
