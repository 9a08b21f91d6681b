"""tests/asm_restatement.py pinned on the CPU: the subdomain growth against a hand-worked
nonsymmetric pattern and against a plain set-based loop, the two identities (overlap 0 is
bjacobi, one block is ilu), and what the four types do to a row's contributions.
tests/test_gpu_asm.py holds the device against this restatement.

Recorded, not asserted (restated right-preconditioned GMRES, "pc type" diagonal, preonly inner
solves, B = 3 on both blocks, ILU(0); outer iterations to rtol 1e-6 / atol 1e-8):

    system      bjacobi   asm overlap 1   asm overlap 2   (restrict)
    2-D N = 6      17          12              12
    3-D N = 4      15          11              10
"""
import numpy as np
import pytest
import scipy.sparse as sp

from asm_restatement import PCASM, TYPES, subdomains
from iluk_restatement import PCBJacobi, PCILUk
from oracle import synthetic as S
from oracle.blockpc import submatrix

# ----------------------------------------------- the hand-worked pattern ----
# Structurally nonsymmetric 6 x 6, two blocks {0, 1, 2} and {3, 4, 5} (x stored, 0 a stored zero):
#        0  1  2  3  4  5
#   0  [ x  .  .  .  x  . ]      (0, 4) has no (4, 0)
#   1  [ .  x  x  .  .  . ]
#   2  [ .  x  x  .  .  . ]
#   3  [ .  .  0  x  .  . ]      (3, 2) is a stored zero, and has no (2, 3)
#   4  [ .  .  .  .  x  x ]
#   5  [ x  .  .  .  .  x ]      (5, 0) has no (0, 5)
# Block 0: round 1 reads rows 0, 1, 2 -> columns {0, 4, 1, 2}: adds 4.  Round 2 reads row 4 -> adds 5.
#          Round 3 reads row 5 -> {0, 5}: nothing new.
#          A transposed search would add 3 and 5 in round 1 (columns 2 and 0 of rows 3 and 5), a
#          symmetrised one 3, 4 and 5.
# Block 1: round 1 reads rows 3, 4, 5 -> {2, 3, 4, 5, 0}: adds 0 and 2 (the stored zero counts).
#          Round 2 reads rows 0 and 2 -> {0, 4, 1, 2}: adds 1.
HAND_ROWS = [[0, 4], [1, 2], [1, 2], [2, 3], [4, 5], [0, 5]]
HAND_SETS = {0: ([0, 1, 2], [3, 4, 5]),
             1: ([0, 1, 2, 4], [0, 2, 3, 4, 5]),
             2: ([0, 1, 2, 4, 5], [0, 1, 2, 3, 4, 5]),
             3: ([0, 1, 2, 4, 5], [0, 1, 2, 3, 4, 5])}


def _hand_matrix():
    ci = np.concatenate(HAND_ROWS).astype(np.int32)
    rp = np.concatenate([[0], np.cumsum([len(r) for r in HAND_ROWS])]).astype(np.int32)
    v = np.where((np.repeat(np.arange(6), 2) == 3) & (ci == 2), 0.0, 1.0)  # (3, 2): the stored zero
    M = sp.csr_matrix((v, ci, rp), shape=(6, 6))
    assert M.nnz == 12 and M[3, 2] == 0.0
    return M


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_growth_on_the_hand_worked_pattern(k):
    bounds, sets = subdomains(_hand_matrix(), 2, k)
    assert bounds.tolist() == [0, 3, 6]
    assert [s.tolist() for s in sets] == [list(s) for s in HAND_SETS[k]]
    assert all(s.dtype == np.int32 for s in sets)


def _set_loop(rows_of, n, nblocks, k):
    """MatIncreaseOverlap_SeqAIJ with Python sets, one row at a time."""
    sizes = [n // nblocks + (b < n % nblocks) for b in range(nblocks)]
    out, lo = [], 0
    for sz in sizes:
        have = set(range(lo, lo + sz))
        added = set(have)
        for _ in range(k):
            new = set()
            for r in added:
                for j in rows_of[r]:
                    if j not in have:
                        new.add(j)
            have |= new
            added = new
        out.append(sorted(have))
        lo += sz
    return out


@pytest.mark.parametrize("nblocks", [1, 4, 7, 60])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_growth_on_a_random_nonsymmetric_pattern(k, nblocks):
    rng = np.random.default_rng(60)
    n = 60
    D = (rng.random((n, n)) < 0.04) | np.eye(n, dtype=bool)
    assert (D != D.T).sum() > 50  # one-sided entries
    M = sp.csr_matrix(D.astype(np.float64))
    rows_of = [M.indices[M.indptr[i]:M.indptr[i + 1]].tolist() for i in range(n)]
    _, sets = subdomains(M, nblocks, k)
    assert [s.tolist() for s in sets] == _set_loop(rows_of, n, nblocks, k)
    # and the transposed pattern grows differently
    if k == 1 and nblocks == 4:
        assert [s.tolist() for s in subdomains(M.T.tocsr(), nblocks, k)[1]] != [s.tolist() for s in sets]


# ------------------------------------------------------------ identities ----
@pytest.fixture(scope="module")
def block_s():
    spec = S.SynthSpec(2, 6)
    is_s = S.field_major_index_sets(spec)[0]
    M = submatrix(S.matrix(spec, 1), is_s, is_s)
    assert M.shape[0] == 338
    return M, np.random.default_rng(11).standard_normal(M.shape[0])


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("nblocks", [3, 7])
def test_overlap_0_is_bjacobi_bitwise(block_s, nblocks, k):
    M, x = block_s
    for t in TYPES:  # no overlap: nothing to mask
        assert np.array_equal(PCASM(M, nblocks, 0, t, k).apply(x), PCBJacobi(M, nblocks, k).apply(x))


@pytest.mark.parametrize("k", [0, 1])
def test_one_block_is_ilu_bitwise(block_s, k):
    M, x = block_s
    pc = PCASM(M, 1, 1, "restrict", k)
    assert pc.rows[0].tolist() == list(range(M.shape[0])) and pc.nnz == PCILUk(M, k).nnz
    assert np.array_equal(pc.apply(x), PCILUk(M, k).apply(x))


# ------------------------------------------------------------- the types ----
def test_the_four_types_differ_at_overlap_1(block_s):
    M, x = block_s
    ys = [PCASM(M, 3, 1, t).apply(x) for t in TYPES]
    for i in range(4):
        for j in range(i):
            assert np.max(np.abs(ys[i] - ys[j])) > 1e-6 * np.max(np.abs(ys[i])), (TYPES[i], TYPES[j])
    assert np.max(np.abs(ys[0] - PCBJacobi(M, 3, 0).apply(x))) > 1e-6 * np.max(np.abs(ys[0]))


@pytest.mark.parametrize("overlap", [1, 2])
def test_restrict_writes_every_row_exactly_once(block_s, overlap):
    M, x = block_s
    for t, once in (("restrict", True), ("none", True), ("basic", False), ("interpolate", False)):
        pc = PCASM(M, 3, overlap, t)
        pc.apply(x)
        assert (pc.writes >= 1).all()
        assert (pc.writes.max() == 1) == once, t
        assert pc.stats(False)[3] == sum(r.size for r in pc.rows) > M.shape[0]


def test_basic_sums_in_block_order(block_s):
    M, x = block_s
    pc = PCASM(M, 7, 2, "basic")
    y = pc.apply(x)
    assert pc.writes.max() >= 2
    want = np.zeros(M.shape[0])
    for b in range(7):  # 0.0 + block 0's + block 1's + ...: one row at a time
        yb = pc.subs[b].apply(x[pc.rows[b]])
        for r, v in zip(pc.rows[b], yb):
            want[r] = want[r] + v
    assert np.array_equal(y, want)
    # the reverse order gives other bits somewhere (the order is part of the definition)
    rev = np.zeros(M.shape[0])
    for b in reversed(range(7)):
        rev[pc.rows[b]] += pc.subs[b].apply(x[pc.rows[b]])
    assert np.allclose(rev, y, rtol=1e-12, atol=0)
