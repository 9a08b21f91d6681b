"""y = A x of the outer operator on adversarial CSR patterns, every storage layout pinned.

Each case of tests/spmv_layout_cases.py builds a handle from the assembled matrix (P a diagonal
matrix, no setup), multiplies once and destroys the handle.  Two things are required:

* ``spmv_layout()`` equals the numpy restatement's (d16, bytes) to the byte
  (tests/spmv_layout_restatement.py, pinned on the CPU by tests/test_spmv_layout_restatement.py,
  which also asserts the branch every case reaches).  Every term of the bytes -- stored entries,
  slices, bases per lane, mapped rows, the B3 part, the RCM gather -- follows from the plan, so a
  device plan that leaves the named branch changes them.
* the product.  Exact: integer values in [-8, 8] and x in [-16, 16] make every partial sum an
  integer far below 2^53, so ``y`` must equal the int64 product bit for bit in every layout and
  summation order.  Rounded (rows of at most 512 entries): standard-normal data against the
  product in np.longdouble, row by row within (m + 2) * 2^-53 * (|A| |x|)_row for a row of m
  entries -- m roundings of the products and sums in any order plus the alpha multiply, and the
  first-order form is safe because (m + 2)^2 * 2^-106 is far below 2^-53 for m <= 512.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import spmv_layout_cases as C
import spmv_layout_restatement as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_restated = {}


def _expected_layout(case):
    """(d16, bytes) of the restated layout, computed once per case (values do not enter it)."""
    if case.id not in _restated:
        A = C.pattern(*case.pattern)
        perm = C.index_sets(case, A.shape[0])[3]
        L = R.layout(C.internal(A, perm), case.options)
        _restated[case.id] = (L.d16, L.bytes())
    return _restated[case.id]


def _device_product(case, A, x, extra=None):
    """(y, spmv_layout()) of one handle: from_csr, matmult, destroy."""
    from lib.handle import Handle
    n = A.shape[0]
    is_s, is_f, is_p, _ = C.index_sets(case, n)
    opts = dict(case.options, **(extra or {}))
    h = Handle.from_csr(A, sp.identity(n, format="csr"), None, is_s, is_f, is_p, [], opts)
    try:
        y = h.matmult(x)
        lay = h.spmv_layout()
    finally:
        h.destroy()
    return y, lay


def _check_exact(case, extra=None):
    A, x = C.matrix(case, "int")
    y, lay = _device_product(case, A, x, extra)
    exact = C.exact_product(A, x)
    wrong = np.nonzero(y != exact)[0]
    print(f"{case.id} {extra or ''} int: layout {lay} restated {_expected_layout(case)}, rows wrong {len(wrong)}"
          + (f" (first {wrong[:5]}: {y[wrong[:5]]} for {exact[wrong[:5]]})" if len(wrong) else ""))
    assert lay == _expected_layout(case)
    assert np.array_equal(y, exact.astype(np.float64))
    return y


def _check_rounded(case, extra=None):
    A, x = C.matrix(case, "normal")
    y, lay = _device_product(case, A, x, extra)
    Al = sp.csr_matrix((A.data.astype(np.longdouble), A.indices, A.indptr), shape=A.shape)
    ref = Al @ x.astype(np.longdouble)
    m = np.diff(A.indptr)
    assert m.max() <= 512
    bound = (m + 2) * U * (abs(A) @ np.abs(x))
    err = np.abs(y.astype(np.longdouble) - ref).astype(np.float64)
    worst = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    print(f"{case.id} {extra or ''} normal: layout {lay}, worst error / bound {worst:.3f}, "
          f"rows with no entry off zero {int((err[bound == 0] != 0).sum())}")
    assert lay == _expected_layout(case)
    assert np.all(err <= bound)
    return y


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_layout_and_product(gpu, case):
    _check_exact(case)
    if case.rounded:
        _check_rounded(case)


@pytest.mark.parametrize("name", C.UNROLL_CASES)
def test_unroll_does_not_change_the_sums(gpu, name):
    """pls.d16_unroll 1, 2 and 4 (8-entry groups per lane in flight; the ramp's slices hold 1..5
    groups, the sigma pattern's 1 and 8, so 2 and 4 both meet slices that end in a partial step):
    the summation order does not depend on it, so the products are bitwise equal on the rounded
    data too."""
    case = C.BY_ID[name]
    ys = [(_check_exact(case, {"pls.d16_unroll": u}), _check_rounded(case, {"pls.d16_unroll": u}))
          for u in ("1", "2", "4")]
    for yi, yr in ys[1:]:
        assert np.array_equal(yi, ys[0][0])
        assert np.array_equal(yr, ys[0][1])


@pytest.mark.parametrize("name", C.XCD_CASES)
def test_xcd_block_map_gives_the_same_bits(gpu, name):
    """pls.d16_xcd 1 hands every XCD a contiguous range of slices; the grid is rounded up to a
    multiple of 8 blocks and the surplus blocks exit.  Same bits as pls.d16_xcd 0 before and after
    in this process: the flag is an option of the handle, one handle at a time here."""
    case = C.BY_ID[name]
    runs = [(_check_exact(case, {"pls.d16_xcd": v}), _check_rounded(case, {"pls.d16_xcd": v}))
            for v in ("0", "1", "0")]
    for yi, yr in runs[1:]:
        assert np.array_equal(yi, runs[0][0])
        assert np.array_equal(yr, runs[0][1])


@pytest.mark.parametrize("name", C.XCD_CASES)
def test_xcd_flag_belongs_to_the_handle(gpu, name):
    """Two handles on one matrix, pls.d16_xcd 1 and 0, both alive, multiplied in the order 1, 0, 1,
    0: every product of the "int" data equals the int64 product bit for bit.  One value of the
    handle decides both the grid rounding and the kernel's block map.  These cases' slice counts are
    no multiple of 32 (tests/test_spmv_layout_restatement.py), so the rounded grid has surplus
    blocks, and a map under an unrounded grid -- one handle's flag reaching another's launch --
    would skip slices.  The mapped and the plain product are bitwise equal by design, so this
    guards only a grid and a map that disagree; it cannot see which map ran."""
    from lib.handle import Handle
    case = C.BY_ID[name]
    A, x = C.matrix(case, "int")
    n = A.shape[0]
    is_s, is_f, is_p, _ = C.index_sets(case, n)
    exact = C.exact_product(A, x).astype(np.float64)
    handles = []
    try:
        for v in ("1", "0"):
            handles.append(Handle.from_csr(A, sp.identity(n, format="csr"), None, is_s, is_f, is_p, [],
                                           dict(case.options, **{"pls.d16_xcd": v})))
        for turn in range(4):
            y = handles[turn % 2].matmult(x)
            wrong = np.nonzero(y != exact)[0]
            print(f"{case.id} product {turn} (pls.d16_xcd {1 - turn % 2}): rows wrong {len(wrong)}")
            assert np.array_equal(y, exact)
    finally:
        for h in handles:
            h.destroy()
