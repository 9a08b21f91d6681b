"""y = A^ x -- the outer operator with its stored values rounded to fp32 once, x and every sum in
fp64 (``Handle.matmult_single``, the product of ``-<prefix>pls_gmres_operator single``) -- on the
adversarial CSR patterns of tests/spmv_layout_cases.py, every SELL-64/D16 layout the fp32 value
stream rides on.

Wherever ``spmv_layout()`` reports D16 and the layout has no B3 part:

* bytes: ``spmv_layout_single()`` equals (True, the restated layout's bytes - 4 per stored entry).
* integer data: the values +-1..8 are exact in fp32, so the product equals the int64 product bit for
  bit in every layout and summation order.
* normal data (rows of at most 512 entries): every row within (m + 2) * 2^-53 * (|A^| |x|)_row of
  the np.longdouble product of ``A.data.astype(float32)`` -- the bound of the fp64 test, since the
  values are exact once rounded -- and different from ``matmult(x)`` somewhere, so the fp32 stream
  was read.

The other layouts (int32 SELL-64, a B3 part) are refused with a message that names the layout.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import spmv_layout_cases as C
import spmv_layout_restatement as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_restated = {}


def _expected(case):
    """(d16, bytes, stored, has a B3 part) of the restated layout, computed once per case."""
    if case.id not in _restated:
        A = C.pattern(*case.pattern)
        perm = C.index_sets(case, A.shape[0])[3]
        L = R.layout(C.internal(A, perm), case.options)
        _restated[case.id] = (L.d16, L.bytes(), L.stored, bool(L.b3))
    return _restated[case.id]


def _supported(case):
    d16, _, _, b3 = _expected(case)
    return d16 and not b3


def _handle(case, A, extra=None):
    from lib.handle import Handle
    n = A.shape[0]
    is_s, is_f, is_p, _ = C.index_sets(case, n)
    opts = dict(case.options, **(extra or {}))
    return Handle.from_csr(A, sp.identity(n, format="csr"), None, is_s, is_f, is_p, [], opts)


def _products(case, kind, extra=None):
    """(A, x, A^ x, A x) of one handle, the layouts checked."""
    A, x = C.matrix(case, kind)
    h = _handle(case, A, extra)
    try:
        y = h.matmult_single(x)
        yd = h.matmult(x)
        lay, low = h.spmv_layout(), h.spmv_layout_single()
    finally:
        h.destroy()
    d16, nbytes, stored, _ = _expected(case)
    print(f"{case.id} {extra or ''} {kind}: layout {lay}, single {low}, restated {(d16, nbytes)} stored {stored}")
    assert lay == (d16, nbytes)
    assert low == (True, nbytes - 4 * stored)
    return A, x, y, yd


def _check_exact(case, extra=None):
    A, x, y, yd = _products(case, "int", extra)
    exact = C.exact_product(A, x).astype(np.float64)
    assert np.array_equal(y, exact)
    assert np.array_equal(yd, exact)
    return y


def _check_rounded(case, extra=None):
    A, x, y, yd = _products(case, "normal", extra)
    a32 = A.data.astype(np.float32)
    Al = sp.csr_matrix((a32.astype(np.longdouble), A.indices, A.indptr), shape=A.shape)
    ref = Al @ x.astype(np.longdouble)
    m = np.diff(A.indptr)
    assert m.max() <= 512
    Aabs = sp.csr_matrix((np.abs(a32).astype(np.float64), A.indices, A.indptr), shape=A.shape)
    bound = (m + 2) * U * (Aabs @ np.abs(x))
    err = np.abs(y.astype(np.longdouble) - ref).astype(np.float64)
    worst = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    differ = int((y != yd).sum())
    print(f"{case.id} normal: worst error / bound {worst:.3f}; rows that differ from the fp64 product {differ}")
    assert np.all(err <= bound)
    assert differ > 0
    return y


SUPPORTED = [c for c in C.CASES if c.id not in ("b3-all", "b3-mixed", "b3-nine", "segments-9")
             and not c.id.endswith("-sell")]
REFUSED = [c for c in C.CASES if c not in SUPPORTED]


@pytest.mark.parametrize("case", SUPPORTED, ids=lambda c: c.id)
def test_layout_and_low_product(gpu, case):
    assert _supported(case)
    _check_exact(case)
    if case.rounded:
        _check_rounded(case)


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: c.id)
def test_other_layouts_are_refused(gpu, case):
    """int32 SELL-64 (pls.sell_d16 0, or a lane that needs 9 bases) and layouts that keep a B3 part:
    no fp32 stream; the message names the layout, and spmv_layout_single() reports (False, 0)."""
    assert not _supported(case)
    A, x = C.matrix(case, "int")
    h = _handle(case, A)
    try:
        assert h.spmv_layout_single() == (False, 0)
        name = "SELL/B3" if _expected(case)[3] else "int32 SELL-64"
        with pytest.raises(RuntimeError, match=f"pls_matmult_single.*{name}"):
            h.matmult_single(x)
        assert np.array_equal(h.matmult(x), C.exact_product(A, x).astype(np.float64))
    finally:
        h.destroy()


@pytest.mark.parametrize("name", C.UNROLL_CASES)
def test_unroll_does_not_change_the_sums(gpu, name):
    """pls.d16_unroll_single 1, 2, 4 and 8 (8-entry groups per lane in flight in the fp32-value
    kernel; the ramp's slices hold 1..5 groups, the sigma pattern's 1 and 8, so every depth above 1
    meets a slice that ends in a partial step): the same bits on both data sets."""
    case = C.BY_ID[name]
    ys = [(_check_exact(case, {"pls.d16_unroll_single": u}), _check_rounded(case, {"pls.d16_unroll_single": u}))
          for u in ("1", "2", "4", "8")]
    for yi, yr in ys[1:]:
        assert np.array_equal(yi, ys[0][0])
        assert np.array_equal(yr, ys[0][1])


def _diagonal_handle(vals):
    from lib.handle import Handle
    n = vals.size
    A = sp.csr_matrix((vals, np.arange(n), np.arange(n + 1)), shape=(n, n))
    sets = [np.arange(0, 22, dtype=np.int32), np.arange(22, 43, dtype=np.int32), np.arange(43, n, dtype=np.int32)]
    return Handle.from_csr(A, sp.identity(n, format="csr"), None, *sets, [], {})


ROUNDING_VALUES = [1.0 + 2.0 ** -24,              # a tie: to even, 1.0
                   1.0 + 2.0 ** -24 + 2.0 ** -40,  # just above the tie: 1 + 2^-23
                   1e-40,                          # an fp32 subnormal
                   2.0 ** -150,                    # a tie between 0 and the smallest subnormal: 0
                   -1e-50,                         # below every subnormal: -0.0
                   3.4e38]                         # just under FLT_MAX


def test_values_round_to_nearest_even_once(gpu):
    """64 rows of one entry each and x = ones: y is vals.astype(float32), subnormals kept, ties to
    even -- bit for bit where it is not zero; a row sum starts from +0.0 as in the fp64 kernel, so
    the -0.0 that -1e-50 rounds to comes out as 0.0, which compares equal."""
    vals = np.resize(np.array(ROUNDING_VALUES), 64)
    h = _diagonal_handle(vals)
    try:
        y = h.matmult_single(np.ones(64))
        yd = h.matmult(np.ones(64))
    finally:
        h.destroy()
    want = vals.astype(np.float32).astype(np.float64)
    print("y[:6]", y[:6], "want", want[:6])
    assert np.array_equal(y, want)
    nz = want != 0.0
    assert nz.sum() == 43  # two of the six values round to zero: the 11 rows 3 mod 6 and the 10 rows 4 mod 6
    assert np.array_equal(y[nz].view(np.int64), want[nz].view(np.int64))
    assert np.array_equal(yd, vals)


def test_a_value_that_overflows_fp32_is_refused(gpu):
    vals = np.resize(np.array(ROUNDING_VALUES), 64)
    vals[37] = 1e39
    h = _diagonal_handle(vals)
    try:
        with pytest.raises(RuntimeError, match="pls_matmult_single.*infinite once rounded to fp32"):
            h.matmult_single(np.ones(64))
        assert np.array_equal(h.matmult(np.ones(64)), vals)
    finally:
        h.destroy()


def test_update_matrices_rebuilds_the_fp32_stream(gpu):
    case = C.BY_ID["sigma-lpr2"]
    A, x = C.matrix(case, "normal")
    h = _handle(case, A)
    try:
        y1 = h.matmult_single(x)
        A2 = A.copy()
        A2.data[:] = np.random.default_rng(7).standard_normal(A.nnz)
        h.update_matrices(A=A2)
        y2 = h.matmult_single(x)
        y2d = h.matmult(x)
    finally:
        h.destroy()
    h2 = _handle(case, A2)
    try:
        fresh = h2.matmult_single(x)
    finally:
        h2.destroy()
    assert np.array_equal(y2, fresh)
    assert not np.array_equal(y2, y1) and not np.array_equal(y2, y2d)
