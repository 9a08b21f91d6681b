"""y = A x over shared delta streams (option pls.d16_share 1; DESIGN.md "Shared delta streams").

For every case of tests/d16_share_restatement.py (pinned on the CPU by
tests/test_d16_share_restatement.py, which asserts the classes each case reaches):

* ``spmv_layout()`` equals the restated bytes of the shared layout to the byte, and
  ``d16_share()`` reports the restated numbers of shared slices and stored deltas -- the class
  kernels found the classes the restatement finds, and the product ran over the shared stream;
* ``matmult`` on integer data (values in [-8, 8], x in [-16, 16]: every partial sum an integer far
  below 2^53) equals the int64 product bit for bit;
* on standard-normal data, pls.d16_share 1 equals pls.d16_share 0 bit for bit: the columns, the
  values and the order of the sums are the same.

pls.d16_share is passed explicitly: auto leaves matrices of this size as they are.
"""
import numpy as np
import pytest

import d16_share_restatement as D
import spmv_layout_cases as LC

pytestmark = pytest.mark.gpu


def _product(case, kind, share, extra=None, single=False):
    """(y, spmv_layout(), spmv_layout_single() or None, d16_share()) of one handle."""
    import scipy.sparse as sp
    from lib.handle import Handle
    A, x, is_s, is_f, is_p, opts = D.system(case, kind)
    opts = dict(opts, **{"pls.d16_share": str(share)}, **(extra or {}))
    h = Handle.from_csr(A, sp.identity(A.shape[0], format="csr"), None, is_s, is_f, is_p, [], opts)
    try:
        y = h.matmult_single(x) if single else h.matmult(x)
        out = y, h.spmv_layout(), (h.spmv_layout_single() if single else None), h.d16_share()
    finally:
        h.destroy()
    return (A, x) + out


def _check(case, extra=None, single=False):
    """The three checks of one case; returns the shared products (int, normal)."""
    L, _, Sh = D.restated(case)
    A, x, y, lay, low, st = _product(case, "int", 1, extra, single)
    print(f"{case.id} {extra or ''} single={single}: layout {lay} {low}, restated {Sh.bytes} "
          f"(plain {L.bytes()}), d16_share {st}, restated slices {L.nslices} shared {Sh.shared_slices} "
          f"deltas {Sh.dstored}")
    assert lay == (True, Sh.bytes)
    if single:
        assert low == (True, Sh.bytes - 4 * L.stored)
    assert st[:4] == (1, L.nslices, Sh.shared_slices, Sh.dstored) and st[4] >= 1
    assert np.array_equal(y, LC.exact_product(A, x).astype(np.float64))
    _, _, y1, lay1, _, _ = _product(case, "normal", 1, extra, single)
    _, _, y0, lay0, low0, st0 = _product(case, "normal", 0, extra, single)
    assert lay1 == (True, Sh.bytes) and lay0 == (True, L.bytes())
    assert st0 == (0, L.nslices, 0, L.stored, 0)
    assert np.any(y1 != 0.0) and np.array_equal(y1, y0)
    return y, y1


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.id)
def test_layout_and_product(gpu, case):
    _check(case)


@pytest.mark.parametrize("case", [c for c in D.CASES if c.single], ids=lambda c: c.id)
def test_fp32_values_over_shared_deltas(gpu, case):
    """matmult_single: the fp32 value stream over the shared deltas; its layout streams 4 B less
    per stored entry."""
    _check(case, single=True)


def test_unroll_does_not_change_the_sums(gpu):
    """pls.d16_unroll 1, 2 and 4 on the ramp's slices of 1..5 groups of 8 entries (C = 3): a step
    that ends in a partial group clamps its group number, so no pack beyond the slice's C * L
    deltas is read."""
    ys = [_check(D.BY_ID["ramp"], {"pls.d16_unroll": u}) for u in ("1", "2", "4")]
    for yi, yn in ys[1:]:
        assert np.array_equal(yi, ys[0][0]) and np.array_equal(yn, ys[0][1])


def test_xcd_block_map_gives_the_same_bits(gpu):
    """pls.d16_xcd 1 against 0 on the sorted plan (a row map, 1 and 2 lanes per row)."""
    a = _check(D.BY_ID["sorted"], {"pls.d16_xcd": "0"})
    b = _check(D.BY_ID["sorted"], {"pls.d16_xcd": "1"})
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_auto_rule(gpu):
    """pls.d16_share -1: off below pls.d16_share_min_bytes (the default, 256 MiB, leaves every
    matrix here alone); with the threshold at 1 byte it engages where the shared layout is smaller
    (classes-320) and declines where it is not (64 different streams: nothing saved, 80 B more)."""
    import scipy.sparse as sp
    from lib.handle import Handle
    import spmv_layout_restatement as R

    def run(A, opts):
        n = A.shape[0]
        is_s, is_f, is_p, _ = LC.index_sets(LC.Case("auto", ()), n)
        h = Handle.from_csr(A, sp.identity(n, format="csr"), None, is_s, is_f, is_p, [], opts)
        try:
            return h.matmult(np.ones(n)), h.spmv_layout(), h.d16_share()
        finally:
            h.destroy()

    case = D.BY_ID["classes-320"]
    L, _, Sh = D.restated(case)
    A = D.system(case)[0]
    assert Sh.bytes < L.bytes()
    y0, lay, st = run(A, {})
    assert lay == (True, L.bytes()) and st[0] == 0 and st[4] == 0
    y1, lay, st = run(A, {"pls.d16_share": "-1", "pls.d16_share_min_bytes": "1"})
    assert lay == (True, Sh.bytes) and st[:4] == (1, 5, 4, Sh.dstored)
    assert np.array_equal(y0, y1)
    B = D.distinct_64()
    Lb = R.layout(B, {})
    yb, lay, st = run(B, {"pls.d16_share": "-1", "pls.d16_share_min_bytes": "1"})
    assert lay == (True, Lb.bytes()) and st[:4] == (0, 1, 0, Lb.stored)
    assert np.array_equal(yb, B @ np.ones(64))
