"""The preconditions of tests/lu_cases.py, on the CPU.

For every case: the numpy restatements of the runtime's geometry (tile rows and tile bandwidths from
the stored pattern, SPIKE partition length and partition sizes per pls.band_spike_plen) give the values
the table names and the branch each case is there for; the "int" and "swap" data are exact -- L^-1, U^-1
and K^-1 are dyadic far below 2^53 and K^-1 x is y* bit for bit; the restated pivot rule exchanges
nothing on "int" data and exactly the tabled rows on "swap" data; on the "normal" data the plain float64
solve is within 1e-13 of the np.longdouble reference, a tenfold margin under the device bar.
"""
import numpy as np
import pytest

import lu_cases as C

BAND = [pytest.param(c, id=c.id) for c in C.BAND_CASES]
ALL = [pytest.param(c, id=c.id) for c in C.CASES]
DENSE = [pytest.param(c, id=c.id) for c in C.DENSE_CASES]


@pytest.mark.parametrize("case", ALL)
def test_bandwidths_are_the_named_ones(case):
    """The stored pattern of every data set has exactly the scalar bandwidths the case names (the swap
    cases move rows, so only their unswapped K is held to it)."""
    kinds = ["int"] if not case.swaps else []
    kinds += ["normal"] if not case.swaps else []
    for kind in kinds:
        K = C.data(case, kind).K
        assert K.has_sorted_indices
        assert C.bandwidths(K) == (case.kl, case.ku), kind
        r, c = C.coords(K)
        assert np.count_nonzero(r == c) == case.n  # the diagonal is stored (K_ii itself may be 0: the pivots are U's)
    if case.swaps:
        _, _, K, _ = C._factors(case.id)
        assert C.bandwidths(K) == (case.kl, case.ku)
        r, c = C.coords(C.data(case, "swap").K)
        assert np.count_nonzero(r == c) == case.n  # K' stores its diagonal, zeros included


@pytest.mark.parametrize("case", BAND)
def test_band_geometry_as_tabled(case):
    nb, bl, bu = C.tile_geometry(case.n, *C.bandwidths(C.data(case, "int").K))
    assert (nb, bl, bu) == case.geometry
    for run, want in case.runs.items():
        plen, parts = C.spike_partitions(nb, bl, bu, C.requested_plen(run))
        assert (plen, parts) == want, run
        assert sum(parts) == nb and (plen == 0 or (plen % 2 == 0 and plen >= max(bl, bu)))


def test_band_cases_reach_their_branches():
    """What each table row is there for, from the restated geometry."""
    g = {c.id: c for c in C.BAND_CASES}
    parts = {(c.id, r): C.spike_partitions(*c.geometry, C.requested_plen(r)) for c in C.BAND_CASES for r in c.runs}
    assert g["one-tile"].geometry[0] == 1 and parts["one-tile", "auto"][0] == 0
    assert g["diagonal"].geometry[1:] == (0, 0) and parts["diagonal", "auto"][0] == 0
    assert g["lower-only"].geometry[2] == 0 and g["upper-only"].geometry[1] == 0
    assert g["lower-only"].n % 64 != 0 and g["upper-only"].n % 64 != 0
    # bandwidth 64 is one tile, 65 two
    assert C.tile_geometry(256, 64, 65) == (4, 1, 2) and g["tile-edges"].n % 64 == 0
    assert g["odd-nb"].geometry[0] % 2 == 1 and g["tile-edges"].geometry[0] % 2 == 0
    assert parts["odd-nb", "3"] == (4, (4, 3)) and len(parts["odd-nb", "auto"][1]) == 2  # odd plen rounded; P == 2
    bw = g["wide"].geometry[1]
    assert bw > C.SPIKE_CG and C.tail_groups(bw) == 2 and C.tail_groups(g["skewed"].geometry[2]) == 1
    assert parts["wide", "auto"][1][-1] < bw and len(parts["wide", "auto"][1]) >= 3  # short last partition; tails run
    assert len(parts["wide", "10"][1]) == 2 and len(parts["wide", "8"][1]) == 3
    nb = g["long-narrow"].geometry[0]
    assert -(-nb // 16) == 3 > g["long-narrow"].geometry[1] and parts["long-narrow", "auto"][0] == 4  # auto plen rounded
    assert len(parts["long-narrow", "auto"][1]) == 9 and parts["long-narrow", "auto"][1][-1] == 1
    assert parts["long-narrow", "2"][1][-1] == 1
    assert parts["lower-only", "2"][0] == 2  # a requested plen of bw stays
    assert C.spike_partitions(20, 5, 5, 2)[0] == 6  # a requested plen below bw is raised to it, then to even
    assert g["skewed"].geometry[1:] == (1, 4) and parts["skewed", "auto"][0] == 4


@pytest.mark.parametrize("case", ALL)
def test_exact_data_is_exact(case):
    d = C.data(case, C.exact_kind(case))
    n = case.n
    L, U = d.L, d.U
    r, c = C.coords(L)
    assert np.all(c <= r) and np.array_equal(L.diagonal(), np.ones(n))
    off = r != c
    assert np.all(c[off] % 4 < r[off] % 4) and np.all(np.abs(L.data[off]) == 1.0)
    assert np.all(r[off] - c[off] <= case.kl) and np.bincount(r[off], minlength=n).max(initial=0) <= C.PER_ROW
    assert not np.any(c[off] % 4 == 3)  # no class-3 column below the diagonal
    ur, uc = C.coords(U)
    uoff = ur != uc
    assert np.all(uc >= ur) and np.all(ur[uoff] % 4 < uc[uoff] % 4) and np.all(uc[uoff] - ur[uoff] <= case.ku)
    assert set(np.unique(U.diagonal())) <= set(C.DIAG_U)
    Li, Ui = C.exact_inverses(L, U)
    Ki = Ui @ Li
    for M in (Li, Ui, Ki):
        assert C.is_dyadic(M)
    print(f"{case.id}: max |L^-1| {np.abs(Li).max():g}, |U^-1| {np.abs(Ui).max():g}, |K^-1| {np.abs(Ki).max():g}")
    Kd = (L @ U).toarray()
    assert np.array_equal(Ki @ Kd, np.eye(n))
    x = d.x[:n]
    perm = C.row_order(case)  # K' = Pi K: K'^-1 x = K^-1 Pi^T x
    assert np.array_equal(d.K.toarray(), Kd[perm])
    unpermuted = np.empty(n)
    unpermuted[perm] = x
    assert np.array_equal(Ki @ unpermuted, d.y)
    # the second right-hand side of the epoch test, -2 x + e: its solution is dyadic and K' maps it back exactly
    x2, y2 = C.second_rhs(case)
    assert np.array_equal(x2[:n], -2.0 * x + d.e) and np.array_equal(x2[n:], -2.0 * d.x[n:])
    assert C.is_dyadic(y2)
    assert np.array_equal(d.K.toarray() @ y2, x2[:n])


@pytest.mark.parametrize("case", DENSE)
def test_pivot_rule_predicts_the_exchanges(case):
    d = C.data(case, C.exact_kind(case))
    exchanged, below, zero, perm = C.pivot_rule(d.K.toarray())
    assert (exchanged, below, zero) == (len(case.swaps), 0, 0)
    want = np.arange(case.n)
    for j, s in case.swaps:
        assert j % 4 == 3 and s > j
        want[[j, s]] = want[[s, j]]
    assert np.array_equal(perm, want)
    if not case.swaps:  # the rounded data is diagonally dominant by rows: |l_ij| can pass 1, 100 it cannot
        assert C.pivot_rule(C.data(case, "normal").K.toarray())[:3] == (0, 0, 0)


def test_pivot_rule_on_hand_examples():
    """The rule's three clauses on columns small enough to read: the diagonal stays at exactly u x the
    largest candidate and goes just below it; a tie takes the smaller row; a zero column is counted."""
    def first(col):
        A = np.eye(len(col))
        A[0, 1:] = 1.0  # (row 0 stays nonzero where its first entry is 0)
        A[:, 0] = col
        return C.pivot_rule(A)
    assert first([0.01, 1.0, 0.5])[0] == 0                       # |a_jj| == u amax: kept
    assert list(first([0.0099, 0.5, 1.0])[3]) == [2, 1, 0]       # below: the largest candidate
    assert list(first([0.0, 1.0, -1.0])[3]) == [1, 0, 2]         # a tie: the smaller row
    assert first([0.0, -1.0, 1.0, 1.0])[3][0] == 1               # (of three)
    assert C.pivot_rule(np.diag([1.0, 0.0, 2.0]))[:3] == (0, 0, 1)  # a zero column: nothing to choose
    assert C.pivot_rule(np.array([[0.0, 1.0], [1.0, 0.0]]), u=0.0)[0] == 0  # u = 0: never (a zero pivot then)


def test_swap_cases_reach_their_tiles():
    t = {c.id: [(j // 64, s // 64) for j, s in c.swaps] for c in C.DENSE_CASES if c.swaps}
    assert t["swap-in-tile"] == [(0, 0)] and t["swap-tile0-tile2"] == [(0, 2)]
    assert t["swap-into-last"] == [(1, 3)] and 200 - 3 * 64 < 64
    assert t["swap-two"] == [(0, 0), (0, 0)]
    assert sorted(c.n for c in C.DENSE_CASES if not c.swaps and c.threshold is None) == [1, 2, 63, 64, 65, 129, 200]


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in C.CASES if not c.swaps])
def test_normal_reference_margin(case):
    d = C.data(case, "normal")
    n = case.n
    y_ref, y0 = C.refined_solve(d.K, d.x[:n])
    assert np.array_equal(y_ref, d.y)
    scale = float(np.abs(y_ref).max())
    ratio = float(np.abs(y0.astype(np.longdouble) - y_ref).max()) / scale
    r, c = C.coords(d.K)
    res = d.x[:n].astype(np.longdouble)
    np.subtract.at(res, r, d.K.data.astype(np.longdouble) * y_ref[c])
    print(f"{case.id}: float64 solve off the reference by {ratio:.2e}, reference residual {float(np.abs(res).max()):.2e}")
    assert ratio <= 1e-13
    # (the refinement ends at the longdouble residual's own rounding: below float64's unit roundoff of x)
    assert float(np.abs(res).max()) <= 1e-16 * float(np.abs(d.x[:n]).max())
