"""Adversarial CSR patterns for the outer SpMV layouts, one table for the CPU tests of the
restatement (tests/test_spmv_layout_restatement.py) and the device tests
(tests/test_gpu_spmv_layouts.py).

A case names a pattern, the ``pls.*`` options it runs with and the branch of the planner it is
there for (``expect``, asserted on the restated plan by the CPU test).  Sizes are the smallest that
reach the branch.  Values: "int" -- nonzero integers in [-8, 8] with x in [-16, 16] (every partial
sum is an integer far below 2^53, so every summation order gives the same bits); "normal" --
standard-normal values and x.
"""
import functools
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp


def _pattern(n, rows, cols):
    M = sp.csr_matrix((np.ones(len(rows)), (np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64))),
                      shape=(n, n))
    M.sum_duplicates()
    M.sort_indices()
    M.data[:] = 1.0
    return M


def _runs(n, lens, start, modulus=None, offset=0):
    """Rows of lens[r] consecutive columns offset + (start[r] + j) % modulus."""
    lens = np.asarray(lens, dtype=np.int64)
    rows = np.repeat(np.arange(len(lens)), lens)
    j = np.arange(len(rows)) - np.repeat(np.cumsum(lens) - lens, lens)
    cols = np.asarray(start, dtype=np.int64)[rows] + j
    if modulus is not None:
        cols = cols % modulus
    return rows, cols + offset


def _replace_rows(M, new_rows):
    """M with the rows in new_rows ({row: columns}) replaced."""
    M = M.tolil()
    for r, cols in new_rows.items():
        M.rows[r] = sorted(int(c) for c in cols)
        M.data[r] = [1.0] * len(cols)
    return M.tocsr()


# ------------------------------------------------------------------ patterns --
def edges(n):
    """Tridiagonal; the first, the last and (n > 3) a middle row empty, one row with a single entry."""
    empty = {0, n - 1} | ({n // 2} if n > 3 else set())
    single = 1 if n == 3 else n // 2 + 1
    rows, cols = [], []
    for r in range(n):
        if r in empty:
            continue
        for c in ((r,) if r == single else (r - 1, r, r + 1)):
            if 0 <= c < n:
                rows.append(r)
                cols.append(c)
    return _pattern(n, rows, cols)


WIDE_LEN = 512


def wide(n):
    """Every row 512 consecutive columns from (5 r) % (n - 512): the first columns of rows 63 apart
    differ by 315 except where the start wraps."""
    r = np.arange(n)
    return _pattern(n, *_runs(n, np.full(n, WIDE_LEN), (5 * r) % (n - WIDE_LEN)))


def wide_groups_expected(n):
    """Full 64-row groups of wide(n) whose rows r and r + 63 start more than 4 * 63 columns apart."""
    c0 = (5 * np.arange(n)) % (n - WIDE_LEN)
    return sum(1 for r in range(0, n - 63, 64) if c0[r + 63] - c0[r] > 4 * 63)


def sigma(n):
    """Rows of 128 entries where r % 3 == 0, else 8; columns (r + j) % n."""
    r = np.arange(n)
    return _pattern(n, *_runs(n, np.where(r % 3 == 0, 128, 8), r, modulus=n))


def ramp():
    """Lane-per-row slices of 1, 2, 3, 4 and 5 groups of 8 entries: rows of group g hold
    8 (g + 1) - r % 3 consecutive columns."""
    n = 320
    r = np.arange(n)
    lens = 8 * (r // 64 + 1) - r % 3
    return _pattern(n, *_runs(n, lens, np.minimum(r, n - lens)))


def dense_row():
    """n = 3000, two entries per row; row 1234 holds every column, rows 7 and n - 1 are empty."""
    n = 3000
    r = np.arange(n)
    M = _pattern(n, np.concatenate((r, r)), np.concatenate((r, (r + 7) % n)))
    return _replace_rows(M, {1234: range(n), 7: [], n - 1: []})


def segments(k):
    """Diagonal, every 4099th row replaced by k entries 65600 columns apart: k bases on one lane."""
    n = 9 * 65536 + 300
    r = np.arange(n)
    far = r[r % 4099 == 0]
    keep = r[r % 4099 != 0]
    rows = np.concatenate((keep, np.repeat(far, k)))
    cols = np.concatenate((keep, (np.repeat(far % 100, k) + 65600 * np.tile(np.arange(k), len(far)))))
    return _pattern(n, rows, cols)


def delta_edge():
    """Column gaps of exactly 65535 (one base) and 65536 (two)."""
    n = 2 * 65536 + 200
    r = np.arange(n)
    return _replace_rows(_pattern(n, r, r), {10: [3, 3 + 65535, 3 + 2 * 65535], 20: [3, 3 + 65536],
                                             30: [0, 65535, 131070, n - 1], 40: [0, 65536]})


def _triples(first_row, lens, n):
    """Row triples from first_row on, triple t with lens[t] consecutive columns in all three rows."""
    lens = np.asarray(lens, dtype=np.int64)
    row_lens = np.repeat(lens, 3)
    heads = first_row + 3 * np.arange(len(lens))
    rows, cols = _runs(n, row_lens, np.repeat(np.minimum(heads, n - lens), 3))
    return rows + first_row, cols


def b3_all():
    """n = 192, every row in a triple, lengths 1..30: the D16 part is empty."""
    n = 192
    return _pattern(n, *_triples(0, 1 + (7 * np.arange(64)) % 30, n))


def _b3_with_singles(ntrip, trip_lens, nsingle, single_lens):
    n = 3 * ntrip + nsingle
    tr, tc = _triples(0, trip_lens, n)
    sr, sc = _runs(n, single_lens, np.minimum(3 * ntrip + np.arange(nsingle), n - np.asarray(single_lens)))
    return _pattern(n, np.concatenate((tr, sr + 3 * ntrip)), np.concatenate((tc, sc)))


def b3_mixed():
    """70 triples of 10..40 entries and 90 single rows of 1..80 (neighbours differ in length)."""
    return _b3_with_singles(70, 10 + (11 * np.arange(70)) % 31, 90, 1 + (11 * np.arange(90)) % 80)


def b3_minor():
    """10 triples among 270 single rows: the triples hold less than half the entries."""
    return _b3_with_singles(10, 10 + np.arange(10), 270, 1 + (11 * np.arange(270)) % 40)


def b3_nine():
    """300 triples, a few short single rows and one single row that needs 9 bases; every other row
    is empty."""
    n = 8 * 65600 + 1000
    tr, tc = _triples(0, 20 + (3 * np.arange(300)) % 17, n)
    extra_r = np.array([1000, 1001, 1001, 2000] + [5000] * 9)
    extra_c = np.array([1000, 7, 1001, 2000] + [17 + 65600 * j for j in range(9)])
    return _pattern(n, np.concatenate((tr, extra_r)), np.concatenate((tc, extra_c)))


RCM_N = 16384 + 100


def uniform():
    """8 entries in every row, columns (r + j) % n: nothing to pad."""
    r = np.arange(RCM_N)
    return _pattern(RCM_N, *_runs(RCM_N, np.full(RCM_N, 8), r, modulus=RCM_N))


def two_components():
    """Two blocks of the sigma pattern that share no column, and an empty row."""
    na = 8000
    nb = RCM_N - na
    ra, ca = _runs(na, np.where(np.arange(na) % 3 == 0, 128, 8), np.arange(na), modulus=na)
    rb, cb = _runs(nb, np.where(np.arange(nb) % 3 == 0, 128, 8), np.arange(nb), modulus=nb, offset=na)
    return _replace_rows(_pattern(RCM_N, np.concatenate((ra, rb + na)), np.concatenate((ca, cb))), {12345: []})


def source_row():
    """The uniform pattern on rows and columns 1..n-1; row 0 points into them and no row points back:
    the RCM sweep from row 0 ends in vertices that do not reach it."""
    m = RCM_N - 1
    rows, cols = _runs(m, np.full(m, 8), np.arange(m), modulus=m, offset=1)
    r0 = np.zeros(8, dtype=np.int64)
    c0 = np.concatenate(([0], 5 + 4 * np.arange(7)))
    return _pattern(RCM_N, np.concatenate((r0, rows + 1)), np.concatenate((c0, cols)))


@functools.lru_cache(maxsize=4)
def pattern(name, *args):
    return globals()[name](*args)


# --------------------------------------------------------------------- cases --
@dataclass(frozen=True)
class Case:
    id: str
    pattern: tuple                 # (function name, arguments...)
    opts: tuple = ()               # ((pls.* key, value string), ...)
    expect: tuple = ()             # ((property, value), ...) of the restated layout
    rounded: bool = True           # rows of at most 512 entries: the rounded-data check applies
    interleaved: bool = False      # index sets r % 3 instead of three contiguous ranges
    seed: int = 0

    @property
    def options(self):
        return dict(self.opts)


def _case(id, pattern, opts=None, rounded=True, interleaved=False, **expect):
    return Case(id, pattern, tuple(sorted((opts or {}).items())), tuple(sorted(expect.items())), rounded, interleaved,
                seed=len(id) + sum(map(ord, id)))


PLAIN = dict(d16=True, fallback=False, sorted=False, multi=0, b3=False, rcm=False)
SELL = dict(d16=False, fallback=False, b3=False, rcm=False)


def _cases():
    out = []
    for n in (3, 63, 64, 65, 130):
        # n = 130: sorting moves the empty rows into the 2-row last slice, which then stores nothing:
        # 2 x 512 entries against 3 x 512, below the 0.85 the sorted plan needs
        out.append(_case(f"edges-{n}", ("edges", n), **dict(PLAIN, sorted=n == 130), max_bases=1, nsegs=4))
        out.append(_case(f"edges-{n}-sell", ("edges", n), {"pls.sell_d16": "0"}, **SELL))
    for n in (1100, 1111):
        g = wide_groups_expected(n)
        for l in (1, 2, 4, 8, 16, 32, 64):
            out.append(_case(f"wide-{n}-lpr{l}", ("wide", n), {"pls.d16_wide_lpr": str(l)},
                             **dict(PLAIN, multi=g * l if l > 1 else 0), wide_groups=g, max_bases=1))
    srt = dict(PLAIN, sorted=True)
    for l, multi in ((1, 0), (2, 26), (4, 51), (8, 101), (16, 202)):
        out.append(_case(f"sigma-lpr{l}", ("sigma", 2085), {"pls.d16_sorted_lpr": str(l)}, **dict(srt, multi=multi),
                         mixed_lanes=l > 1, max_bases=1))
    out.append(_case("sigma-window64", ("sigma", 2085), {"pls.d16_sigma": "64"}, **dict(srt, multi="all")))
    out.append(_case("sigma-off", ("sigma", 2085), {"pls.d16_sigma": "0"}, **PLAIN))
    out.append(_case("sigma-pad", ("sigma", 2085), {"pls.d16_sigma_pad": "2.0"}, **PLAIN))
    out.append(_case("sigma-sell", ("sigma", 2085), {"pls.sell_d16": "0"}, **SELL))
    out.append(_case("sigma-interleaved", ("sigma", 2085), interleaved=True, d16=True, fallback=False))
    out.append(_case("ramp", ("ramp",), **PLAIN, groups_of_8=(1, 2, 3, 4, 5)))
    out.append(_case("dense-row", ("dense_row",), rounded=False, **dict(srt, multi=2), max_bases=1))
    out.append(_case("dense-row-sell", ("dense_row",), {"pls.sell_d16": "0"}, rounded=False, **SELL))
    for k in (4, 5, 8):
        out.append(_case(f"segments-{k}", ("segments", k), **PLAIN, max_bases=k, nsegs=4 if k == 4 else 8))
    out.append(_case("segments-9", ("segments", 9), d16=False, fallback=True, max_bases=9, b3=False, rcm=False))
    out.append(_case("segments-4-segs8", ("segments", 4), {"pls.d16_segs": "8"}, **PLAIN, max_bases=4, nsegs=8))
    out.append(_case("delta-edge", ("delta_edge",), **PLAIN, max_bases=2, nsegs=4))
    b3 = {"pls.spmv_b3": "1"}
    out.append(_case("b3-all", ("b3_all",), b3, d16=True, b3=True, singles=0, d16_slices=0, rcm=False))
    out.append(_case("b3-mixed", ("b3_mixed",), b3, d16=True, b3=True, singles=90, mixed_lanes=True, rcm=False))
    out.append(_case("b3-minor", ("b3_minor",), b3, d16=True, b3=False, fallback=False, rcm=False))
    # spmv_rcm 0: without B3 this size is open to the RCM relabelling, which would bring the 9 far
    # columns together and fit D16 after all
    out.append(_case("b3-nine", ("b3_nine",), dict(b3, **{"pls.spmv_rcm": "0"}), d16=False, b3=False, fallback=True, max_bases=9, rcm=False))
    out.append(_case("rcm-auto", ("sigma", RCM_N), d16=True, rcm=True, b3=False))
    out.append(_case("rcm-off", ("sigma", RCM_N), {"pls.spmv_rcm": "0"}, d16=True, rcm=False, sorted=True))
    out.append(_case("rcm-forced-uniform", ("uniform",), {"pls.spmv_rcm": "1"}, d16=True, rcm=True, sorted=False))
    out.append(_case("rcm-uniform-auto", ("uniform",), **PLAIN))
    out.append(_case("rcm-components", ("two_components",), d16=True, rcm=True))
    out.append(_case("rcm-source-row", ("source_row",), {"pls.spmv_rcm": "1"}, d16=True, rcm=True))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
UNROLL_CASES = ("sigma-lpr2", "ramp")          # run with pls.d16_unroll 1, 2 and 4
XCD_CASES = ("sigma-lpr2", "segments-8")       # run with pls.d16_xcd 1 against 0


# ---------------------------------------------------------------------- data --
def index_sets(case, n):
    """(is_s, is_f, is_p, perm): perm[internal] = caller's index, the order pls_create gives the
    rows (2-way: s, then f and p merged ascending)."""
    if case.interleaved:
        sets = [np.arange(k, n, 3) for k in range(3)]
    else:
        a, b = (n + 2) // 3, (2 * n + 2) // 3
        sets = [np.arange(0, a), np.arange(a, b), np.arange(b, n)]
    perm = np.concatenate((sets[0], np.sort(np.concatenate((sets[1], sets[2])))))
    return sets[0].astype(np.int32), sets[1].astype(np.int32), sets[2].astype(np.int32), perm


def matrix(case, kind):
    """(A, x) of the case with "int" or "normal" values."""
    A = pattern(*case.pattern).copy()
    rng = np.random.default_rng(case.seed + (0 if kind == "int" else 1000))
    if kind == "int":
        A.data[:] = rng.integers(1, 9, A.nnz) * rng.choice((-1.0, 1.0), A.nnz)
        x = rng.integers(-16, 17, A.shape[0]).astype(np.float64)
    else:
        A.data[:] = rng.standard_normal(A.nnz)
        x = rng.standard_normal(A.shape[0])
    return A, x


def internal(A, perm):
    """The matrix in the internal order, as pls_create uploads it."""
    if np.array_equal(perm, np.arange(len(perm))):
        return A
    return A[perm][:, perm].tocsr()


def exact_product(A, x):
    """A x in int64 arithmetic (integer data)."""
    Ai = sp.csr_matrix((A.data.astype(np.int64), A.indices, A.indptr), shape=A.shape)
    return Ai @ x.astype(np.int64)
