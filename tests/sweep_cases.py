"""Adversarial patterns for the ILU(0) sweep kernels, one table for the CPU tests of the cases'
preconditions (tests/test_sweep_cases.py) and the device tests (tests/test_gpu_sweep_conformance.py).

A case is a square pattern K (symmetric pattern, full diagonal) used as the solid block of
block_diag(K, I_32, I_32) with A = P, no coupling, the 2-way ``pc type diagonal`` and ``preonly`` inner
solves: the block PC's apply is [ILU0(K)^-1 x_s, x_fp].  ``runs`` maps the name of a forced option set
(RUNS) to the sweep kind the solid block's ``[pls ilu]`` line must report for it, fall-backs
included; ``records`` are the window kinds' stream records per wave (L, U).  Sizes are the smallest
that reach the branch the case is there for ("Sweep conformance cases").

Three data sets per case (``data``):

"int"     The factors come first: L unit lower and U upper on the (block-truncated) pattern, off-
          diagonals from {+-1, +-2, +-3}, diag(U) from {1/2, 1, 2, 4}; K = (L U) restricted to the
          pattern (explicit zeros kept, cross-block entries arbitrary integers); y* integer in
          [-16, 16], t = U y*, x_s = L t.  ILU(0) of K is then exactly (L, U), and every partial sum
          of the factorization and of both substitutions is a multiple of 1/2 far below 2^53: exact
          in every order.
"unit"    As "int" with every off-diagonal and every diag(U) entry +-1, for the four kinds that invert
          64-row window triangles explicitly: with the "int" values an inverse's entries pass 2^53
          (they grow like 6^k along a chain of k rows) and the windowed solve returns inf and NaN on
          the CPU too; with units an entry of a window's inverse is a signed count of paths inside
          the window, an integer of modest size, so the windowed solve is exact as well.
"normal"  Off-diagonals -U(0.2, 1), diagonal 2 (row abs sum) + U(0.05, 0.5), x standard normal; the
          reference is ILU(0) and both substitutions in np.longdouble (``longdouble_solve``).
"""
import functools
import zlib
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from oracle.petsc import bjacobi_block_sizes

NFP = 64  # the fp block: I_32 (f) and I_32 (p)

# ------------------------------------------------------------------ option sets --
RUNS = {
    "default": {},
    "lds": {"pls.sweep_window": "0", "pls.sweep_chain": "0"},
    "levels": {"pls.ilu_lds": "0"},
    "levels-csr": {"pls.ilu_lds": "0", "pls.ilu_gmem": "-2"},
    "gmem": {"pls.ilu_gmem": "1", "pls.ilu_ring": "0"},
    "ring": {"pls.ilu_gmem": "1"},
    "chain": {"pls.sweep_chain": "1"},
    "window": {"pls.sweep_window": "1"},
    "window-ring": {"pls.sweep_window": "1", "pls.window_ring": "1"},
    "gmem-window-ring": {"pls.ilu_gmem": "1", "pls.sweep_window": "1"},
    "mixed": {"pls.ilu_gmem": "1", "pls.sweep_window": "1", "pls.window_mixed": "1"},
    "swin": {"pls.ilu_gmem": "1", "pls.sweep_swin": "1"},
    # lanes per row and levels in flight of the LDS sweep (pls.sweep_lpr is read by bjacobi: one block)
    "lds-lpr1": {"pls.sweep_window": "0", "pls.sweep_chain": "0", "pls.sweep_lpr": "1"},
    "lds-lpr2": {"pls.sweep_window": "0", "pls.sweep_chain": "0", "pls.sweep_lpr": "2"},
    "lds-lpr4": {"pls.sweep_window": "0", "pls.sweep_chain": "0", "pls.sweep_lpr": "4"},
    "lds-depth2": {"pls.sweep_window": "0", "pls.sweep_chain": "0", "pls.sweep_depth": "2"},
    "lds-depth3": {"pls.sweep_window": "0", "pls.sweep_chain": "0", "pls.sweep_depth": "3"},
    "lds-depth4": {"pls.sweep_window": "0", "pls.sweep_chain": "0", "pls.sweep_depth": "4"},
    # the window sweep's data in flight and records per wave
    "window-depth2": {"pls.sweep_window": "1", "pls.window_depth": "2"},
    "window-depth3": {"pls.sweep_window": "1", "pls.window_depth": "3"},
    "window-kpw8": {"pls.sweep_window": "1", "pls.window_kpw": "8"},
    "window-ring-kpw8": {"pls.sweep_window": "1", "pls.window_ring": "1", "pls.window_kpw": "8"},
}
KINDS = ("levels", "levels-csr", "lds", "gmem", "ring", "chain", "window", "window-ring", "levels+window-ring", "swin")
LEVEL_KINDS = ("levels", "levels-csr", "lds", "gmem", "ring", "chain")
INVERSE_KINDS = ("window", "window-ring", "levels+window-ring", "swin")

# the kernels' limits (csrc: ilu_lds_max_rows, ilu_window_max_rows, ilu_window_ring_max_rows,
# ilu_window_ring_rows - 64, ilu_ring_chunk, ilu_ring_slots, ilu_window_max_entries, SW_P, RING_P)
LDS_ROWS, WINDOW_ROWS, WINDOW_RING_ROWS = 20480, 19904, 65472
WINDOW_RING_REACH, RING_CHUNK, RING_SLOTS, WINDOW_ENTRIES, LANE_ENTRIES = 16384 - 64, 4096, 16384, 32, 7


# ------------------------------------------------------------------ patterns --
def _sym(n, rows, cols):
    """The symmetric pattern with a full diagonal that holds (rows, cols)."""
    i = np.arange(n)
    r = np.concatenate([np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), i])
    c = np.concatenate([np.asarray(cols, dtype=np.int64), np.asarray(rows, dtype=np.int64), i])
    M = sp.csr_matrix((np.ones(r.size), (r, c)), shape=(n, n))
    M.sum_duplicates()
    M.sort_indices()
    M.data[:] = 1.0
    return M


def _band(n):
    i = np.arange(1, n)
    return [i], [i - 1]


def _cat(rows, cols):
    return np.concatenate(rows), np.concatenate(cols)


def diag(n):
    return _sym(n, [], [])


def chain(n):
    return _sym(n, *_cat(*_band(n)))


def twolevel(n):
    """Rows [0, n/2) hold their diagonal only; row i of [n/2, n) has 1 + i % 12 entries in the first half."""
    h = n // 2
    rng = np.random.default_rng(41)
    rows, cols = [], []
    for i in range(h, n):
        c = rng.choice(h, 1 + i % 12, replace=False)
        rows.append(np.full(c.size, i))
        cols.append(c)
    return _sym(n, *_cat(rows, cols))


LANE_COUNTS = (0, 1, 7, 8, 14, 15, 28, 29, 56, 57, 112, 113, 224, 225)


def lanes_rows(n=3000):
    """{count: row} of the rows of lanes(n) that carry exactly `count` entries in L, and in U."""
    inL = {c: (0 if c == 0 else 2000 + 40 * k) for k, c in enumerate(LANE_COUNTS)}
    inU = {c: (n - 1 if c == 0 else 20 + 16 * k) for k, c in enumerate(LANE_COUNTS)}
    return inL, inU


def lanes(n=3000):
    """Band i +- 1.  The rows of lanes_rows carry the counts of LANE_COUNTS: the L rows (2000 ...) take
    their further columns from [300, 1000), the U rows (20 ...) theirs from [1100, 1900) -- rows of
    those ranges get at most 13 further entries in the other triangle."""
    rng = np.random.default_rng(42)
    rows, cols = _band(n)
    inL, inU = lanes_rows(n)
    for c in LANE_COUNTS[2:]:
        rows.append(np.full(c - 1, inL[c]))
        cols.append(300 + rng.choice(700, c - 1, replace=False))
        rows.append(1100 + rng.choice(800, c - 1, replace=False))  # (given as their lower mirror images)
        cols.append(np.full(c - 1, inU[c]))
    return _sym(n, *_cat(rows, cols))


WINDOW_COUNTS = (16, 17, 24, 25, 32)


def win_rows():
    """{count: row} of win_records' rows with exactly `count` off-window entries in L, and in U (rows in
    the middle of their 64-row window: both band neighbours inside it)."""
    return ({c: 64 * (20 + k) + 32 for k, c in enumerate(WINDOW_COUNTS)},
            {c: 64 * (1 + k) + 32 for k, c in enumerate(WINDOW_COUNTS)})


WIN33_ROW = 64 * 6 + 32


def win_records(n, max_l, max_u, row33=False):
    """Band i +- 1.  Rows 1312 + 64 k have 16, 17, 24, 25, 32 (those <= max_l) entries in [500, 1000),
    left of their window; rows 96 + 64 k as many (<= max_u) in [1700, 2000), right of theirs.  By
    symmetry the rows of those two ranges get at most 5 off-window entries (6 with the band).
    row33: row 416 with 33 off-window entries in U."""
    rng = np.random.default_rng(43)
    rows, cols = _band(n)
    inL, inU = win_rows()
    for c in WINDOW_COUNTS:
        pl, pu = 500 + rng.choice(500, c, replace=False), 1700 + rng.choice(300, c, replace=False)
        if c <= max_l:
            rows.append(np.full(c, inL[c]))
            cols.append(pl)
        if c <= max_u:
            rows.append(pu)
            cols.append(np.full(c, inU[c]))
    if row33:
        rows.append(1700 + rng.choice(300, 33, replace=False))
        cols.append(np.full(33, WIN33_ROW))
    return _sym(n, *_cat(rows, cols))


def arrow(n=2000, long=400):
    """Band i +- 1; the last row has `long` entries in L (columns 0, 5, 10, ... and n - 2)."""
    rows, cols = _band(n)
    c = 5 * np.arange(long - 1)
    rows.append(np.full(c.size, n - 1))
    cols.append(c)
    return _sym(n, *_cat(rows, cols))


def far(n, *dist):
    """i - 1 and i - 70; every 97th row also i - d for every d of dist."""
    i = np.arange(n)
    rows, cols = [], []
    for d, sel in [(1, i), (70, i)] + [(d, i[i % 97 == 0]) for d in dist]:
        sel = sel[sel >= d]
        rows.append(sel)
        cols.append(sel - d)
    return _sym(n, *_cat(rows, cols))


def scattered(n, per_row, span, seed):
    """Band i +- 1 plus per_row lower entries per row at i - U[1, min(i, span)] (and their mirror images)."""
    rng = np.random.default_rng(seed)
    rows, cols = _band(n)
    i = np.repeat(np.arange(1, n), per_row)
    rows.append(i)
    cols.append(i - rng.integers(1, np.minimum(i, span) + 1))
    return _sym(n, *_cat(rows, cols))


# ------------------------------------------------------------------ cases --
@dataclass(frozen=True)
class Case:
    id: str
    pattern: tuple                 # (builder, args...)
    runs: dict = field(hash=False, default_factory=dict)  # RUNS name -> the kind the [pls ilu] line must report
    blocks: int = 1                # > 1: s_pc_type bjacobi with that many blocks
    records: tuple = None          # window kinds: stream records per wave (L, U) where pls.window_kpw is not set

    @property
    def n(self):
        return self.pattern[1]


# (fall-backs: diag-4100's level of 4,100 rows is wider than the ring chunk -- gmem for ring;
# lanes and arrow have rows too long for 16 lanes x 7 entries -- lds for chain -- and more than 32
# off-window entries -- no window kind; far and reach-16321 reach beyond 16,320 rows -- no window-
# ring; win33 -- chain or lds for window; 64 blocks and more keep their levels per block -- levels for
# levels-csr)
_LONG = {"default": "ring", "levels": "levels", "levels-csr": "levels-csr", "gmem": "gmem", "ring": "ring",
         "window": "ring", "gmem-window-ring": "ring", "mixed": "ring", "swin": "swin"}
_WIN = {"default": "window", "lds": "lds", "levels": "levels", "levels-csr": "levels-csr", "gmem": "gmem", "ring": "ring",
        "chain": "chain", "window": "window", "window-ring": "window-ring", "gmem-window-ring": "window-ring",
        "mixed": "levels+window-ring", "swin": "swin", "window-depth2": "window", "window-depth3": "window",
        "window-kpw8": "window", "window-ring-kpw8": "window-ring"}
_NOWIN = {"default": "lds", "lds": "lds", "levels": "levels", "levels-csr": "levels-csr", "gmem": "gmem", "ring": "ring",
          "chain": "lds", "window": "lds", "window-ring": "lds", "gmem-window-ring": "ring", "mixed": "ring",
          "swin": "swin"}
_LPR = {"lds-lpr1": "lds", "lds-lpr2": "lds", "lds-lpr4": "lds", "lds-depth2": "lds", "lds-depth3": "lds",
        "lds-depth4": "lds"}
_BLOCKS = {"default": "window", "lds": "lds", "levels": "levels", "levels-csr": "levels", "gmem": "gmem",
           "ring": "ring", "chain": "chain",
           "window": "window", "window-ring": "window-ring", "gmem-window-ring": "window-ring",
           "mixed": "levels+window-ring", "swin": "swin"}

CASES = [
    Case("diag-4100", ("diag", 4100), records=(4, 4),
         runs={"default": "lds", "lds": "lds", "levels": "levels", "levels-csr": "levels-csr", "gmem": "gmem",
               "ring": "gmem", "chain": "chain", "window": "window", "window-ring": "window-ring",
               "gmem-window-ring": "levels+window-ring", "mixed": "levels+window-ring", "swin": "swin"}),
    Case("diag-4096", ("diag", 4096), runs={"ring": "ring", "gmem": "gmem"}),
    Case("chain", ("chain", 1000), runs=_WIN, records=(4, 4)),
    Case("twolevel", ("twolevel", 2600), records=(4, 6),
         runs={"default": "lds", "lds": "lds", "levels": "levels", "levels-csr": "levels-csr", "gmem": "gmem",
               "ring": "ring", "chain": "chain", "window": "window", "window-ring": "window-ring",
               "gmem-window-ring": "levels+window-ring", "mixed": "levels+window-ring", "swin": "swin"}),
    Case("lanes", ("lanes", 3000), runs=dict(_NOWIN, **_LPR)),
    Case("win_records-4/8", ("win_records", 2000, 16, 32), runs=_WIN, records=(4, 8)),
    Case("win_records-6/4", ("win_records", 2000, 24, 16), runs=_WIN, records=(6, 4)),
    Case("win_records-8/6", ("win_records", 2000, 32, 24), runs=_WIN, records=(8, 6)),
    Case("win33", ("win_records", 2000, 16, 32, True),
         runs={"default": "chain", "lds": "lds", "chain": "chain", "window": "chain", "window-ring": "chain",
               "gmem-window-ring": "ring", "mixed": "ring", "swin": "swin"}),
    Case("arrow", ("arrow", 2000, 400), runs=_NOWIN),
    Case("far", ("far", 21000, 17000, 20900), runs=dict(_LONG, **{"window-ring": "ring"})),
    Case("reach-16320", ("far", 21000, 16320), records=(4, 4),
         runs=dict(_LONG, **{"default": "window-ring", "window": "window-ring", "window-ring": "window-ring",
                             "gmem-window-ring": "window-ring", "mixed": "levels+window-ring"})),
    Case("reach-16321", ("far", 21000, 16321), runs=dict(_LONG, **{"window-ring": "ring"})),
    Case("blocks-3", ("scattered", 1000, 3, 1000, 44), blocks=3, runs=dict(_BLOCKS, **{"levels-csr": "levels-csr"}),
         records=(4, 4)),
    Case("blocks-70", ("scattered", 4500, 3, 4500, 45), blocks=70, runs=_BLOCKS, records=(4, 4)),
    Case("blocks-100", ("scattered", 130, 3, 130, 46), blocks=100, runs=_BLOCKS, records=(4, 4)),
    Case("random", ("scattered", 5000, 3, 2000, 47), runs=_WIN, records=(4, 6)),
]
BY_ID = {c.id: c for c in CASES}
# the equalities the code claims (window-ring == window, pls.window_kpw 8 == the chosen records,
# pls.window_depth 2 == 3) and the factorization paths are checked on these
EQUALITY_CASES = ("win_records-4/8", "win_records-6/4", "win_records-8/6", "chain", "random")
FACTOR_CASES = ("lanes", "arrow", "random")
FACTOR_RUNS = {"dep0": {"pls.ilu_factor_dep": "0"}, "dep2": {"pls.ilu_factor_dep": "2"},
               "dep2-grid1": {"pls.ilu_factor_dep": "2", "pls.ilu_dep_grid": "1"},
               "dep2-stage0": {"pls.ilu_factor_dep": "2", "pls.ilu0_stage": "0"},
               "dep2-stage64": {"pls.ilu_factor_dep": "2", "pls.ilu0_stage": "64"},
               "dep0-stage0": {"pls.ilu_factor_dep": "0", "pls.ilu0_stage": "0"},
               "dep0-stage64": {"pls.ilu_factor_dep": "0", "pls.ilu0_stage": "64"}}

PARAMS = {"solver type": "gmres", "solver atol": 1e-8, "solver rtol": 1e-6, "solver maxiter": 100,
          "pc type": "diagonal", "inner ksp type": "preonly", "inner pc type": "ilu", "inner accel order": 0,
          "AAR order": 10, "AAR p": 5, "AAR omega": 1, "AAR beta": 1}


def options(case, run_options):
    """The option database of one handle: preonly inner solves, ilu (bjacobi where the case has blocks
    or the run sets pls.sweep_lpr, which only bjacobi reads) on the solid block, ilu on the fp block."""
    db = {"global_ksp_type": "gmres", "global_ksp_pc_side": "right", "pls.ilu_view": "1",
          "s_ksp_type": "preonly", "s_pc_type": "ilu", "fp_ksp_type": "preonly", "fp_pc_type": "ilu"}
    if case.blocks > 1 or "pls.sweep_lpr" in run_options:
        db.update({"s_pc_type": "bjacobi", "s_pc_bjacobi_blocks": str(case.blocks)})
    db.update(run_options)
    return db


@functools.lru_cache(maxsize=None)
def pattern(name, *args):
    return globals()[name](*args)


def block_starts(case):
    return np.concatenate([[0], np.cumsum(bjacobi_block_sizes(case.n, case.blocks))]).astype(np.int64)


def coords(M):
    """(row, column) of every stored entry in CSR order."""
    return np.repeat(np.arange(M.shape[0]), np.diff(M.indptr)), M.indices.astype(np.int64)


def truncated(case, M):
    """M without its cross-block entries (stored entries kept, explicit zeros included)."""
    if case.blocks == 1:
        return M
    r, c = coords(M)
    blk = np.searchsorted(block_starts(case), np.arange(case.n), side="right")
    keep = blk[r] == blk[c]
    T = sp.csr_matrix((M.data[keep], (r[keep], c[keep])), shape=M.shape)
    T.sort_indices()
    return T


def _seed(case, kind):
    return zlib.crc32((case.id + kind).encode())


def system(K):
    """block_diag(K, I_32, I_32) and its index sets."""
    n = K.shape[0]
    A = sp.block_diag([K, sp.identity(NFP)], format="csr")
    A.sort_indices()
    assert A.nnz == K.nnz + NFP  # (K's explicit zeros stay stored)
    i = np.arange(n + NFP, dtype=np.int32)
    return A, i[:n], i[n:n + NFP // 2], i[n + NFP // 2:]


def _triangles(r, c, f, n):
    """(L, U) of the factor values f at (r, c): L unit lower (its diagonal 1), U upper with f's diagonal."""
    lo, up = c < r, c >= r
    L = sp.csr_matrix((f[lo], (r[lo], c[lo])), shape=(n, n)) + sp.identity(n, format="csr")
    return L.tocsr(), sp.csr_matrix((f[up], (r[up], c[up])), shape=(n, n))


@dataclass
class Data:
    K: sp.csr_matrix   # the solid block (explicit zeros stored), cross-block entries included
    x: np.ndarray      # n + 64: the block PC's input
    y: np.ndarray      # the solid block's reference solution (int, unit: y*, float64; normal: np.longdouble)
    factors: np.ndarray = None  # int, unit: L + U - I on truncated(K)'s stored entries


@functools.lru_cache(maxsize=None)
def _data(case_id, kind):
    case = BY_ID[case_id]
    rng = np.random.default_rng(_seed(case, kind))
    P = pattern(*case.pattern)
    n = case.n
    r, c = coords(P)
    x_fp = rng.integers(-16, 17, NFP).astype(np.float64) if kind != "normal" else rng.standard_normal(NFP)
    if kind == "normal":
        v = -rng.uniform(0.2, 1.0, r.size)
        v[r == c] = 0.0
        rowsum = np.bincount(r, weights=np.abs(v), minlength=n)
        v[r == c] = 2.0 * rowsum + rng.uniform(0.05, 0.5, n)
        K = sp.csr_matrix((v, P.indices, P.indptr), shape=P.shape)
        x = rng.standard_normal(n)
        return Data(K, np.concatenate([x, x_fp]), longdouble_solve(truncated(case, K), x))
    # the factors on the truncated pattern, in its CSR order
    T = truncated(case, P)
    tr, tc = coords(T)
    f = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0] if kind == "int" else [-1.0, 1.0], tr.size)
    f[tr == tc] = rng.choice([0.5, 1.0, 2.0, 4.0] if kind == "int" else [-1.0, 1.0], n)
    L, U = _triangles(tr, tc, f, n)
    LU = (L @ U).tocsr()
    LU.sort_indices()
    pr, pc = coords(LU)
    # (every stored entry of T is an entry of L U; the product drops those whose terms cancel: explicit zeros of K)
    at = np.minimum(np.searchsorted(pr * n + pc, tr * n + tc), pr.size - 1)
    lu_at = np.where((pr * n + pc)[at] == tr * n + tc, LU.data[at], 0.0)
    # K: (L U) on the truncated pattern, arbitrary nonzero integers across blocks
    kv = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], r.size)
    key = np.searchsorted(r * n + c, tr * n + tc)
    kv[key] = lu_at
    K = sp.csr_matrix((kv, P.indices, P.indptr), shape=P.shape)
    y = rng.integers(-16, 17, n).astype(np.float64)
    x = L @ (U @ y)
    return Data(K, np.concatenate([x, x_fp]), y, f)


def data(case, kind):
    return _data(case.id, kind)


def int_factors(case, kind="int"):
    """(|L|, |U|) of the "int" or "unit" data as CSR matrices (for the magnitude bounds)."""
    T = truncated(case, pattern(*case.pattern))
    tr, tc = coords(T)
    return _triangles(tr, tc, np.abs(data(case, kind).factors), case.n)


# ------------------------------------------------------------------ references --
def diagonal_positions(M):
    r, c = coords(M)
    dg = np.nonzero(r == c)[0]
    assert dg.size == M.shape[0]
    return dg


def longdouble_solve(T, x):
    """(L U)^-1 x with the ILU(0) factors of T (natural order, T's pattern), all in np.longdouble."""
    n = T.shape[0]
    rp, ci = T.indptr.astype(np.int64), T.indices.astype(np.int64)
    lu = T.data.astype(np.longdouble)
    dg = diagonal_positions(T)
    pos = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        a, b = rp[i], rp[i + 1]
        pos[ci[a:b]] = np.arange(a, b)
        for k in range(a, dg[i]):
            j = ci[k]
            lik = lu[k] / lu[dg[j]]
            lu[k] = lik
            u0, u1 = dg[j] + 1, rp[j + 1]
            if u1 > u0:
                p = pos[ci[u0:u1]]
                m = p >= 0
                lu[p[m]] -= lik * lu[u0:u1][m]
        pos[ci[a:b]] = -1
    t = np.zeros(n, dtype=np.longdouble)
    xl = x.astype(np.longdouble)
    for i in range(n):
        a, d = rp[i], dg[i]
        t[i] = xl[i] - (lu[a:d] @ t[ci[a:d]] if d > a else 0)
    y = np.zeros(n, dtype=np.longdouble)
    for i in range(n - 1, -1, -1):
        d, b = dg[i], rp[i + 1]
        y[i] = (t[i] - (lu[d + 1:b] @ y[ci[d + 1:b]] if b > d + 1 else 0)) / lu[d]
    return y


def _invert_window(T, upper):
    """T^-1 of a window's triangle by row substitution, as csrc/ilu.cpp invert_window_triangle."""
    m = T.shape[0]
    X = np.zeros((m, m))
    if not upper:
        for i in range(m):
            X[i, :i] = -(T[i, :i] @ X[:i, :i])
            X[i, i] = 1.0
    else:
        for i in range(m - 1, -1, -1):
            X[i, i] = 1.0 / T[i, i]
            X[i, i + 1:] = -(T[i, i + 1:] @ X[i + 1:, i + 1:]) / T[i, i]
    return X


def windowed_solve(T, lu, bst, x):
    """The window kinds' solve in float64: per block, windows of 64 rows from the block's first row,
    y_w = T_w^-1 (b_w - A_off y_off) with the inverse of the window's triangle formed explicitly --
    the unit lower triangle of the factors ``lu`` (on T's pattern) forwards, then the upper one backwards."""
    n = T.shape[0]
    r, c = coords(T)
    Lo = sp.csr_matrix((np.where(c < r, lu, 0.0), T.indices, T.indptr), shape=T.shape)
    Up = sp.csr_matrix((np.where(c >= r, lu, 0.0), T.indices, T.indptr), shape=T.shape)
    wins = [(w0, min(w0 + 64, bst[b + 1])) for b in range(len(bst) - 1) for w0 in range(bst[b], bst[b + 1], 64)]
    t = np.zeros(n)
    for w0, w1 in wins:  # (t is zero from w0 on: Lo[w0:w1] @ t is the off-window part)
        Tw = Lo[w0:w1, w0:w1].toarray() + np.eye(w1 - w0)
        t[w0:w1] = _invert_window(Tw, False) @ (x[w0:w1] - Lo[w0:w1] @ t)
    y = np.zeros(n)
    for w0, w1 in reversed(wins):
        Tw = Up[w0:w1, w0:w1].toarray()
        y[w0:w1] = _invert_window(Tw, True) @ (t[w0:w1] - (Up[w0:w1] @ y))
    return y


# ------------------------------------------------------------------ LDS stream layout --
def lds_layout(case, upper, force_lpr=0, max_lpr=4):
    """build_lds_tri's (csrc/ilu.cpp) layout of one triangle in the numbers its pls.ilu_view 2 line
    prints: per block the fewest lanes per row (1, 2, 4; force_lpr pins them) whose share of the
    block's longest row is at most 7 entries, levels cut into slices of 64 / lanes rows (a level's rows
    ascending).  Returns (blocks, most levels of a block, most slices of a level, most slices beyond
    16 per level summed over a block's levels, that block, 7, most slices of a block whose lanes hold
    more than 7 entries) and the lanes per row of every block."""
    from oracle import native
    T = truncated(case, pattern(*case.pattern))
    r, c = coords(T)
    lens = np.bincount(r[(c > r) if upper else (c < r)], minlength=case.n)
    _, lvl = native.levels(T, lower=not upper)
    bst = block_starts(case)
    worst_lev = wmax = worst_inline = b_inl = worst_long = 0
    lprs = []
    for b in range(case.blocks):
        rows = np.arange(bst[b], bst[b + 1])
        mx = int(lens[rows].max())
        lpr = 1
        while lpr < max_lpr and -(-mx // lpr) > LANE_ENTRIES:
            lpr *= 2
        lpr = force_lpr or lpr
        lprs.append(lpr)
        per = 64 // lpr
        inl = lng = 0
        nlev = int(lvl[rows].max()) + 1
        for g in range(nlev):
            share = -(-lens[rows[lvl[rows] == g]] // lpr)
            slices = [int(share[k:k + per].max()) for k in range(0, share.size, per)]
            wmax = max(wmax, len(slices))
            inl += max(0, len(slices) - 16)
            lng += sum(s > LANE_ENTRIES for s in slices)
        if inl > worst_inline:
            worst_inline, b_inl = inl, b
        worst_lev, worst_long = max(worst_lev, nlev), max(worst_long, lng)
    return (case.blocks, worst_lev, wmax, worst_inline, b_inl, LANE_ENTRIES, worst_long), lprs


# (case, run): the LDS sweep's stream layout line is compared with lds_layout
LAYOUT_RUNS = (("lanes", "lds"), ("lanes", "lds-lpr1"), ("lanes", "lds-lpr2"), ("lanes", "lds-lpr4"),
               ("arrow", "lds"), ("twolevel", "lds"), ("diag-4100", "lds"), ("blocks-70", "lds"))
