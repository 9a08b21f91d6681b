"""Edge shapes for the exact-LU family -- the band / SPIKE kernels (csrc/band.hip), the dense
Gauss-Jordan inverse with threshold pivoting (csrc/dense.hip), the envelope path and the multifrontal
path of make_lu -- one table for the CPU tests of the cases' preconditions (tests/test_lu_cases.py) and
the device tests (tests/test_gpu_lu_conformance.py).

A case is a square K of lower / upper scalar bandwidth (kl, ku), used as the solid block of
sweep_cases.system(K) = block_diag(K, I_32, I_32) with A = P, no coupling, the 2-way ``pc type
diagonal`` and ``preonly`` inner solves: the block PC's apply is [K^-1 x_s, x_fp].  A band case's
``runs`` maps a value of pls.band_spike_plen ("auto": unset) to the SPIKE partition length and the
partition sizes the ``[band lu]`` line must report.  Sizes are the smallest that reach the branch the
case is there for ("LU conformance cases").

Data sets (``data``):

"int"     The factors come first.  Row and column i have the class i % 4.  L is unit lower; row i
          holds up to 6 entries from {+1, -1} at columns j with i - kl <= j < i and j % 4 < i % 4, the
          band edge i - kl among them wherever its class allows.  U is the transpose of the same
          construction with ku, diag(U) from {1/2, 1, 2, -1}.  K = L U, the whole product on its
          structural pattern (entries whose terms cancel stay stored as zeros).  A distance that is a
          multiple of 4 joins two rows of one class, so where kl (ku) is one, no +-1 sits at the band
          edge; K therefore stores both edge diagonals in full, as explicit zeros where the product
          has no entry: the structural bandwidth -- what csr_bandwidths reads -- is the one the case
          names.  y* integer in [-16, 16], x = K y*.
          L - I and D^-1 U - I are nilpotent of index 4 (a path climbs through the classes), so
          L^-1 = I - N + N^2 - N^3 and U^-1 stay small dyadic numbers; so does every leading or
          trailing block of them, and with them every partial sum of the tile LU, of Dl, Du, Gl, Gu,
          of the spikes, of the Gauss-Jordan inverse and of both sweeps: exact in any order.  Every
          |l_ij| is 1, so the dense path's threshold rule exchanges nothing.
"swap"    Dense cases only.  No column of class 3 has an entry below the diagonal of L.  K' is K with
          rows j and s > j exchanged for the listed class-3 j (the diagonal stored explicitly, 0
          included): at step j the diagonal is exactly 0 and the one nonzero candidate is the original
          row j at position s, so the pivot search must undo exactly that permutation.  x = K' y*.
"normal"  K's pattern with off-diagonals -U(0.2, 1), diagonal = row abs sum + U(0.05, 0.5), x standard
          normal; the reference is a float64 LU solve refined with np.longdouble residuals until the
          longdouble residual stops falling.
"""
import functools
import zlib
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from sweep_cases import NFP, PARAMS, coords, system  # noqa: F401  (shared with the device tests)

PER_ROW = 6
DIAG_U = (0.5, 1.0, 2.0, -1.0)
DYADIC_BITS = 20  # inverses: multiples of 2^-20 below 2^20 -- 40 bits, exact in float64 sums of any order
ND_LEAVES = ("8", "64")
PIVOT_U = 0.01  # pls.lu_pivot_threshold's default

# ------------------------------------------------------------------ the runtime's geometry, restated --
TILE_ROWS = 64  # band.hip BT, dense.hip DB
SPIKE_CG = 4    # band.hip: spike tiles per tail workgroup


def tile_geometry(n, kl, ku):
    """(nb, bl, bu) as the PCBandLU constructor computes them from the scalar bandwidths."""
    return -(-n // TILE_ROWS), -(-kl // TILE_ROWS), -(-ku // TILE_ROWS)


def bandwidths(K):
    """csr_bandwidths: first and last stored column of every row (explicit zeros count)."""
    n = K.shape[0]
    kl = ku = 0
    for i in range(n):
        a, b = K.indptr[i], K.indptr[i + 1]
        if b > a:
            kl = max(kl, i - int(K.indices[a]))
            ku = max(ku, int(K.indices[b - 1]) - i)
    return kl, ku


def spike_partitions(nb, bl, bu, requested):
    """(plen, partition sizes) as the PCBandLU constructor chooses them; requested: pls.band_spike_plen
    (-1: auto, about 16 partitions).  A partition is at least the wider triangle's tiles and a whole
    number of two-position super-rows; one partition (or no band at all) means no SPIKE: plen 0."""
    bwmax = max(bl, bu, 1)
    pl = max(bwmax, -(-nb // 16)) if requested < 0 else requested
    if pl > 0:
        pl = max(pl, bwmax)
        pl += pl & 1
    if not (pl > 0 and pl < nb and (bl > 0 or bu > 0)):
        return 0, (nb,)
    return pl, tuple(min(pl, nb - k) for k in range(0, nb, pl))


def tail_groups(bw):
    """Workgroups per tail position of launch_spike_apply."""
    return -(-bw // SPIKE_CG)


def pivot_rule(A, u=PIVOT_U):
    """panel_pivot's selection rule (csrc/dense.hip) as a right-looking LU of the dense A over every
    remaining row: column j keeps its diagonal row while |a_jj| >= u max_{i >= j} |a_ij|, else it takes
    the largest candidate, the smaller row on a tie.  Returns (rows exchanged, pivots below u x the
    column's largest entry, zero columns, the row order) -- the three counts of the [dense lu] line (the
    dense block has no update rows, so the second is 0 by construction of the rule: amax < u amax)."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    perm = np.arange(n)
    exchanged = below = zero = 0
    for j in range(n):
        col = np.abs(A[j:, j])
        amax = float(col.max())
        sel = j
        if amax > 0.0 and col[0] < u * amax:
            sel = j + int(np.argmax(col))  # (argmax: the first, i.e. smaller, row of a tie)
        exchanged += sel != j
        below += amax < u * amax
        zero += amax == 0.0
        if sel != j:
            A[[j, sel]] = A[[sel, j]]
            perm[[j, sel]] = perm[[sel, j]]
        if A[j, j] != 0.0:
            l = A[j + 1:, j] / A[j, j]
            A[j + 1:, j] = l
            A[j + 1:, j + 1:] -= np.outer(l, A[j, j + 1:])
    return int(exchanged), int(below), int(zero), perm


# ------------------------------------------------------------------ cases --
@dataclass(frozen=True)
class Case:
    id: str
    n: int
    kl: int
    ku: int
    geometry: tuple = None       # (nb, bl, bu) the [band lu] line must report
    runs: dict = field(hash=False, default_factory=dict)  # pls.band_spike_plen -> (plen, partition sizes)
    swaps: tuple = ()            # dense "swap" data: (j, s) row exchanges, j of class 3
    threshold: str = None        # dense: pls.lu_pivot_threshold (None: the default)
    reaches: str = ""


BAND_CASES = [
    Case("one-tile", 40, 5, 5, (1, 1, 1), {"auto": (0, (1,)), "0": (0, (1,))},
         reaches="nb == 1, no partitions"),
    Case("diagonal", 130, 0, 0, (3, 0, 0), {"auto": (0, (3,))},
         reaches="bl == bu == 0"),
    Case("lower-only", 321, 70, 0, (6, 2, 0), {"auto": (2, (2, 2, 2)), "0": (0, (6,)), "2": (2, (2, 2, 2))},
         reaches="bu == 0 (pl > 0, pu == 0); padding"),
    Case("upper-only", 321, 0, 70, (6, 0, 2), {"auto": (2, (2, 2, 2)), "0": (0, (6,)), "2": (2, (2, 2, 2))},
         reaches="bl == 0; padded tile row first in the backward sweep"),
    Case("tile-edges", 256, 64, 65, (4, 1, 2), {"auto": (2, (2, 2)), "0": (0, (4,))},
         reaches="bandwidth 64 -> bl 1, 65 -> bu 2; n % 64 == 0; even nb"),
    Case("odd-nb", 447, 130, 70, (7, 3, 2), {"auto": (4, (4, 3)), "0": (0, (7,)), "3": (4, (4, 3))},
         reaches="nb == 7, inactive second group; plen 3 becomes 4; P == 2"),
    Case("wide", 1217, 260, 260, (20, 5, 5),
         {"auto": (6, (6, 6, 6, 2)), "0": (0, (20,)), "8": (8, (8, 8, 4)), "10": (10, (10, 10))},
         reaches="bw == 5 > SPIKE_CG; last partition < bw; P == 2"),
    Case("long-narrow", 2112, 40, 40, (33, 1, 1),
         {"auto": (4, (4,) * 8 + (1,)), "0": (0, (33,)), "2": (2, (2,) * 16 + (1,))},
         reaches="nb == 33; auto plen 3 becomes 4; P == 9; last partition one position; bw == 1"),
    Case("skewed", 641, 40, 250, (11, 1, 4), {"auto": (4, (4, 4, 3)), "0": (0, (11,))},
         reaches="bl == 1, bu == 4; one plen serves both triangles"),
]

DENSE_CASES = (
    [Case(f"dense-{n}", n, n - 1, n - 1) for n in (1, 2, 63, 64, 65, 129, 200)]
    + [Case("dense-200-u0", 200, 199, 199, threshold="0"),
       Case("swap-in-tile", 200, 199, 199, swaps=((7, 40),), reaches="one exchange inside tile 0"),
       Case("swap-tile0-tile2", 200, 199, 199, swaps=((11, 150),), reaches="partner two tiles later"),
       Case("swap-into-last", 200, 199, 199, swaps=((67, 195),), reaches="partner in the last partial tile (m < 64)"),
       Case("swap-two", 200, 199, 199, swaps=((7, 40), (23, 50)), reaches="two exchanges in one tile")])
CASES = BAND_CASES + DENSE_CASES
BY_ID = {c.id: c for c in CASES}


def exact_kind(case):
    return "swap" if case.swaps else "int"


def requested_plen(run):
    return -1 if run == "auto" else int(run)


def options(path, run=None, leaf=None, threshold=None):
    """The option database of one handle: preonly + lu on the solid block through the forced path,
    preonly + ilu on the fp block (the identity), both view lines."""
    db = {"global_ksp_type": "gmres", "global_ksp_pc_side": "right", "pls.lu_view": "1", "pls.ilu_view": "1",
          "s_ksp_type": "preonly", "s_pc_type": "lu", "fp_ksp_type": "preonly", "fp_pc_type": "ilu",
          "pls.lu_path": path}
    if run is not None and run != "auto":
        db["pls.band_spike_plen"] = run
    if leaf is not None:
        db["pls.lu_nd_leaf"] = leaf
    if threshold is not None:
        db["pls.lu_pivot_threshold"] = threshold
    return db


# ------------------------------------------------------------------ data --
def _seed(case, kind):
    return zlib.crc32(("lu " + case.id + kind).encode())


def _unit_lower(n, k, rng):
    """The strictly lower part: row i holds up to PER_ROW entries from {+1, -1} at columns j with
    i - k <= j < i and j % 4 < i % 4, the band edge i - k among them where its class allows."""
    rows, cols = [], []
    for i in range(1, n):
        j = np.arange(max(0, i - k), i)
        j = j[j % 4 < i % 4]
        if j.size == 0:
            continue
        pick = rng.choice(j, min(PER_ROW, j.size), replace=False)
        if j[0] == i - k and j[0] not in pick:
            pick[0] = j[0]
        rows.append(np.full(pick.size, i))
        cols.append(pick)
    if not rows:
        return sp.csr_matrix((n, n))
    r, c = np.concatenate(rows), np.concatenate(cols)
    return sp.csr_matrix((rng.choice([-1.0, 1.0], r.size), (r, c)), shape=(n, n))


def _stored(n, groups):
    """CSR with exactly the given (rows, cols, values) triples stored, zeros included (the callers give
    every coordinate once)."""
    r = np.concatenate([g[0] for g in groups]).astype(np.int64)
    c = np.concatenate([g[1] for g in groups]).astype(np.int64)
    v = np.concatenate([g[2] for g in groups]).astype(np.float64)
    order = np.argsort(r * n + c, kind="stable")
    r, c, v = r[order], c[order], v[order]
    assert np.all(np.diff(r * n + c) > 0)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))])
    return sp.csr_matrix((v, c.astype(np.int32), indptr), shape=(n, n))


def _with_band_edges(K, kl, ku):
    """K with the band edges (i, i - kl), (i, i + ku) stored (as zeros where K has no entry there)."""
    n = K.shape[0]
    r, c = coords(K)
    have = set((r * n + c).tolist())
    i = np.arange(n)
    er = np.concatenate([i[kl:], i[:n - ku]])
    ec = np.concatenate([i[kl:] - kl, i[:n - ku] + ku])
    # (an edge of width 0 is the diagonal, which K stores: the two halves never name one new entry twice)
    new = np.array([k not in have for k in (er * n + ec).tolist()], dtype=bool)
    er, ec = er[new], ec[new]
    return _stored(n, [(r, c, K.data), (er, ec, np.zeros(er.size))])


@dataclass
class Data:
    K: sp.csr_matrix   # the solid block (explicit zeros stored)
    x: np.ndarray      # n + 64: the block PC's input
    y: np.ndarray      # the reference solution (int, swap: y*, float64; normal: np.longdouble)
    L: sp.csr_matrix = None  # int, swap: the factors K (before the row exchanges) was built from
    U: sp.csr_matrix = None
    e: np.ndarray = None     # int, swap: another integer vector (second_rhs: -2 x + e)


@functools.lru_cache(maxsize=None)
def _factors(case_id):
    case = BY_ID[case_id]
    rng = np.random.default_rng(_seed(case, "int"))
    n = case.n
    L = (_unit_lower(n, case.kl, rng) + sp.identity(n, format="csr")).tocsr()
    U = (_unit_lower(n, case.ku, rng).T + sp.diags(rng.choice(DIAG_U, n))).tocsr()
    # the structural pattern of the product (|L| |U| cannot cancel), then its values
    S = (abs(L) @ abs(U)).tocsr()
    S.sort_indices()
    V = (L @ U).tocsr()
    V.sort_indices()
    r, c = coords(S)
    vr, vc = coords(V)
    at = np.minimum(np.searchsorted(vr * n + vc, r * n + c), max(vr.size - 1, 0))
    val = np.where((vr * n + vc)[at] == r * n + c, V.data[at], 0.0)
    K = _with_band_edges(sp.csr_matrix((val, S.indices, S.indptr), shape=(n, n)), case.kl, case.ku)
    return L, U, K, rng


def swap_rows(K, swaps):
    """K with rows j and s exchanged for every (j, s), the diagonal stored explicitly."""
    n = K.shape[0]
    perm = np.arange(n)
    for j, s in swaps:
        perm[[j, s]] = perm[[s, j]]
    Kp = K[perm].tocsr()
    Kp.sort_indices()
    r, c = coords(Kp)
    have = set((r * n + c).tolist())
    d = np.array([i for i in range(n) if i * n + i not in have], dtype=np.int64)
    return _stored(n, [(r, c, Kp.data), (d, d, np.zeros(d.size))])


def refined_solve(K, x):
    """K^-1 x: float64 sparse LU, refined with np.longdouble residuals until the residual stops falling.
    Returns (the np.longdouble reference, the plain float64 solve)."""
    n = K.shape[0]
    lu = spla.splu(K.tocsc()) if n > 1 else None
    solve = lu.solve if lu is not None else (lambda b: b / K.toarray()[0, 0])
    r, c = coords(K)
    v, xl = K.data.astype(np.longdouble), x.astype(np.longdouble)

    def residual(y):
        out = xl.copy()
        np.subtract.at(out, r, v * y[c])
        return out

    y0 = solve(x)
    y = y0.astype(np.longdouble)
    res = residual(y)
    best = float(np.abs(res).max())
    for _ in range(20):
        cand = y + solve(res.astype(np.float64)).astype(np.longdouble)
        rc = residual(cand)
        if float(np.abs(rc).max()) >= best:
            break
        y, res, best = cand, rc, float(np.abs(rc).max())
    return y, y0


@functools.lru_cache(maxsize=None)
def _data(case_id, kind):
    case = BY_ID[case_id]
    n = case.n
    L, U, K, _ = _factors(case_id)
    rng = np.random.default_rng(_seed(case, kind))
    if kind == "normal":
        if case.swaps:
            raise ValueError("the swap cases have no rounded data")
        r, c = coords(K)
        v = -rng.uniform(0.2, 1.0, r.size)
        v[r == c] = 0.0
        rowsum = np.bincount(r, weights=np.abs(v), minlength=n)
        v[r == c] = rowsum + rng.uniform(0.05, 0.5, n)
        Kn = sp.csr_matrix((v, K.indices, K.indptr), shape=K.shape)
        x = rng.standard_normal(n)
        return Data(Kn, np.concatenate([x, rng.standard_normal(NFP)]), refined_solve(Kn, x)[0])
    if (kind == "swap") != bool(case.swaps):
        raise ValueError(f"{case.id} has no {kind} data")
    if case.swaps:
        K = swap_rows(K, case.swaps)
    y = rng.integers(-16, 17, n).astype(np.float64)
    e = rng.integers(-16, 17, n).astype(np.float64)
    x_fp = rng.integers(-16, 17, NFP).astype(np.float64)
    return Data(K, np.concatenate([K @ y, x_fp]), y, L, U, e)


def data(case, kind):
    return _data(case.id, kind)


# ------------------------------------------------------------------ references --
def exact_inverses(L, U):
    """(L^-1, U^-1) dense by the nilpotent series: exact while the entries stay small dyadic numbers."""
    n = L.shape[0]
    I = sp.identity(n, format="csr")
    N = (L - I).tocsr()
    d = U.diagonal()
    M = (sp.diags(1.0 / d) @ U - I).tocsr()  # (1 / d: +-1, +-2, 1/2 -- exact)
    N2, M2 = N @ N, M @ M
    assert (N2 @ N2).count_nonzero() == 0 and (M2 @ M2).count_nonzero() == 0  # index 4
    Li = (I - N + N2 - N2 @ N).toarray()
    Ui = ((I - M + M2 - M2 @ M) @ sp.diags(1.0 / d)).toarray()
    return Li, Ui


def row_order(case):
    """perm with K' = K[perm] for the case's row exchanges (the identity without)."""
    perm = np.arange(case.n)
    for j, s in case.swaps:
        perm[[j, s]] = perm[[s, j]]
    return perm


@functools.lru_cache(maxsize=None)
def _second(case_id):
    case = BY_ID[case_id]
    d = data(case, exact_kind(case))
    n = case.n
    Li, Ui = exact_inverses(d.L, d.U)
    e = np.empty(n)
    e[row_order(case)] = d.e  # K' = Pi K: K'^-1 e = K^-1 Pi^T e
    x2 = -2.0 * d.x
    x2[:n] += d.e
    return x2, -2.0 * d.y + Ui @ (Li @ e)


def second_rhs(case):
    """(x2, y2*) of the exact data's second right-hand side: x2 = -2 x + e on the solid block (e the
    data's other integer vector; -2 x_fp on the fp block), y2* = -2 y* + K^-1 e by the exact inverses --
    multiples of 1/16, not integers."""
    return _second(case.id)


def is_dyadic(M, bits=DYADIC_BITS):
    """Every entry a multiple of 2^-bits below 2^bits in magnitude."""
    s = np.asarray(M) * 2.0 ** bits
    return bool(np.all(s == np.round(s)) and np.abs(M).max(initial=0.0) < 2.0 ** bits)
