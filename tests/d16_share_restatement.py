"""Shared delta streams of the SELL-64/D16 layout (option pls.d16_share; csrc/runtime.cpp:
d16_share; csrc/kernels.hip: k_d16_share_classes, k_d16_share_fill, k_d16_spmv), restated in numpy
on top of tests/spmv_layout_restatement.py.

The lanes of a slice whose encoded uint16 delta streams are equal over the slice's whole length L
(padding included; a lane without a row has the all-zero stream, and so has a lane with a single
entry) form a class.  C = classes of the slice, ids 0..C-1 ordered by lowest member lane.  The
shared stream holds one 16-B pack per class and 8-entry group,

    dls[dptr[slice] + (g * C + cls[slice * 64 + lane]) * 8 + k % 8]      g = k / 8

with dptr the prefix sums of C * L.  Values, bases, slice pointers and the row map stay as they are.
``share(L, E)`` computes all of it from the restated layout ``L`` and its plain streams ``E``;
``Shared.bytes`` is DevSELL::bytes() of the shared layout: 8 B per stored value, 2 B per stored
delta, 64 B of classes and 8 B of dptr per slice (+ 8), and the plain layout's other terms.
``lane_columns`` walks a delta stream the way k_d16_spmv does, through either addressing.

``CASES`` is the table of the CPU test (tests/test_d16_share_restatement.py, which pins the C
values every case is there for) and of the device tests (tests/test_gpu_d16_share.py).
"""
import functools
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import spmv_layout_cases as LC
import spmv_layout_restatement as R

LANES = np.arange(64)


@dataclass
class Shared:
    C: np.ndarray        # classes per slice
    cls: np.ndarray      # uint8, slices * 64
    dptr: np.ndarray     # slices + 1, in deltas
    dls: np.ndarray      # uint16, the shared stream
    bytes: int           # DevSELL::bytes() with the shared stream
    bytes_low: int       # ... of a product over the fp32 value stream

    @property
    def dstored(self):
        return int(self.dptr[-1])

    @property
    def shared_slices(self):
        return int((self.C < 64).sum())


def _lane_streams(E):
    """{L: (slices with that length, their delta streams as (slices, 64, L))} from the plain stream."""
    L = np.diff(E.sptr) // 64
    out = {}
    for Lv in np.unique(L):
        S = np.nonzero(L == Lv)[0]
        k = np.arange(int(Lv))
        where = E.sptr[S][:, None, None] + (k >> 3)[None, None, :] * 512 + LANES[None, :, None] * 8 + (k & 7)
        out[int(Lv)] = (S, E.dl[where])
    return out


def share(L, E):
    """The shared layout of a D16 layout L with plain streams E = L.encode()."""
    assert L.d16 and E.kind == "d16"
    ns = L.nslices
    cls = np.zeros(ns * 64, dtype=np.uint8)
    C = np.zeros(ns, dtype=np.int64)
    streams = _lane_streams(E)
    for Lv, (S, d) in streams.items():
        if Lv == 0:  # nothing stored: every lane has the empty stream
            C[S] = 1
            continue
        # one key per (slice, stream): the slice number in front keeps equal streams of two slices apart
        rows = np.concatenate((np.repeat(S, 64)[:, None], d.reshape(len(S) * 64, Lv).astype(np.int64)), axis=1)
        _, first, inv = np.unique(rows, axis=0, return_index=True, return_inverse=True)
        rep = first[inv.reshape(-1)]                       # the lowest lane with the same stream (flat index)
        is_rep = rep == np.arange(len(rep))
        ids = np.cumsum(is_rep.reshape(len(S), 64), axis=1) - 1   # class ids in order of the lowest member lane
        c = ids.reshape(-1)[rep].reshape(len(S), 64)
        cls[(S[:, None] * 64 + LANES).reshape(-1)] = c.reshape(-1)
        C[S] = is_rep.reshape(len(S), 64).sum(axis=1)
    Ls = np.diff(E.sptr) // 64
    dptr = np.concatenate(([0], np.cumsum(C * Ls))).astype(np.int64)
    dls = np.zeros(max(int(dptr[-1]), 8), dtype=np.uint16)
    for Lv, (S, d) in streams.items():
        if Lv == 0:
            continue
        k = np.arange(Lv)
        c = cls[S[:, None] * 64 + LANES].astype(np.int64)
        where = dptr[S][:, None, None] + ((k >> 3)[None, None, :] * C[S][:, None, None] + c[:, :, None]) * 8 + (k & 7)
        dls[where] = d  # the members of a class write the same values
    nbytes = L.bytes() - 2 * L.stored + 2 * int(dptr[-1]) + ns * 72 + 8
    return Shared(C, cls, dptr, dls, nbytes, nbytes - 4 * L.stored)


def lane_columns(E, shared=None):
    """The column every stored entry decodes to, {L: (slices, columns (slices, 64, L))}: the walk of
    k_d16_spmv over the plain stream, or (shared) over the shared one through dptr / cls."""
    Ls = np.diff(E.sptr) // 64
    out = {}
    for Lv in np.unique(Ls):
        S = np.nonzero(Ls == Lv)[0]
        slot = S[:, None] * 64 + LANES
        col = np.zeros((len(S), 64), dtype=np.int64)
        si = np.zeros((len(S), 64), dtype=np.int64)
        cols = np.zeros((len(S), 64, int(Lv)), dtype=np.int64)
        for k in range(int(Lv)):
            if shared is None:
                d = E.dl[E.sptr[S][:, None] + (k >> 3) * 512 + LANES * 8 + (k & 7)]
            else:
                c = shared.cls[slot].astype(np.int64)
                d = shared.dls[shared.dptr[S][:, None] + ((k >> 3) * shared.C[S][:, None] + c) * 8 + (k & 7)]
            d = d.astype(np.int64)
            zero = d == 0
            col = np.where(zero, E.seg[slot, np.minimum(si, E.nsegs - 1)], col + d)
            si = si + zero
            cols[:, :, k] = col
        out[int(Lv)] = (S, cols)
    return out


# --------------------------------------------------------------------- cases --
def _rows(n, cols_of_row):
    rows = np.concatenate([np.full(len(c), r) for r, c in enumerate(cols_of_row)])
    return LC._pattern(n, rows, np.concatenate(cols_of_row))


def classes_320():
    """Five 64-row slices that reach C = 2, 3, 22, 63 and 64 in turn.  Every row holds three
    entries: a start column, a gap of 1 + (the row's class number), a gap of 1.  (200 rows hold
    only four slices of 64 rows, so this is the smallest matrix with the five.)"""
    n = 320
    out = []
    for r in range(n):
        s, i = r // 64, r % 64
        kind = (i % 2, i % 3, i // 3, min(i, 62), i)[s]
        start = r % 200
        out.append(np.array([start, start + 1 + kind, start + 2 + kind]))
    return _rows(n, out)


def short_last_slice():
    """n = 100, tridiagonal with row 70 a single entry: the second slice holds 36 rows, and its 28
    lanes without a row share the all-zero class with the single-entry row."""
    n = 100
    out = [np.array([c for c in (r - 1, r, r + 1) if 0 <= c < n]) for r in range(n)]
    out[70] = np.array([70])
    return _rows(n, out)


def padded_twins():
    """n = 64: even rows hold columns c, c + 1, c + 2, odd rows c, c + 1.  The odd rows' deltas are
    the even rows' first ones, but their padding starts one entry earlier, so the streams differ."""
    n = 64
    return _rows(n, [np.arange(r % 32, r % 32 + (3 if r % 2 == 0 else 2)) for r in range(n)])


def distinct_64():
    """n = 64, row i holds columns 0, a, a + b with a = 1 + i % 8, b = 1 + i / 8: 64 different
    streams, so the shared layout saves no delta and costs the classes and dptr -- the case the
    auto rule declines.  (A diagonal matrix does not show it: all its streams are zero, C = 1, and
    sharing saves 1008 of every 1024 delta bytes.)"""
    return _rows(64, [np.array([0, 1 + i % 8, 2 + i % 8 + i // 8]) for i in range(64)])


@functools.lru_cache(maxsize=2)
def synthetic_2d(N=24):
    """The 2-D synthetic system in field-major order: (A, is_s, is_f, is_p)."""
    from oracle import synthetic as S
    spec = S.SynthSpec(2, N)
    return (S.matrix(spec, 0),) + tuple(np.asarray(i, dtype=np.int32) for i in S.field_major_index_sets(spec))


@dataclass(frozen=True)
class Case:
    id: str
    source: tuple                  # ("own", function name) or ("layout", id of a case of spmv_layout_cases)
    opts: tuple = ()
    expect_C: tuple = ()           # C of every slice in order; () where the CPU test states it otherwise
    single: bool = False           # also run the fp32 value stream over the shared deltas

    @property
    def options(self):
        return dict(self.opts)


CASES = [
    Case("synthetic-2d-24", ("own", "synthetic_2d"), single=True),
    Case("classes-320", ("own", "classes_320"), expect_C=(2, 3, 22, 63, 64), single=True),
    Case("short-last-slice", ("own", "short_last_slice"), expect_C=(2, 3)),
    Case("padded-twins", ("own", "padded_twins"), expect_C=(2,)),
    Case("wide", ("layout", "wide-1100-lpr8"), single=True),
    Case("sorted", ("layout", "sigma-lpr2"), single=True),
    Case("bases-8", ("layout", "segments-5")),
    Case("ramp", ("layout", "ramp")),
]
BY_ID = {c.id: c for c in CASES}


def system(case, kind="int"):
    """(A, x, is_s, is_f, is_p, options) of a case; values as spmv_layout_cases.matrix gives them."""
    if case.source[0] == "layout":
        lc = LC.BY_ID[case.source[1]]
        A, x = LC.matrix(lc, kind)
        is_s, is_f, is_p, _ = LC.index_sets(lc, A.shape[0])
        return A, x, is_s, is_f, is_p, dict(lc.options, **case.options)
    made = globals()[case.source[1]]()
    if isinstance(made, tuple):
        A, is_s, is_f, is_p = made
    else:
        A = made
        is_s, is_f, is_p, _ = LC.index_sets(LC.Case(case.id, ()), A.shape[0])
    A = sp.csr_matrix(A).copy()
    A.sort_indices()
    rng = np.random.default_rng(len(case.id) + (0 if kind == "int" else 1000))
    if kind == "int":
        A.data[:] = rng.integers(1, 9, A.nnz) * rng.choice((-1.0, 1.0), A.nnz)
        x = rng.integers(-16, 17, A.shape[0]).astype(np.float64)
    else:
        A.data[:] = rng.standard_normal(A.nnz)
        x = rng.standard_normal(A.shape[0])
    return A, x, is_s, is_f, is_p, case.options


_restated = {}


def restated(case):
    """(layout, plain streams, shared layout) of a case in the internal row order, computed once."""
    if case.id not in _restated:
        A, _, is_s, is_f, is_p, opts = system(case)
        perm = np.concatenate((is_s, np.sort(np.concatenate((is_f, is_p))))).astype(np.int64)
        L = R.layout(LC.internal(A, perm), opts)
        E = L.encode()
        _restated[case.id] = (L, E, share(L, E))
    return _restated[case.id]
