"""The exact-LU family -- band / SPIKE (csrc/band.hip), the dense Gauss-Jordan inverse with threshold
pivoting (csrc/dense.hip), the envelope path and the multifrontal path of make_lu -- on the edge shapes
of tests/lu_cases.py (their preconditions are pinned on the CPU by tests/test_lu_cases.py).

The block PC of block_diag(K, I_32, I_32) is applied through Handle.from_csr / pc_apply with
pls.lu_path forced -- a handle holds one matrix, so the exact and the "normal" K get a handle each:

1. the path's view line reports what the table names: ``[band lu]`` tile rows, bl, bu, SPIKE partition
   length and partition count for every pls.band_spike_plen the case lists; ``[dense lu]`` the rows
   exchanged (the restated pivot rule's count), no pivot below the threshold, no zero column;
   ``[pls ilu] type lu`` one block for the envelope path; ``[sparse lu]`` the fronts, levels and largest
   front of lib.handle.sparse_lu_analyze and no delayed pivot;
2. exact data ("int", the swap cases "swap"): the band path (every run), the dense path and the
   envelope path (which eliminates in natural order on the profile pattern) return y* bit for bit;
3. one handle applies x, then -2 x + e (e another integer vector), then x again: each result is its
   own solution bit for bit and the third equals the first -- a consumer that accepted a granule of an
   earlier sweep's epoch, or scratch that kept a previous right-hand side, would not;
4. "normal" data against the np.longdouble reference: every path, the multifrontal one (dissection
   order: rounded only) included, within 1e-12 max |y_ref|, finite (the bar of
   tests/test_gpu_sparse_lu.py); a second apply equals the first bitwise (the sums run in a fixed order);
5. the fp block (the identity) returns x_fp bit for bit.

Runs of one case with different partition lengths are not compared with each other on the rounded
data: SPIKE reorders the sums.
"""
import re
import sys

import numpy as np
import pytest

import lu_cases as C

pytestmark = pytest.mark.gpu

BAND_LINE = re.compile(r"\[band lu\] n (\d+): tile rows (\d+), bl (\d+), bu (\d+), spike plen (\d+), partitions (\d+)$")
DENSE_LINE = re.compile(r"\[dense lu\] n (\d+): threshold pivoting u = (\S+): (\d+) rows exchanged, (\d+) pivots below "
                        r"u x column max \(delayed by MUMPS\), (\d+) zero columns$")
SPARSE_LINE = re.compile(r"\[sparse lu\] n (\d+): (\d+) fronts, (\d+) levels, largest front (\d+), .*; (\d+) delayed "
                         r"pivots \((\d+) re-analyses\)")
ILU_LINE = re.compile(r"\[pls ilu\] type (\S+) n (\d+) blocks (\d+) ")


def _apply(capfd, K, xs, db):
    """One handle on block_diag(K, I_32, I_32): stderr of its setup and applies, and pc_apply of every x."""
    from lib.handle import Handle, params_to_options
    A, is_s, is_f, is_p = C.system(K)
    db = dict(db)
    db.update(params_to_options(C.PARAMS))
    before = capfd.readouterr()
    h = Handle.from_csr(A, A, None, is_s, is_f, is_p, [], db)
    try:
        ys = [h.pc_apply(x) for x in xs]
    finally:
        h.destroy()
    got = capfd.readouterr()
    sys.stdout.write(before.out + got.out)  # (the figures printed so far stay in the test's output)
    return got.err, ys


def _view(err, regex, n):
    """The groups of the one view line of the n-row block, as integers where they are."""
    got = [m.groups() for m in (regex.match(ln) for ln in err.splitlines()) if m and int(m.group(1)) == n]
    assert len(got) == 1, err
    return tuple(int(v) if v.isdigit() else v for v in got[0])


def _exact(capfd, case, db, tag):
    """Items 2, 3 and 5 on the case's exact data; returns stderr."""
    d = C.data(case, C.exact_kind(case))
    n = case.n
    x2, y2_want = C.second_rhs(case)
    err, (y1, y2, y3) = _apply(capfd, d.K, [d.x, x2, d.x], db)
    for name, y, want in (("x", y1, d.y), ("-2 x + e", y2, y2_want), ("x again", y3, d.y)):
        wrong = np.nonzero(y[:n] != want)[0]
        with np.errstate(invalid="ignore"):
            dev = float(np.abs(y[:n] - want).max())
        print(f"{tag} {C.exact_kind(case)} [{name}]: rows wrong {len(wrong)}, max |y - y*| = {dev:.2e}"
              + (f" (first {wrong[:5]}: {y[wrong[:5]]} for {want[wrong[:5]]})" if len(wrong) else ""))
    assert np.array_equal(y1[:n], d.y)
    assert np.array_equal(y2[:n], y2_want)
    assert np.array_equal(y3, y1)
    assert np.array_equal(y1[n:], d.x[n:]) and np.array_equal(y2[n:], x2[n:])
    return err


def _rounded(capfd, case, db, tag):
    """Items 4 and 5 on the case's "normal" data; returns stderr."""
    d = C.data(case, "normal")
    n = case.n
    err, (y1, y2) = _apply(capfd, d.K, [d.x, d.x], db)
    scale = float(np.abs(d.y).max())
    with np.errstate(invalid="ignore"):
        ratio = float(np.abs(y1[:n].astype(np.longdouble) - d.y).max()) / scale
    print(f"{tag} normal: max |y - y_ref| / max |y_ref| = {ratio:.2e}")
    assert np.all(np.isfinite(y1))
    assert ratio <= 1e-12
    assert np.array_equal(y1[n:], d.x[n:])
    assert np.array_equal(y2, y1)
    return err


BAND_RUNS = [pytest.param(c, r, id=f"{c.id}-plen-{r}") for c in C.BAND_CASES for r in c.runs]


@pytest.mark.parametrize("case,run", BAND_RUNS)
def test_band_path(gpu, capfd, case, run):
    plen, parts = case.runs[run]
    db = C.options("band", run=run)
    want = (case.n,) + case.geometry + (plen, len(parts))
    tag = f"{case.id} plen {run} [band]"
    assert _view(_exact(capfd, case, db, tag), BAND_LINE, case.n) == want
    assert _view(_rounded(capfd, case, db, tag), BAND_LINE, case.n) == want


def _dense_line(err, case, exchanged, threshold=None):
    u = threshold if threshold is not None else f"{C.PIVOT_U:g}"
    assert _view(err, DENSE_LINE, case.n) == (case.n, int(u) if u.isdigit() else u, exchanged, 0, 0)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in C.DENSE_CASES])
def test_dense_path(gpu, capfd, case):
    """n = 1 (no pivot buffers), 2, 63, 64, 65, odd n (the gemv's tail column), the fast panel path
    ("int": nothing exchanged), pls.lu_pivot_threshold 0, and the one-workgroup panel_pivot on the
    "swap" data: an exchange inside a tile, into a later tile, into the last partial tile, two in a tile."""
    db = C.options("dense", threshold=case.threshold)
    tag = f"{case.id} [dense]"
    _dense_line(_exact(capfd, case, db, tag), case, len(case.swaps), case.threshold)
    if not case.swaps:
        _dense_line(_rounded(capfd, case, db, tag), case, 0, case.threshold)


BAND = [pytest.param(c, id=c.id) for c in C.BAND_CASES]


@pytest.mark.parametrize("case", BAND)
def test_band_cases_on_the_dense_path(gpu, capfd, case):
    db = C.options("dense")
    tag = f"{case.id} [dense]"
    _dense_line(_exact(capfd, case, db, tag), case, 0)
    _dense_line(_rounded(capfd, case, db, tag), case, 0)


@pytest.mark.parametrize("case", BAND)
def test_band_cases_on_the_envelope_path(gpu, capfd, case):
    db = C.options("envelope")
    tag = f"{case.id} [envelope]"
    for err in (_exact(capfd, case, db, tag), _rounded(capfd, case, db, tag)):
        lines = [m.groups() for m in (ILU_LINE.match(ln) for ln in err.splitlines()) if m and m.group(1) == "lu"]
        assert lines == [("lu", str(case.n), "1")], err


@pytest.mark.parametrize("leaf", C.ND_LEAVES)
@pytest.mark.parametrize("case", BAND)
def test_band_cases_on_the_sparse_path(gpu, capfd, case, leaf):
    """Dissection order: the pivots of the "int" K are not the dyadic ones of its natural order, so the
    multifrontal path runs the rounded data only.  Its fronts are those of sparse_lu_analyze."""
    from lib.handle import sparse_lu_analyze
    db = C.options("sparse", leaf=leaf)
    err = _rounded(capfd, case, db, f"{case.id} leaf {leaf} [sparse]")
    st = sparse_lu_analyze(C.data(case, "normal").K, {"pls.lu_nd_leaf": leaf})
    n, fronts, levels, largest, delayed, rounds = _view(err, SPARSE_LINE, case.n)
    assert (fronts, levels, largest) == (int(st["fronts"]), int(st["levels"]), int(st["max_front"]))
    assert (delayed, rounds) == (0, 0)
