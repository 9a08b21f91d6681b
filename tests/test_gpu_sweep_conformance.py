"""The ten ILU(0) sweep kernels on the adversarial patterns of tests/sweep_cases.py.

For every case and every forced option set the case lists (its preconditions are pinned on the CPU
by tests/test_sweep_cases.py) the block PC of block_diag(K, I_32, I_32) is applied through
Handle.from_csr / pc_apply -- a handle holds one matrix, so the exact and the "normal" K get a handle
each, one after the other, and each handle applies twice:

1. the solid block's ``[pls ilu]`` line reports the kind the case lists for the run (fall-backs
   included), its type and block count, and for the window kinds the records per wave;
2. exact data: the six level kinds run the "int" data and return y* bit for bit (every partial sum is
   exact in any order).  The four kinds with explicit window inverses run the "unit" data (integer
   inverses of the "int" windows pass 2^53, on the CPU restatement too; the "unit" windows' do not) and
   are held to max |y - y*| <= 1e-12 max |y*|, finite;
3. "normal" data against the np.longdouble reference: level kinds <= 1e-13 max |y_ref|, inverse kinds
   <= 1e-12 max |y_ref| (the bars of tests/test_gpu_sweeps.py);
4. the second apply on either handle equals the first bitwise (scratch, ring and epoch reuse);
5. the fp block (the identity) returns x_fp bit for bit.

Then the equalities the code claims (window-ring == window, pls.window_kpw 8 == the chosen records,
pls.window_depth 2 == 3), and the factorization paths (pls.ilu_factor_dep, pls.ilu_dep_grid,
pls.ilu0_stage) under the LDS sweep on the "int" data, bit for bit.  The lanes per row of the LDS sweep
do not show in any sum (a lane's entries beyond its 7 prefetched ones are reloaded in the level), so the
stream layout that pls.ilu_view 2 prints is compared with its restatement (sweep_cases.lds_layout).
"""
import re

import numpy as np
import pytest

import sweep_cases as C

pytestmark = pytest.mark.gpu

LINE = re.compile(r"\[pls ilu\] type (\S+) n (\d+) blocks (\d+) max_len \d+ levels \d+/\d+ sweep (\S+)"
                  r"(?: \(records (\d)/(\d)\))?")
LAYOUT = re.compile(r"\[pls ilu lds ([LU])\] blocks (\d+): max levels (\d+), max slices per level (\d+), inline slices "
                    r"\(beyond 16 waves\) max (\d+) \(block (\d+)\), slices with > (\d+) entries per lane max (\d+)")
_applied = {}


def _apply(capfd, case, kind, opts, xs):
    """One handle on the case's `kind` K: the solid block's [pls ilu] line and pc_apply of every x."""
    from lib.handle import Handle, params_to_options
    d = C.data(case, kind)
    A, is_s, is_f, is_p = C.system(d.K)
    db = C.options(case, opts)
    db.update(params_to_options(C.PARAMS))
    capfd.readouterr()
    h = Handle.from_csr(A, A, None, is_s, is_f, is_p, [], db)
    try:
        ys = [h.pc_apply(x) for x in xs]
    finally:
        h.destroy()
    err = capfd.readouterr().err
    lines = [LINE.match(ln) for ln in err.splitlines() if ln.startswith("[pls ilu]")]
    mine = [m.groups() for m in lines if m and int(m.group(2)) == case.n]
    assert len(mine) == 1, lines
    return mine[0], ys, err


def exact_kind(case, run):
    """The exact data set a run is held to: "int" for the level kinds, "unit" for the inverse kinds."""
    return "int" if case.runs[run] in C.LEVEL_KINDS else "unit"


def applied(capfd, case, run):
    """(line, the two y of the exact data, the two y of the normal data) of a (case, run), computed once."""
    key = (case.id, run)
    if key not in _applied:
        exact = C.data(case, exact_kind(case, run))
        line, ye, _ = _apply(capfd, case, exact_kind(case, run), C.RUNS[run], [exact.x] * 2)
        line2, yn, _ = _apply(capfd, case, "normal", C.RUNS[run], [C.data(case, "normal").x] * 2)
        assert line2 == line
        _applied[key] = (line, ye, yn)
    return _applied[key]


def _check_exact(tag, case, kind, y, bitwise):
    """y against y* of the case's `kind` data: bit for bit, or (inverse kinds) within 1e-12 max |y*|."""
    d = C.data(case, kind)
    n = case.n
    wrong = np.nonzero(y[:n] != d.y)[0]
    with np.errstate(invalid="ignore"):
        ratio = float(np.abs(y[:n] - d.y).max()) / float(np.abs(d.y).max())
    print(f"{tag} {kind}: rows wrong {len(wrong)}, max |y - y*| / max |y*| = {ratio:.2e}"
          + (f" (first {wrong[:5]}: {y[wrong[:5]]} for {d.y[wrong[:5]]})" if len(wrong) else ""))
    assert np.array_equal(y[n:], d.x[n:])
    if bitwise:
        assert np.array_equal(y[:n], d.y)
    else:
        assert np.all(np.isfinite(y)) and ratio <= 1e-12


RUN_PARAMS = [pytest.param(c, r, id=f"{c.id}-{r}") for c in C.CASES for r in c.runs]


@pytest.mark.parametrize("case,run", RUN_PARAMS)
def test_sweep_kind_and_apply(gpu, capfd, case, run):
    kind = case.runs[run]
    (typ, _, blocks, got, ra, rb), (ye, ye2), (y1, y2) = applied(capfd, case, run)
    tag = f"{case.id} {run} [{got}]"
    assert got == kind
    assert typ == ("bjacobi" if case.blocks > 1 else "ilu") and int(blocks) == case.blocks
    if kind in ("window", "window-ring", "levels+window-ring"):
        want = (8, 8) if "pls.window_kpw" in C.RUNS[run] else case.records
        assert (int(ra), int(rb)) == want
    else:
        assert ra is None
    _check_exact(tag, case, exact_kind(case, run), ye, kind in C.LEVEL_KINDS)
    assert np.array_equal(ye2, ye)
    d = C.data(case, "normal")
    n = case.n
    scale = float(np.abs(d.y).max())
    ratio = float(np.abs(y1[:n].astype(np.longdouble) - d.y).max()) / scale
    print(f"{tag} normal: max |y - y_ref| / max |y_ref| = {ratio:.2e}")
    assert np.all(np.isfinite(y1))
    assert ratio <= (1e-13 if kind in C.LEVEL_KINDS else 1e-12)
    assert np.array_equal(y1[n:], d.x[n:])
    assert np.array_equal(y2, y1)


@pytest.mark.parametrize("name", C.EQUALITY_CASES)
def test_window_variants_give_the_same_bits(gpu, capfd, name):
    """The ring variant loads the same sums in the same order as the LDS window sweep, 8 records per wave
    the same as 4 or 6, and 3 windows of data in flight the same as 2: bitwise equal on the rounded and
    on the "unit" data."""
    case = C.BY_ID[name]
    runs = ("window", "window-ring", "window-kpw8", "window-ring-kpw8", "window-depth2", "window-depth3")
    got = {r: applied(capfd, case, r) for r in runs}
    assert [got[r][0][3] for r in runs] == ["window", "window-ring", "window", "window-ring", "window", "window"]
    assert got["window-kpw8"][0][4:] == ("8", "8") and got["window"][0][4:] == tuple(str(k) for k in case.records)
    for r in runs[1:]:
        for k in (0, 1):
            assert np.array_equal(got[r][1][k], got["window"][1][k]), r
            assert np.array_equal(got[r][2][k], got["window"][2][k]), r


@pytest.mark.parametrize("name", C.FACTOR_CASES)
@pytest.mark.parametrize("path", list(C.FACTOR_RUNS))
def test_factorization_paths_are_exact(gpu, capfd, name, path):
    """The one-launch dependency-driven factorization (pls.ilu_factor_dep 2; one workgroup:
    pls.ilu_dep_grid 1), the launch per level (0) and the staged-entry caps (pls.ilu0_stage 0, 64): the
    factors of the "int" K are exact on every path, so the LDS sweep returns y* bit for bit."""
    case = C.BY_ID[name]
    line, (y,), _ = _apply(capfd, case, "int", dict(C.RUNS["lds"], **C.FACTOR_RUNS[path]), [C.data(case, "int").x])
    assert line[3] == "lds"
    _check_exact(f"{case.id} {path} [lds]", case, "int", y, True)


@pytest.mark.parametrize("name,run", C.LAYOUT_RUNS)
def test_lds_stream_layout_as_restated(gpu, capfd, name, run):
    """The LDS sweep's streams per triangle -- levels, slices per level, slices beyond the 16 waves,
    slices whose lanes hold more than the 7 prefetched entries -- as build_lds_tri prints them under
    pls.ilu_view 2, against the restatement: 1, 2 and 4 lanes per row, chosen and forced, on rows of
    0 to 225 entries (lanes), one 400-entry row (arrow), levels of 21 to 82 slices (twolevel,
    diag-4100) and 70 blocks."""
    case = C.BY_ID[name]
    opts = dict(C.RUNS[run], **{"pls.ilu_view": "2"})
    line, (y,), err = _apply(capfd, case, "int", opts, [C.data(case, "int").x])
    assert line[3] == "lds"
    _check_exact(f"{case.id} {run} [lds]", case, "int", y, True)
    printed = {tri: set() for tri in "LU"}
    for m in LAYOUT.finditer(err):
        printed[m.group(1)].add(tuple(int(v) for v in m.groups()[1:]))
    for tri in "LU":
        want, lprs = C.lds_layout(case, tri == "U", int(C.RUNS[run].get("pls.sweep_lpr", 0)))
        print(f"{case.id} {run} {tri}: restated {want}, lanes per row {sorted(set(lprs))}, printed {sorted(printed[tri])}")
        assert want in printed[tri]
