"""ILU(k) on the device (<prefix>pc_factor_levels, <prefix>sub_pc_factor_levels; csrc/iluk.hip)
against the numpy restatement tests/iluk_restatement.py (pinned by tests/test_iluk_restatement.py).

Pattern: pls_get_ilu_fill's entries and longest row equal the restatement's exactly.  PC apply:
<= 1e-13 relative (max norm), the project's bar for a PC application.  Solves: iteration count
and reason exact, every history entry within max(1e-10, 10 x the restatement's own worst
deviation over 4 seeds when every inner PC output is perturbed by 1e-15 relative) -- the rule
of tests/test_gpu_ksp_types.py, whose _noise_floor is copied here.

Sizes: synthetic 2-D N = 6 (s block 338 rows, fp block 387) and 3-D N = 4 (2,187 and 2,312).  The oracle is built
from the options without the levels keys (it restates ILU(0) only) and gets the restated PCs
installed in place of its own.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from iluk_restatement import PCBJacobi, PCILUk
from oracle import synthetic as S
from oracle.solver import OracleSolver

pytestmark = pytest.mark.gpu

BASE = {"solver type": "gmres", "solver atol": 1e-8, "solver rtol": 1e-6, "solver maxiter": 300,
        "pc type": "diagonal", "inner ksp type": "preonly", "inner pc type": "ilu", "inner rtol": 1e-6,
        "inner atol": 0, "inner maxiter": 1000, "inner monitor": False, "solver monitor": False,
        "inner accel order": 0, "AAR order": 10, "AAR p": 5, "AAR omega": 1, "AAR beta": 1}
TWO, THREE = ("s_", "fp_"), ("s_", "f_", "p_", "diff_")
KSP_OF = {"s_": "ksp_s", "fp_": "ksp_fp", "f_": "ksp_f", "p_": "ksp_p", "diff_": "ksp_p_diff"}
INNER = ("ksp_s", "ksp_fp", "ksp_f", "ksp_p")
SPECS = {"2d6": S.SynthSpec(2, 6), "3d4": S.SynthSpec(3, 4)}
NB = 3  # bjacobi blocks


def _db(prefixes, pc, levels=None, extra=None):
    """preonly + ilu / bjacobi (3 blocks) on every prefix; levels: the levels-of-fill keys too."""
    db = {"global_ksp_type": "gmres", "global_ksp_pc_side": "right"}
    for pre in prefixes:
        db[pre + "ksp_type"] = "preonly"
        db[pre + "pc_type"] = pc
        if pc == "bjacobi":
            db[pre + "pc_bjacobi_blocks"] = str(NB)
        if levels is not None:
            db[pre + ("sub_pc_factor_levels" if pc == "bjacobi" else "pc_factor_levels")] = str(levels)
    db.update(extra or {})
    return db


def _handle(spec, params, db):
    from lib.handle import Handle, params_to_options
    opts = dict(db)
    opts.update(params_to_options(params))
    return Handle.synthetic(spec.dim, spec.N, spec.seed, spec.delta, opts)


_restated = {}


def _restate(key, M, pc, k):
    """The restated PC of a block, computed once per (system, prefix, pc, k) and left unchanged."""
    key = key + (pc, k)
    if key not in _restated:
        # 3-D blocks (2,187 and 2,312 rows of hundreds of entries): the restatement's fast path,
        # pinned equal to the plain one by tests/test_iluk_restatement.py
        fast = key[0] == "3d4"
        _restated[key] = PCILUk(M, k, fast) if pc == "ilu" else PCBJacobi(M, NB, k, fast)
    return _restated[key]


def _oracle(name, params, prefixes, pc, k, system=None):
    """The oracle on the db without the levels keys, the restated ILU(k) PCs installed."""
    spec = SPECS[name]
    if system is None:
        A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    else:
        A, P, Pd = system
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    o = OracleSolver(A, P, Pd, is_s, is_f, is_p, params, _db(prefixes, pc), S.bcs_sub_pressure(spec))
    for pre in prefixes:
        ksp = getattr(o.block_pc, KSP_OF[pre])
        ksp.pc = _restate((name, system is not None, pre), ksp.A, pc, k)
    return o


def _noise_floor(o, b, ho, its, eps=1e-15, seeds=4):
    """Worst relative deviation of the restatement's own history over the seeds
    (every inner PC output perturbed by eps relative); its count must not move."""
    worst = 0.0
    for seed in range(seeds):
        rng = np.random.default_rng(seed)
        saved = []
        for name in INNER:
            ksp = getattr(o.block_pc, name, None)
            if ksp is None:
                continue
            orig = ksp.pc.apply
            saved.append((ksp.pc, orig))
            ksp.pc.apply = (lambda f: lambda x: (lambda y: y * (1 + eps * rng.standard_normal(y.size)))(f(x)))(orig)
        o.solve(b)
        for pc, orig in saved:
            pc.apply = orig
        assert o.its == its, f"bad input: the restatement takes {o.its} iterations with seed {seed}, {its} without"
        h2 = np.asarray(o.history)
        worst = max(worst, float(np.max(np.abs(h2 - ho) / np.abs(ho))))
    return worst


def _rel(y, yo):
    return float(np.max(np.abs(y - yo)) / np.max(np.abs(yo)))


# ------------------------------------------------------ pattern and fill ----
@pytest.mark.parametrize("pc", ["ilu", "bjacobi"])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("name", list(SPECS))
def test_pattern_and_fill(gpu, name, k, pc):
    o = _oracle(name, BASE, TWO, pc, k)
    h = _handle(SPECS[name], BASE, _db(TWO, pc, k))
    h.setup()
    for pre in TWO:
        ksp = getattr(o.block_pc, KSP_OF[pre])
        M = sp.csr_matrix(ksp.A)
        if pc == "bjacobi":  # entries of the truncated block
            nnz0 = sum(M[lo:hi, lo:hi].nnz for lo, hi in zip(ksp.pc.bounds[:-1], ksp.pc.bounds[1:]))
        else:
            nnz0 = M.nnz
        got = h.ilu_fill(pre)
        print(pre, "levels, nnz before, after, longest row:", got, "restatement", (nnz0, ksp.pc.nnz, ksp.pc.max_row))
        assert got == (k, nnz0, ksp.pc.nnz, ksp.pc.max_row)
        assert got[2] > got[1]
    h.destroy()


def test_fill_of_the_2d_blocks_as_measured(gpu):
    """2-D N = 6, levels 1: fill 2.96 on s, 3.48 on fp; longest rows 69 and 176."""
    h = _handle(SPECS["2d6"], BASE, _db(TWO, "ilu", 1))
    h.setup()
    s, fp = h.ilu_fill("s_"), h.ilu_fill("fp_")
    assert (round(s[2] / s[1], 2), s[3]) == (2.96, 69) and (round(fp[2] / fp[1], 2), fp[3]) == (3.48, 176)
    h.destroy()


def test_ilu_fill_refuses_other_pcs(gpu):
    h = _handle(SPECS["2d6"], BASE, dict(_db(TWO, "ilu", 1), fp_pc_type="jacobi"))
    h.setup()
    with pytest.raises(RuntimeError, match="pls_get_ilu_fill.*fp_.*jacobi"):
        h.ilu_fill("fp_")
    with pytest.raises(RuntimeError, match="pls_get_ilu_fill.*no inner solver.*nope_"):
        h.ilu_fill("nope_")
    assert h.ilu_fill("s_")[0] == 1
    h.destroy()


# -------------------------------------------------------------- PC apply ----
@pytest.mark.parametrize("name,pc", [("2d6", "ilu"), ("2d6", "bjacobi"), ("3d4", "ilu")])
def test_pc_apply(gpu, name, pc):
    o = _oracle(name, BASE, TWO, pc, 1)
    h = _handle(SPECS[name], BASE, _db(TWO, pc, 1))
    x = np.random.default_rng(5).standard_normal(SPECS[name].n)
    y, yo = h.pc_apply(x), o.block_pc.apply(x)
    print(f"PC apply rel diff {_rel(y, yo):.3e}")
    assert _rel(y, yo) <= 1e-13
    # and it is not the ILU(0) application
    y0 = _handle(SPECS[name], BASE, _db(TWO, pc)).pc_apply(x)
    assert _rel(y0, yo) > 1e-6
    h.destroy()


@pytest.mark.parametrize("forced", [{}, {"pls.ilu_gmem": "1"}], ids=["default", "ilu_gmem"])
def test_pc_apply_forced_sweeps(gpu, capfd, forced):
    """Filled rows are longer (69 and 176 entries against 23 and 42): other lanes per row in the
    LDS sweep, and in the y-resident workgroup sweep that pls.ilu_gmem 1 forces."""
    o = _oracle("2d6", BASE, TWO, "ilu", 1)
    capfd.readouterr()
    h = _handle(SPECS["2d6"], BASE, _db(TWO, "ilu", 1, dict(forced, **{"pls.ilu_view": "1"})))
    x = np.random.default_rng(6).standard_normal(SPECS["2d6"].n)
    y, yo = h.pc_apply(x), o.block_pc.apply(x)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[pls ilu]")]
    print("\n".join(lines), f"\nPC apply rel diff {_rel(y, yo):.3e}")
    assert len(lines) == 2 and all(" levels 1 fill " in ln for ln in lines)
    kinds = {ln.split(" sweep ")[1].split(" ")[0] for ln in lines}
    if forced:  # the y-resident workgroup sweep (its ring variant where every level fits a chunk)
        assert kinds <= {"gmem", "ring"}, kinds
    else:       # blocks of a few hundred rows stay LDS-resident
        assert kinds <= {"lds", "chain", "window"}, kinds
    assert _rel(y, yo) <= 1e-13
    h.destroy()


# ---------------------------------------------------------------- solves ----
@pytest.mark.parametrize("name,pc_type,k", [("2d6", "diagonal", 1), ("2d6", "diagonal", 2),
                                            ("2d6", "diagonal 3-way", 1), ("2d6", "diagonal 3-way", 2),
                                            ("3d4", "diagonal", 1)])
def test_solve(gpu, name, pc_type, k):
    spec = SPECS[name]
    params = dict(BASE, **{"pc type": pc_type})
    prefixes = THREE if "3-way" in pc_type else TWO
    b = S.rhs(spec)
    o = _oracle(name, params, prefixes, "ilu", k)
    xo = o.solve(b)
    its, reason, ho = o.its, o.reason, np.asarray(o.history)
    tol = max(1e-10, 10 * _noise_floor(o, b, ho, its))
    h = _handle(spec, params, _db(prefixes, "ilu", k))
    x, r = h.solve(b)
    hist = h.history()
    print(f"its {r.its} (restatement {its}) reason {r.reason} ({reason}) history tol {tol:.2e}")
    assert r.its == its, f"its {r.its} vs restatement {its}"
    assert r.reason == reason, f"reason {r.reason} vs restatement {reason}"
    assert hist.shape == ho.shape
    rel = np.max(np.abs(hist - ho) / np.abs(ho))
    print(f"history rel diff {rel:.3e}; |x - x_o| / |x_o| {np.linalg.norm(x - xo) / np.linalg.norm(xo):.3e}")
    assert rel <= tol, f"residual history rel diff {rel:.3e} (tol {tol:.1e})"
    assert np.linalg.norm(x - xo) <= max(1e-8, tol) * np.linalg.norm(xo)
    h.destroy()


def test_the_level_is_observable(gpu):
    """2-D N = 6 "diagonal": 12 / 8 / 7 outer iterations at levels 0 / 1 / 2 (measured on the CPU
    restatement)."""
    spec = SPECS["2d6"]
    b = S.rhs(spec)
    its = []
    for k in (0, 1, 2):
        h = _handle(spec, BASE, _db(TWO, "ilu", k))
        its.append(h.solve(b)[1].its)
        h.destroy()
    assert its == [12, 8, 7]


def test_levels_0_is_untouched(gpu):
    """s_pc_factor_levels 0: the solve of the option being absent, bitwise."""
    spec = SPECS["2d6"]
    b = S.rhs(spec)
    out = []
    for k in (None, 0):
        h = _handle(spec, BASE, _db(TWO, "ilu", k))
        x, r = h.solve(b)
        out.append((x, h.history(), r.its, h.ilu_fill("s_")))
        h.destroy()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    assert out[0][3] == out[1][3] and out[0][3][0] == 0 and out[0][3][1] == out[0][3][2]


# --------------------------------------------- a nonsymmetric pattern ----
def _one_sided_system(spec, count=40, seed=9):
    """The synthetic matrices with `count` entries added to P's s block on one side of the
    diagonal only (where neither (i, j) nor (j, i) is stored)."""
    A, P, Pd = S.matrix(spec, 0), sp.lil_matrix(S.matrix(spec, 1)), S.matrix(spec, 2)
    is_s = np.asarray(S.field_major_index_sets(spec)[0])
    pat = sp.csr_matrix(S.matrix(spec, 1))
    rng = np.random.default_rng(seed)
    added = 0
    while added < count:
        i, j = (int(v) for v in rng.choice(is_s, 2, replace=False))
        if abs(i - j) > 40 or pat[i, j] != 0 or pat[j, i] != 0 or P[i, j] != 0 or P[j, i] != 0:
            continue
        P[i, j] = 1e-2 * rng.standard_normal()
        added += 1
    P = sp.csr_matrix(P)
    P.sort_indices()
    return A, P, Pd


def test_nonsymmetric_pattern(gpu):
    from lib.handle import Handle, params_to_options
    spec = SPECS["2d6"]
    system = _one_sided_system(spec)
    A, P, Pd = system
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    Ms = P[np.asarray(is_s)][:, np.asarray(is_s)]
    assert (Ms != 0).astype(int).T.tocsr().nnz == Ms.nnz and ((Ms != 0) != (Ms != 0).T).nnz == 2 * 40
    o = _oracle("2d6", BASE, TWO, "ilu", 1, system=system)
    opts = _db(TWO, "ilu", 1)
    opts.update(params_to_options(BASE))
    h = Handle.from_csr(A, P, Pd, is_s, is_f, is_p, S.bcs_sub_pressure(spec), opts)
    h.setup()
    pc = o.block_pc.ksp_s.pc
    sym = _oracle("2d6", BASE, TWO, "ilu", 1).block_pc.ksp_s.pc  # the symmetric block's
    got = h.ilu_fill("s_")
    print("s_", got, "restatement", (pc.nnz, pc.max_row), "symmetric pattern", sym.nnz)
    assert got == (1, Ms.nnz, pc.nnz, pc.max_row)
    assert pc.nnz > sym.nnz + 40  # the one-sided entries create fill of their own
    x = np.random.default_rng(7).standard_normal(spec.n)
    y, yo = h.pc_apply(x), o.block_pc.apply(x)
    print(f"PC apply rel diff {_rel(y, yo):.3e}")
    assert _rel(y, yo) <= 1e-13
    h.destroy()


# ------------------------------------------------------ the overflow path ----
def test_small_lds_table_goes_through_global_memory(gpu, capfd):
    """pls.iluk_lds_slots 256 holds 128 vertices per search; level-2 searches on both blocks visit
    more, so rows go through the global-memory launch -- with the identical pattern and apply.
    The default tables (16 x levels x longest row slots: 1,024 and 2,048 here) hold more vertices
    than the blocks have rows, so no search leaves LDS."""
    spec = SPECS["2d6"]
    x = np.random.default_rng(8).standard_normal(spec.n)
    res = []
    for slots in (None, "256"):
        capfd.readouterr()
        extra = {"pls.ilu_view": "1"}
        if slots:
            extra["pls.iluk_lds_slots"] = slots
        h = _handle(spec, BASE, _db(TWO, "ilu", 2, extra))
        y = h.pc_apply(x)
        lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[pls ilu]")]
        moved = [int(ln.split("rows through global memory ")[1].rstrip(")")) for ln in lines]
        res.append((h.ilu_fill("s_"), h.ilu_fill("fp_"), y, moved))
        h.destroy()
    print("rows through global memory:", res[0][3], res[1][3])
    assert res[0][3] == [0, 0] and max(res[1][3]) > 0
    assert res[0][:2] == res[1][:2] and np.array_equal(res[0][2], res[1][2])
    o = _oracle("2d6", BASE, TWO, "ilu", 2)
    assert res[1][1][2:] == (o.block_pc.ksp_fp.pc.nnz, o.block_pc.ksp_fp.pc.max_row)


# -------------------------------------------------------------- refusals ----
@pytest.mark.parametrize("key,pc,value", [("s_pc_factor_levels", "ilu", "-1"), ("s_pc_factor_levels", "ilu", "1.5"),
                                          ("fp_sub_pc_factor_levels", "bjacobi", "-2"),
                                          ("pls.iluk_lds_slots", "ilu", "100")])
def test_refusals_name_the_key(gpu, key, pc, value):
    with pytest.raises(RuntimeError, match=key.replace(".", r"\.")):
        h = _handle(SPECS["2d6"], BASE, dict(_db(TWO, pc, 1), **{key: value}))
        h.setup()
