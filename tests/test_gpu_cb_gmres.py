"""Compressed-basis GMRES on the device -- ``<prefix>pls_gmres_basis single``,
the Krylov basis of gmres / fgmres stored in fp32 -- against its numpy
restatement (tests/cb_gmres_restatement.py, pinned on the CPU by
tests/test_cb_gmres_restatement.py) installed in ``OracleSolver``.

Tolerances, the project's rule (tests/test_gpu_ksp_types.py): iteration count,
reason and history length exact; every history entry within max(1e-10, 10 x
the restatement's own worst deviation over 4 seeds when every inner PC output
is perturbed by 1e-15 relative); the solution within max(1e-8, that bound)
relative.  A rounding to fp32 can flip under a 1e-16 difference (about 1e-4
per case); a flip shows as a history difference near 1e-8 and is to be
reported, not tolerated.

Row counts and their residues mod 4 (the fp32 kernels take four rows per lane;
the tail rows are thread 0's): 2-D N=12 2,669 rows (1), 3-D N=4 4,499 (3), the
s block of 2-D N=32 3-way 8,450 (2; three reduction chunks of 2,820 rows, a
multiple of 4), its p block 1,089 (1).
"""
import numpy as np
import pytest

import cb_gmres_restatement as CB
import gmres_orthog_restatement as G
import test_gpu_ksp_types as K
from oracle import synthetic as S
from oracle.solver import OracleSolver

pytestmark = pytest.mark.gpu

SINGLE = {"global_pls_gmres_basis": "single"}


def _oracle(spec, params, db):
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    odb = {k: v for k, v in db.items() if "pls_gmres_basis" not in k}
    return A, OracleSolver(A, P, Pd, is_s, is_f, is_p, params, odb, S.bcs_sub_pressure(spec))


def _install(ksp, log=None, **kw):
    def solve(b):
        x = CB.gmres(ksp, b, **kw)
        if log is not None:
            log.append((ksp.its, ksp.cb_forced, ksp.cb_confirm, ksp.cb_failed, list(ksp.cb_ratios)))
        return x

    ksp.solve = solve


def _reference(spec, params, db, b=None, target="solver", name=None, **kw):
    """The CPU side: the oracle with the restatement on ``target`` ("solver":
    the outer KSP, else an attribute of the block PC under a restated outer
    fgmres with a double basis), its solution, counters and the tolerance."""
    b = S.rhs(spec) if b is None else b
    A, o = _oracle(spec, params, db)
    log = []
    if target == "solver":
        _install(o.solver, log, **kw)
    else:
        o.solver.solve = lambda bb: G.gmres(o.solver, bb, flexible=True)
        _install(getattr(o.block_pc, target), log, **kw)
    xo = o.solve(b)
    first = list(log)
    its, reason, ho = o.its, o.reason, np.asarray(o.history)
    floor = K._noise_floor(o, b, ho, its) if ho.size and np.all(ho > 0) else 0.0
    tol = max(1e-10, 10 * floor)
    if target == "solver":
        for e in log[1:]:
            assert e[:4] == log[0][:4], f"bad input: counters {e[:4]} with a seed, {log[0][:4]} without"
        if name:
            CB.check_ratios(name, log[0][4])
    print(f"restatement: its {its} reason {reason} entries {ho.size} floor {floor:.2e} tol {tol:.2e} "
          f"counters {first[0][:4] if first else None}")
    return {"A": A, "o": o, "b": b, "xo": xo, "its": its, "reason": reason, "ho": ho, "tol": tol, "first": first}


def _device(spec, params, db, ref):
    h = K._handle(spec, params, db)
    x, r = h.solve(ref["b"])
    hist = h.history()
    ho, xo, tol = ref["ho"], ref["xo"], ref["tol"]
    print(f"device: its {r.its} ({ref['its']}) reason {r.reason} ({ref['reason']}) entries {hist.size} ({ho.size})")
    assert r.its == ref["its"], f"its {r.its} vs restatement {ref['its']}"
    assert r.reason == ref["reason"], f"reason {r.reason} vs restatement {ref['reason']}"
    assert hist.shape == ho.shape
    rel = float(np.max(np.abs(hist - ho) / np.abs(ho))) if ho.size else 0.0
    xerr = np.linalg.norm(x - xo) / np.linalg.norm(xo)
    print(f"history rel diff {rel:.3e} (tol {tol:.2e}); |x - x_o| / |x_o| {xerr:.3e}")
    assert rel <= tol, f"residual history rel diff {rel:.3e} (tol {tol:.1e})"
    assert xerr <= max(1e-8, tol)
    return h, x, r, hist


def _outer_stats(h, ref, spec, restart):
    st = h.gmres_basis_stats("global_")
    print("gmres_basis_stats", st)
    assert st == (1, CB.basis_bytes(spec.n, restart, True)) + ref["first"][0][1:4]
    return st


def _double_history(spec, params, db, b):
    h = K._handle(spec, params, {k: v for k, v in db.items() if "pls_gmres_basis" not in k})
    x, r = h.solve(b)
    return h, x, r, h.history()


# ------------------------------------- 1. the table, CGS refine_never ----
@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", ["2d12_right", "2d12_left", "3d4_right", "2d12_right_restart5"])
def test_table_cases(gpu, name, rtol):
    """its / history entries / counters as recorded on the CPU; the basis takes
    half the bytes of double's up to the ldv rounding; the fp32 path ran (the
    history differs from double's by more than 1e-7 somewhere); the last entry
    is ||b - A x|| (right) from the device's own product."""
    dim, N, side, restart, n = G.TABLE[name][:5]
    spec = S.SynthSpec(dim, N)
    assert spec.n == n
    params = dict(G.PARAMS, **{"solver rtol": rtol})
    db = dict(G.table_db(name), **SINGLE)
    ref = _reference(spec, params, db, name=name)
    want = CB.RECORDED[name][rtol]
    assert (ref["its"], ref["ho"].size) + ref["first"][0][1:4] == want
    h, x, r, hist = _device(spec, params, db, ref)
    st = _outer_stats(h, ref, spec, restart)
    hd, _, rd, histd = _double_history(spec, params, db, ref["b"])
    std = hd.gmres_basis_stats("global_")
    assert std == (0, CB.basis_bytes(n, restart, False), 0, 0, 0)
    assert abs(2 * st[1] - std[1]) <= (restart + 1) * 128 * 4  # half, up to one 512-byte column rounding
    m = min(hist.size, histd.size)
    gap = float(np.max(np.abs(hist[:m] - histd[:m]) / histd[:m]))
    print(f"double: its {rd.its}, entries {histd.size}; |single - double| history {gap:.2e}")
    assert gap > 1e-7
    if side == "right":
        true = np.linalg.norm(ref["b"] - h.matmult(x))
        assert abs(hist[-1] - true) <= 1e-10 * true


# ------------------------------------------ 2. the other three schemes ----
@pytest.mark.parametrize("scheme", ["refine_ifneeded", "refine_always", "mgs"])
def test_schemes(gpu, scheme):
    spec = S.SynthSpec(2, 12)
    dbs, kw = G.SCHEMES[scheme]
    db = dict(G.table_db("2d12_right"), **SINGLE, **{"global_" + k: v for k, v in dbs.items()})
    ref = _reference(spec, G.PARAMS, db, **kw)
    h, _, r, _ = _device(spec, G.PARAMS, db, ref)
    _outer_stats(h, ref, spec, 400)
    ost = h.gmres_orthog_stats("global_")
    o = ref["o"].solver
    print("orthog stats", ost, "restatement", o.orthog_steps, o.second_passes)
    assert ost[0] == r.its and ost[2] == {"refine_ifneeded": 1, "refine_always": 2, "mgs": 3}[scheme]
    if scheme == "refine_always":
        assert ost[1] == r.its
    if scheme == "mgs":
        assert ost[1] == 0


# ----------------------------------------------------------- 3. fgmres ----
def test_fgmres_variable_inner_cg(gpu):
    """Outer fgmres over an inner CG at rtol 1e-1 (not a fixed operator): V in
    fp32, Z in fp64, no PC application in BuildSoln, and the last history entry
    is the true residual."""
    spec = S.SynthSpec(2, 12)
    db = dict(K.FGMRES_DB, s_ksp_type="cg", s_pc_type="jacobi", s_ksp_norm_type="unpreconditioned", s_ksp_rtol="1e-1",
              **SINGLE)
    ref = _reference(spec, K.BASE, db, flexible=True)
    h, x, r, hist = _device(spec, K.BASE, db, ref)
    _outer_stats(h, ref, spec, 300)
    assert r.pc_applies == r.its
    true = np.linalg.norm(ref["b"] - h.matmult(x))
    print(f"true residual {true:.6e}, last history entry {hist[-1]:.6e}")
    assert abs(hist[-1] - true) <= 1e-10 * true


# ------------------------- 4. inner prefix, more than one reduction chunk ----
def test_inner_s_gmres_8450_rows(gpu):
    """s_ksp_type gmres (left, Jacobi, rtol 1e-3) with the fp32 basis on the
    8,450-row s block of 2-D N=32 3-way under outer fgmres (double): three
    reduction chunks with starts on multiples of 4, n mod 4 = 2."""
    spec = S.SynthSpec(2, 32)
    params = dict(K.BASE, **{"pc type": "diagonal 3-way", "solver maxiter": 4})
    db = dict(K.FGMRES_DB, s_ksp_type="gmres", s_pc_type="jacobi", s_ksp_rtol="1e-3", s_ksp_max_it="30",
              s_pls_gmres_basis="single")
    assert S.field_major_index_sets(spec)[0].size == 8450
    ref = _reference(spec, params, db, target="ksp_s")
    solves, its = len(ref["first"]), sum(e[0] for e in ref["first"])
    counters = tuple(sum(e[i] for e in ref["first"]) for i in (1, 2, 3))
    assert its > solves
    h, _, _, _ = _device(spec, params, db, ref)
    st, bst = h.ksp_stats("s_"), h.gmres_basis_stats("s_")
    print(f"s_ solves {st[0]} ({solves}) its {st[1]} ({its}); basis stats {bst} ({counters})")
    assert st[0] == solves and st[1] == its
    assert bst == (1, CB.basis_bytes(8450, 30, True)) + counters
    assert h.gmres_basis_stats("global_")[0] == 0


# ------------------------------------------------------- 5. edge cases ----
def test_norm_none_max_it_8(gpu):
    spec = S.SynthSpec(2, 12)
    db = dict(G.table_db("2d12_right"), global_ksp_norm_type="none", global_ksp_max_it="8", **SINGLE)
    ref = _reference(spec, G.PARAMS, db)
    assert (ref["its"], ref["reason"], ref["ho"].size) == (8, CB.CONVERGED_ITS, 0)
    h, _, _, _ = _device(spec, G.PARAMS, db, ref)
    assert h.gmres_basis_stats("global_")[2:] == (0, 0, 0)


def test_estimate_converges_at_max_it(gpu):
    """2d12_right at rtol 1e-6 converges at step 16: with max_it 16 the estimate
    is still confirmed by the true residual."""
    spec = S.SynthSpec(2, 12)
    params = dict(G.PARAMS, **{"solver rtol": 1e-6, "solver maxiter": 16})
    db = dict(G.table_db("2d12_right"), global_ksp_gmres_restart="400", **SINGLE)
    ref = _reference(spec, params, db)
    assert (ref["its"], ref["reason"], ref["ho"].size) == (16, 2, 18) and ref["first"][0][1:4] == (0, 1, 0)
    h, _, _, _ = _device(spec, params, db, ref)
    _outer_stats(h, ref, spec, 400)


@pytest.mark.parametrize("capped", [True, False], ids=["at_max_it", "goes_on"])
def test_failed_confirmation(gpu, capped):
    """3d4_right at rtol 1e-6 ends with an estimate 6 % below the true residual.
    With atol between the two (their geometric mean, from the restatement) and
    no rtol, the estimate of step 11 converges and its confirmation fails: with
    max_it 11 the reason is DIVERGED_ITS, without a cap another cycle follows."""
    spec = S.SynthSpec(3, 4)
    db = dict(G.table_db("3d4_right"), **SINGLE)
    A, o = _oracle(spec, dict(G.PARAMS, **{"solver rtol": 1e-6}), db)
    CB.gmres(o.solver, S.rhs(spec))
    est, true, its = o.solver.history[-2], o.solver.history[-1], o.solver.its
    assert its == 11 and true > 1.03 * est and min(o.solver.history[:-2]) > 1.03 * true
    params = dict(G.PARAMS, **{"solver rtol": 1e-30, "solver atol": float(np.sqrt(est * true))})
    if capped:
        params["solver maxiter"] = its
    ref = _reference(spec, params, db)
    if capped:
        assert (ref["its"], ref["reason"], ref["ho"].size) == (11, -3, 13) and ref["first"][0][1:4] == (0, 1, 1)
    else:
        assert ref["its"] > 11 and ref["reason"] == 3 and ref["first"][0][2:4] == (2, 1)
    h, _, _, _ = _device(spec, params, db, ref)
    _outer_stats(h, ref, spec, 400)


def test_zero_rhs(gpu):
    spec = S.SynthSpec(2, 12)
    db = dict(G.table_db("2d12_right"), **SINGLE)
    h = K._handle(spec, G.PARAMS, db)
    x, r = h.solve(np.zeros(spec.n))
    assert (r.its, r.reason) == (0, 3) and np.array_equal(h.history(), [0.0]) and not np.any(x)
    A, o = _oracle(spec, G.PARAMS, db)
    xo = CB.gmres(o.solver, np.zeros(spec.n))
    assert (o.solver.its, o.solver.reason, o.solver.history) == (0, 3, [0.0]) and not np.any(xo)


# ------------------------------------------------------- 6. properties ----
def test_reproducible_and_double_is_the_default_bitwise(gpu):
    spec = S.SynthSpec(3, 4)
    db = G.table_db("3d4_right")
    b = S.rhs(spec)

    def run(extra):
        h = K._handle(spec, G.PARAMS, dict(db, **extra))
        x, r = h.solve(b)
        return x, h.history(), h.gmres_basis_stats("global_")

    x1, h1, st1 = run(SINGLE)
    x2, h2, st2 = run(SINGLE)
    assert st1 == st2 and st1[0] == 1
    assert np.array_equal(h1, h2) and np.array_equal(x1, x2)
    xd, hd, std = run({})
    xe, he, ste = run({"global_pls_gmres_basis": "double", "global_pls_gmres_basis_drop": "1e-3"})
    assert std == ste and std[0] == 0 and std[2:] == (0, 0, 0)
    assert np.array_equal(hd, he) and np.array_equal(xd, xe)
    assert not np.array_equal(h1[:hd.size], hd[:h1.size])


def test_debug_bounds_guards_the_fp32_basis(gpu):
    """pls.debug_bounds puts guard floats behind the fp32 basis too and checks
    them after every solve: the solve passes the check and is bitwise the
    unguarded one (restart 5: the last column, next to the guard, is written in
    every cycle)."""
    spec = S.SynthSpec(2, 12)
    db = dict(G.table_db("2d12_right_restart5"), **SINGLE)
    b = S.rhs(spec)
    out = []
    for extra in ({}, {"pls.debug_bounds": "1"}):
        h = K._handle(spec, G.PARAMS, dict(db, **extra))
        x, r = h.solve(b)
        assert r.reason == 2
        out.append((x, h.history(), h.gmres_basis_stats("global_")))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert out[1][2][1] == out[0][2][1] + 4 * (1 << 16)  # the guard is part of the allocation


def test_chebyshev_estimate_keeps_a_double_basis(gpu):
    """The eigenvalue estimate's child KSP ignores the option: the bounds of an
    s_ chebyshev KSP are bitwise the same with s_pls_gmres_basis single (which
    chebyshev itself ignores)."""
    spec = S.SynthSpec(2, 12)
    db = dict(K.FGMRES_DB, s_ksp_type="chebyshev", s_pc_type="jacobi", s_ksp_norm_type="none", s_ksp_max_it="4")
    b = S.rhs(spec)
    out = []
    for extra in ({}, {"s_pls_gmres_basis": "single", "s_pls_gmres_basis_drop": "0.5"}):
        h = K._handle(spec, K.BASE, dict(db, **extra))
        x, r = h.solve(b)
        out.append((np.array(h.chebyshev_bounds("s_")), h.history(), x))
        with pytest.raises(RuntimeError, match="not gmres or fgmres"):
            h.gmres_basis_stats("s_")
    for a, c in zip(*out):
        assert np.array_equal(a, c)


def test_facade_path_options_file(gpu):
    """Solver(...) with the option in the options file: it travels through the
    options database to the outer KSP."""
    from lib import options as popts
    from lib.IndexSet import IndexSet
    from lib.Parser import load_options_lines
    from lib.Preconditioner import Preconditioner
    from lib.Solver import Solver
    spec = S.SynthSpec(2, 12)
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    db = dict(G.table_db("2d12_right"), **SINGLE)
    params = dict(G.PARAMS, **{"solver rtol": 1e-6})
    ref = _reference(spec, params, db)
    popts.DB.clear()
    try:
        load_options_lines([f"-{k} {v}" for k, v in db.items()])
        index_map = IndexSet(S.field_major_index_sets(spec), two_way=True)
        pc = Preconditioner(index_map, A, P, Pd, params, S.bcs_sub_pressure(spec)).get_pc()
        b = ref["b"]
        solver = Solver(A, b, pc, params, index_map)
        solver.create_solver(A, b, pc)
        solver.set_up()
        x = np.zeros_like(b)
        solver.solve(b, x)
        assert solver.getIterationNumber() == ref["its"] and solver.getConvergedReason() == ref["reason"]
        hist = np.asarray(solver.history)
        assert hist.shape == ref["ho"].shape
        assert np.max(np.abs(hist - ref["ho"]) / ref["ho"]) <= ref["tol"]
        assert pc.handle.gmres_basis_stats("global_")[0] == 1
        assert pc.handle.gmres_basis_stats("global_")[2:] == ref["first"][0][1:4]
    finally:
        popts.DB.clear()


# ---------------------------------------------------------- 7. refusals ----
@pytest.mark.parametrize("extra,match", [
    ({"global_pls_gmres_basis": "half"}, "global_pls_gmres_basis.*double, single"),
    ({"global_pls_gmres_basis_drop": "1"}, "global_pls_gmres_basis_drop.*0 <= d < 1"),
    ({"global_pls_gmres_basis_drop": "-0.1"}, "global_pls_gmres_basis_drop.*0 <= d < 1"),
    ({"global_pls_gmres_basis": "single", "global_ksp_gmres_modifiedgramschmidt": None, "pls.gmres_mgs_fused": "1"},
     "global_pls_gmres_basis.*pls.gmres_mgs_fused"),
    ({"s_ksp_type": "gmres", "s_pls_gmres_basis": "float"}, "s_pls_gmres_basis.*double, single"),
])
def test_refusals(gpu, extra, match):
    spec = S.SynthSpec(2, 4)
    with pytest.raises(RuntimeError, match=match):
        h = K._handle(spec, G.PARAMS, dict(G.table_db("2d12_right"), **extra))
        h.solve(S.rhs(spec))


def test_other_types_ignore_the_options_and_have_no_stats(gpu):
    spec = S.SynthSpec(2, 4)
    db = dict(G.BLOCKS_ILU, global_ksp_type="bcgs", global_pls_gmres_basis="half", global_pls_gmres_basis_drop="7")
    h = K._handle(spec, K.BASE, db)
    _, r = h.solve(S.rhs(spec))
    assert r.reason > 0
    with pytest.raises(RuntimeError, match="not gmres or fgmres"):
        h.gmres_basis_stats("global_")
    with pytest.raises(RuntimeError, match="no inner solver with prefix 'nope_'"):
        h.gmres_basis_stats("nope_")
