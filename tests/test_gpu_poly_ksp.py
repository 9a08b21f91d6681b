"""KSP types richardson and chebyshev on the device against their numpy
restatements (tests/poly_restatements.py, pinned on the CPU by
tests/test_poly_restatements.py).

The comparison and the tolerance rule are those of tests/test_gpu_ksp_types.py
(copied: importing that module would collect its tests a second time):
iteration count and reason exact; every history entry within max(1e-10, 10 x
the restatement's own worst deviation over 4 seeds when every inner PC output
is perturbed by 1e-15 relative); the solution within max(1e-8, that bound)
relative.  Every case first asserts that the restatement's iteration count is
the same for all seeds.  An estimated Chebyshev solver estimates anew in every
restated outer solve, so the seeds perturb the estimate too.
"""
import numpy as np
import pytest

from oracle import synthetic as S
from oracle.solver import OracleSolver
from poly_restatements import chebyshev, esteig, richardson

pytestmark = pytest.mark.gpu

BASE = {"solver type": "gmres", "solver atol": 1e-8, "solver rtol": 1e-6, "solver maxiter": 300,
        "pc type": "diagonal", "inner ksp type": "preonly", "inner pc type": "ilu", "inner rtol": 1e-6,
        "inner atol": 0, "inner maxiter": 1000, "inner monitor": False, "solver monitor": False,
        "inner accel order": 0, "AAR order": 10, "AAR p": 5, "AAR omega": 1, "AAR beta": 1}
BLOCKS_ILU = {"s_ksp_type": "preonly", "s_pc_type": "ilu", "f_ksp_type": "preonly", "f_pc_type": "ilu",
              "p_ksp_type": "preonly", "p_pc_type": "ilu", "diff_ksp_type": "preonly", "diff_pc_type": "ilu",
              "fp_ksp_type": "preonly", "fp_pc_type": "ilu"}
GMRES_DB = dict(BLOCKS_ILU, global_ksp_type="gmres", global_ksp_pc_side="right")
FGMRES_DB = dict(BLOCKS_ILU, global_ksp_type="fgmres", global_ksp_gmres_restart="300")
BOUNDS = "0.15,1.6"
CHEB_S = {"s_ksp_type": "chebyshev", "s_pc_type": "jacobi", "s_ksp_norm_type": "none", "s_ksp_max_it": "4"}
RICH_S = {"s_ksp_type": "richardson", "s_pc_type": "ilu", "s_ksp_norm_type": "none", "s_ksp_max_it": "2",
          "s_ksp_richardson_scale": "0.8"}
# (dim, N, pc type): 2-D N = 12 has ns = 1250 and, 3-way, np = 169 rows (below one workgroup); 3-D N = 4 ns = 2187
CASES = [(2, 12, "diagonal"), (2, 12, "diagonal 3-way"), (3, 4, "diagonal")]
IDS = ["2d12", "2d12_3way", "3d4"]
INNER = ("ksp_s", "ksp_fp", "ksp_f", "ksp_p")


def _handle(spec, params, db):
    from lib.handle import Handle, params_to_options
    opts = dict(db)
    opts.update(params_to_options(params))
    return Handle.synthetic(spec.dim, spec.N, spec.seed, spec.delta, opts)


def _install(ksp, db, prefix, fresh):
    """ksp.solve = the restatement of its type, configured from the prefix's options; `fresh`
    collects the callbacks that forget an estimate (called before every outer solve)"""
    if ksp.type == "richardson":
        scale = float(db.get(prefix + "ksp_richardson_scale", 1.0))
        ksp.solve = lambda b: richardson(ksp, b, scale)
        return
    assert ksp.type == "chebyshev"
    state = {}
    if prefix + "ksp_chebyshev_eigenvalues" in db:
        lo, hi = (float(t) for t in db[prefix + "ksp_chebyshev_eigenvalues"].split(","))
        state["fixed"] = (lo, hi, float("nan"), float("nan"))
    else:
        fresh.append(lambda: state.pop("est", None))

    def solve(b):
        if "fixed" not in state and "est" not in state:
            state["est"] = esteig(ksp, int(db.get(prefix + "ksp_chebyshev_esteig_steps", 10)))
        ksp.bounds = state.get("fixed") or state["est"]
        return chebyshev(ksp, b, ksp.bounds[0], ksp.bounds[1])

    ksp.solve = solve


def _oracle(spec, params, db, outer=None, inner=("s_",)):
    """The oracle with restatements installed: outer None (the oracle's own GMRES), "fgmres" or
    "poly" (the outer solver is richardson / chebyshev); inner: prefixes of the blocks that are"""
    from ksp_restatements import fgmres
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    o = OracleSolver(A, P, Pd, is_s, is_f, is_p, params, db, S.bcs_sub_pressure(spec))
    o.fresh = []
    if outer == "fgmres":
        ksp = o.solver
        ksp.solve = lambda b: fgmres(ksp, b)
    elif outer == "poly":
        _install(o.solver, db, "global_", o.fresh)
    for prefix in inner:
        _install(getattr(o.block_pc, "ksp_" + prefix[:-1]), db, prefix, o.fresh)
    return A, o


def _solve(o, b):
    for f in o.fresh:
        f()
    return o.solve(b)


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
        _solve(o, b)
        for pc, orig in saved:
            pc.apply = orig
        assert o.its == its, f"bad input: the restatement takes {o.its} iterations with seed {seed}, {its} without"
        h2 = np.asarray(o.history)
        worst = max(worst, float(np.max(np.abs(h2 - ho) / np.abs(ho))))
    return worst


def _compare(spec, params, db, outer=None, inner=("s_",), b=None):
    b = S.rhs(spec) if b is None else b
    A, o = _oracle(spec, params, db, outer, inner)
    xo = _solve(o, b)
    its, reason, ho = o.its, o.reason, np.asarray(o.history)
    tol = max(1e-10, 10 * _noise_floor(o, b, ho, its))
    h = _handle(spec, params, db)
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
    return A, o, h, x, r, tol


def _fixed_operator(h, b, x):
    """a polynomial inner solve is a fixed linear operator: plain right GMRES's last estimate is
    the true residual norm (the restatement gives 1 + 1.7e-11 and 1 + 8e-10)"""
    res = np.linalg.norm(b - h.matmult(x))
    last = h.history()[-1]
    print(f"true residual {res:.6e}, last history entry {last:.6e}, ratio - 1 = {res / last - 1:.2e}")
    assert res <= (1 + 1e-6) * last


# ------------------------------------- (a) Chebyshev, explicit bounds ----
@pytest.mark.parametrize("dim,N,pc_type", CASES, ids=IDS)
def test_chebyshev_inner_explicit_bounds(gpu, dim, N, pc_type):
    spec = S.SynthSpec(dim, N)
    db = dict(GMRES_DB, **CHEB_S, s_ksp_chebyshev_eigenvalues=BOUNDS)
    b = S.rhs(spec)
    _, o, h, x, r, _ = _compare(spec, dict(BASE, **{"pc type": pc_type}), db, b=b)
    assert r.reason == 2
    _fixed_operator(h, b, x)
    st = h.ksp_stats("s_")
    assert st[1] == 4 * st[0] and st[2] == 4 and st[3] == 0  # every s_ solve: 4 iterations, CONVERGED_ITS
    emin, emax, lo, hi = h.chebyshev_bounds("s_")
    assert (emin, emax) == (0.15, 1.6) and np.isnan(lo) and np.isnan(hi)


# ------------------------------------ (b) Chebyshev, estimated bounds ----
@pytest.mark.parametrize("dim,N,pc_type", CASES, ids=IDS)
def test_chebyshev_inner_estimated_bounds(gpu, dim, N, pc_type):
    spec = S.SynthSpec(dim, N)
    db = dict(GMRES_DB, **CHEB_S)
    b = S.rhs(spec)
    _, o, h, x, r, tol = _compare(spec, dict(BASE, **{"pc type": pc_type}), db, b=b)
    assert r.reason == 2
    _fixed_operator(h, b, x)
    got, want = np.array(h.chebyshev_bounds("s_")), np.array(o.block_pc.ksp_s.bounds)
    print("bounds", got, "restatement", want)
    assert np.max(np.abs(got - want) / np.abs(want)) <= tol
    assert got[1] == 1.1 * got[3] and got[0] == 0.1 * got[3]


def test_chebyshev_esteig_options(gpu):
    """ksp_chebyshev_esteig a,b,c,d and ksp_chebyshev_esteig_steps reach the estimate"""
    spec = S.SynthSpec(2, 12)
    db = dict(GMRES_DB, **CHEB_S, s_ksp_chebyshev_esteig="0.5,0.05,0,1.2", s_ksp_chebyshev_esteig_steps="6")
    h = _handle(spec, BASE, db)
    h.solve(S.rhs(spec))
    _, o = _oracle(spec, BASE, db)
    want = esteig(o.block_pc.ksp_s, 6, transform=(0.5, 0.05, 0.0, 1.2))
    got = h.chebyshev_bounds("s_")
    assert np.max(np.abs(np.array(got) - np.array(want)) / np.abs(want)) <= 1e-10
    assert got[0] == 0.5 * got[2] + 0.05 * got[3] and got[1] == 1.2 * got[3]


# --------------------------------------------------- (c) Richardson ----
@pytest.mark.parametrize("dim,N,pc_type", CASES, ids=IDS)
def test_richardson_inner(gpu, dim, N, pc_type):
    spec = S.SynthSpec(dim, N)
    b = S.rhs(spec)
    _, o, h, x, r, _ = _compare(spec, dict(BASE, **{"pc type": pc_type}), dict(GMRES_DB, **RICH_S), b=b)
    assert r.reason == 2
    _fixed_operator(h, b, x)
    st = h.ksp_stats("s_")
    assert st[1] == 2 * st[0] and st[3] == 0


# ---------------------------------------------- (d) normed Chebyshev ----
@pytest.mark.parametrize("N,norm_type,solves,total", [(12, "preconditioned", 14, 211), (32, "preconditioned", 23, 433),
                                                      (12, "unpreconditioned", 14, 217)],
                         ids=["2d12_pre", "2d32_pre", "2d12_unpre"])
def test_chebyshev_inner_normed(gpu, N, norm_type, solves, total):
    """Chebyshev/Jacobi (estimated bounds) to s_ksp_rtol 1e-3 under outer FGMRES, the host loop with
    one norm read back per iteration; N = 32: 8,450 rows, three reduction blocks.  The s_ solves and
    their iterations in total equal the restatement's (the numbers recorded on the CPU)."""
    spec = S.SynthSpec(2, N)
    db = dict(FGMRES_DB, s_ksp_type="chebyshev", s_pc_type="jacobi", s_ksp_norm_type=norm_type, s_ksp_rtol="1e-3")
    totals = {"solves": 0, "its": 0}
    A, o = _oracle(spec, BASE, db, "fgmres")
    ks = o.block_pc.ksp_s
    counted = ks.solve

    def solve(v):
        y = counted(v)
        totals["solves"] += 1
        totals["its"] += ks.its
        return y

    ks.solve = solve
    b = S.rhs(spec)
    xo = _solve(o, b)
    want = dict(totals)
    assert (want["solves"], want["its"]) == (solves, total)
    its, reason, ho = o.its, o.reason, np.asarray(o.history)
    tol = max(1e-10, 10 * _noise_floor(o, b, ho, its, seeds=4 if N <= 12 else 2))
    h = _handle(spec, BASE, db)
    x, r = h.solve(b)
    hist = h.history()
    st = h.ksp_stats("s_")
    print(f"its {r.its} ({its}); s_ solves {st[0]} ({want['solves']}) its {st[1]} ({want['its']}); tol {tol:.2e}")
    assert r.its == its and r.reason == reason
    rel = np.max(np.abs(hist - ho) / np.abs(ho))
    print(f"history rel diff {rel:.3e}")
    assert rel <= tol
    assert np.linalg.norm(x - xo) <= max(1e-8, tol) * np.linalg.norm(xo)
    assert st[0] == want["solves"] and st[1] == want["its"] and st[3] == 0


# ------------------------------------------- (e) Jacobi fusion bitwise ----
@pytest.mark.parametrize("norm_type", ["none", "unpreconditioned"])
def test_poly_fuse_jacobi_bitwise(gpu, norm_type):
    """PCJacobi's product inside the update kernel (pls.poly_fuse_jacobi 1, the default) against
    pc->apply followed by the update: the same x, history and stats, bit for bit.  2-D N = 32,
    3-way: ns = 8450 rows (more than one workgroup, no multiple of 256), np = 1089."""
    spec = S.SynthSpec(2, 32)
    params = dict(BASE, **{"pc type": "diagonal 3-way", "solver maxiter": 4})
    db = dict(GMRES_DB, s_ksp_type="chebyshev", s_pc_type="jacobi", s_ksp_norm_type=norm_type, s_ksp_max_it="5",
              s_ksp_rtol="1e-30", p_ksp_type="richardson", p_pc_type="jacobi", p_ksp_norm_type=norm_type,
              p_ksp_max_it="3", p_ksp_richardson_scale="0.8", p_ksp_rtol="1e-30")
    b = S.rhs(spec)
    out = []
    for fuse in ("0", "1"):
        h = _handle(spec, params, dict(db, **{"pls.poly_fuse_jacobi": fuse}))
        x, r = h.solve(b)
        out.append((x, h.history(), r.its, r.reason, np.array(h.ksp_stats("s_") + h.ksp_stats("p_")),
                    np.array(h.chebyshev_bounds("s_"))))
    print("s_ / p_ stats", out[0][4])
    assert out[0][2] == 4 and out[0][4][1] == 5 * out[0][4][0] and out[0][4][6] == 3 * out[0][4][5]
    assert np.all(np.isfinite(out[0][0])) and np.any(out[0][0])
    for a, c in zip(out[0], out[1]):
        assert np.array_equal(a, c)


# ---------------------------------------------------- (f) outer type ----
@pytest.mark.parametrize("kind", ["richardson", "chebyshev"])
def test_poly_outer(gpu, kind):
    """global_ksp_type richardson / chebyshev over the 2-way block PC, 5 iterations with the
    preconditioned norm (the default): DIVERGED_ITS, six history entries."""
    spec = S.SynthSpec(2, 12)
    db = dict(BLOCKS_ILU, global_ksp_type=kind, global_ksp_max_it="5", global_ksp_richardson_scale="0.9",
              global_ksp_chebyshev_eigenvalues="0.3,1.8")
    _, o, h, x, r, _ = _compare(spec, BASE, db, "poly", inner=())
    assert r.reason == -3 and r.its == 5 and h.history().size == 6
    assert h.history()[-1] < h.history()[0]


# ------------------------------------------------------ (g) refusals ----
@pytest.mark.parametrize("extra,match", [
    ({"s_ksp_type": "chebyshev", "s_ksp_pc_side": "right"}, r"KSPCHEBYSHEV \(s_\)"),
    ({"s_ksp_type": "richardson", "s_ksp_pc_side": "right"}, r"KSPRICHARDSON \(s_\)"),
    ({"global_ksp_type": "chebyshev", "global_ksp_pc_side": "right"}, r"KSPCHEBYSHEV \(global_\)"),
    ({"s_ksp_type": "chebyshev", "s_ksp_chebyshev_eigenvalues": "1.6,1.6"}, r"KSPCHEBYSHEV \(s_\).*0 < emin < emax"),
    ({"s_ksp_type": "chebyshev", "s_ksp_chebyshev_eigenvalues": "2.0,1.6"}, r"KSPCHEBYSHEV \(s_\).*0 < emin < emax"),
    ({"s_ksp_type": "chebyshev", "s_ksp_chebyshev_eigenvalues": "-0.1,1.6"}, r"KSPCHEBYSHEV \(s_\).*0 < emin < emax"),
    ({"s_ksp_type": "richardson", "s_ksp_richardson_self_scale": "1"}, r"KSPRICHARDSON \(s_\).*self_scale"),
    ({"global_ksp_type": "tfqmr"}, "gmres, fgmres, cg, bcgs, preonly, richardson, chebyshev"),
], ids=["cheb_right", "rich_right", "outer_right", "emin_eq_emax", "emin_gt_emax", "negative", "self_scale", "unknown"])
def test_poly_refusals(gpu, extra, match):
    spec = S.SynthSpec(2, 4)
    with pytest.raises(RuntimeError, match=match):
        h = _handle(spec, BASE, dict(GMRES_DB, **extra))
        h.solve(S.rhs(spec))


def test_chebyshev_bounds_refusals(gpu):
    spec = S.SynthSpec(2, 4)
    h = _handle(spec, BASE, dict(GMRES_DB, **CHEB_S))
    h.setup()
    with pytest.raises(RuntimeError, match="has not run a solve"):
        h.chebyshev_bounds("s_")
    h.solve(S.rhs(spec))
    assert h.chebyshev_bounds("s_")[1] > h.chebyshev_bounds("s_")[0] > 0
    with pytest.raises(RuntimeError, match="pls_get_chebyshev_bounds.*not chebyshev"):
        h.chebyshev_bounds("global_")
    with pytest.raises(RuntimeError, match="pls_get_chebyshev_bounds"):
        h.chebyshev_bounds("nosuch_")


# -------------------------------------------------------- (h) facade ----
@pytest.mark.parametrize("where", ["inner ksp type", "solver type"])
def test_facade_poly_types(gpu, where):
    """parameters["inner ksp type"] = "chebyshev" and ["solver type"] = "richardson" through the
    reference's call sequence (Preconditioner / Solver)."""
    from lib import options as popts
    from lib.IndexSet import IndexSet
    from lib.Parser import load_options_lines
    from lib.Preconditioner import Preconditioner
    from lib.Solver import Solver
    spec = S.SynthSpec(2, 8)
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    dofs = S.field_major_index_sets(spec)
    if where == "inner ksp type":
        db = {"s_pc_type": "jacobi", "s_ksp_norm_type": "none", "s_ksp_max_it": "4",
              "s_ksp_chebyshev_eigenvalues": BOUNDS, "fp_ksp_type": "preonly", "fp_pc_type": "ilu"}
        params = dict(BASE, **{"inner ksp type": "chebyshev"})
        outer, inner = None, ("s_",)
    else:
        db = dict(BLOCKS_ILU, global_ksp_richardson_scale="0.9")
        params = dict(BASE, **{"solver type": "richardson", "solver maxiter": 5})
        outer, inner = "poly", ()
    popts.DB.clear()
    load_options_lines([f"-{k} {v}" for k, v in db.items()])
    index_map = IndexSet(dofs, two_way=True)
    pc = Preconditioner(index_map, A, P, Pd, params, S.bcs_sub_pressure(spec)).get_pc()
    b = S.rhs(spec)
    solver = Solver(A, b, pc, params, index_map)
    solver.create_solver(A, b, pc)
    solver.set_up()
    x = np.zeros_like(b)
    solver.solve(b, x)
    _, o = _oracle(spec, params, db, outer, inner)
    xo = _solve(o, b)
    if where == "inner ksp type":
        assert o.block_pc.ksp_s.type == "chebyshev"
        assert o.solver.restart == params["solver maxiter"]  # restart = maxiter: the outer type is gmres
    else:
        assert o.solver.type == "richardson" and o.its == 5
    assert solver.getIterationNumber() == o.its
    assert np.linalg.norm(x - xo) <= 1e-8 * np.linalg.norm(xo)
    popts.DB.clear()


# ------------------------------------------------- (i) matrix update ----
def test_chebyshev_bounds_follow_matrix_update(gpu):
    """pls_update_matrices sets the block solvers up again: the next solve estimates anew.  The
    s block is unpreconditioned here (Jacobi would scale the change away): P doubled doubles its
    spectrum -- exactly, a power of two."""
    from lib.handle import Handle, params_to_options
    spec = S.SynthSpec(2, 9)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    A, P, Pd = (S.matrix(spec, v) for v in (0, 1, 2))
    params = dict(BASE, **{"solver maxiter": 3})
    opts = dict(dict(GMRES_DB, **CHEB_S), s_pc_type="none")
    opts.update(params_to_options(params))
    b = S.rhs(spec)
    h = Handle.from_csr(A, P, Pd, is_s, is_f, is_p, S.bcs_sub_pressure(spec), opts)
    h.solve(b)
    b1 = np.array(h.chebyshev_bounds("s_"))
    h.update_matrices(A, 2.0 * P, Pd)
    h.solve(b)
    b2 = np.array(h.chebyshev_bounds("s_"))
    print(b1, b2)
    assert b1[3] > b1[2] > 0
    assert np.max(np.abs(b2 - 2.0 * b1) / b2) <= 1e-12
    _, o = _oracle(spec, params, opts)
    want = esteig(o.block_pc.ksp_s, 10)
    assert np.max(np.abs(b1 - np.array(want)) / np.abs(want)) <= 1e-10


# ------------------------------------------------ the shipped option set ----
@pytest.mark.parametrize("pc_type", ["diagonal", "diagonal 3-way"])
def test_inexact_chebyshev_option_set(gpu, pc_type):
    """options/inexact-chebyshev (Chebyshev over BoomerAMG on s, f, p and the fieldsplit's split 0,
    bounds estimated) under its plain GMRES: converges, and the last estimate is the true residual."""
    import os
    from oracle import options
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    db = options.parse_options_file(os.path.join(root, "options", "inexact-chebyshev"))
    spec = S.SynthSpec(2, 12)
    b = S.rhs(spec)
    h = _handle(spec, dict(BASE, **{"pc type": pc_type}), db)
    x, r = h.solve(b)
    print("its", r.its, "bounds s_", h.chebyshev_bounds("s_"))
    assert r.reason == 2 and r.its < 60
    _fixed_operator(h, b, x)
    emin, emax, lo, hi = h.chebyshev_bounds("s_")
    assert 0 < emin == 0.1 * hi and emax == 1.1 * hi
    if pc_type == "diagonal":
        assert h.chebyshev_bounds("fp_fieldsplit_0_")[1] > 0
        assert h.ksp_stats("fp_fieldsplit_0_")[2] == 5
    else:
        assert h.ksp_stats("f_")[2] == 3 and h.ksp_stats("p_")[2] == 3
    assert h.ksp_stats("s_")[2] == 2
