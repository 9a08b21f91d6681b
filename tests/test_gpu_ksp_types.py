"""KSP types fgmres and bcgs on the device against their numpy restatements
(tests/ksp_restatements.py, pinned on the CPU by tests/test_ksp_restatements.py).

Tolerances, the project's rule (tests/test_gpu_parity.py): iteration count and
reason exact; every history entry within max(1e-10, 10 x the restatement's own
worst deviation over 4 seeds when every inner PC output is perturbed by 1e-15
relative); the solution within max(1e-8, that bound) relative.  The bound is
computed here, and every test first asserts that the restatement's iteration
count is the same for all seeds: a case where it is not is a bad input.
"""
import numpy as np
import pytest

from ksp_restatements import bcgs, fgmres
from oracle import synthetic as S
from oracle.solver import OracleSolver

pytestmark = pytest.mark.gpu

BASE = {"solver type": "gmres", "solver atol": 1e-8, "solver rtol": 1e-6, "solver maxiter": 300,
        "pc type": "diagonal", "inner ksp type": "preonly", "inner pc type": "ilu", "inner rtol": 1e-6,
        "inner atol": 0, "inner maxiter": 1000, "inner monitor": False, "solver monitor": False,
        "inner accel order": 0, "AAR order": 10, "AAR p": 5, "AAR omega": 1, "AAR beta": 1}
BLOCKS_ILU = {"s_ksp_type": "preonly", "s_pc_type": "ilu", "f_ksp_type": "preonly", "f_pc_type": "ilu",
              "p_ksp_type": "preonly", "p_pc_type": "ilu", "diff_ksp_type": "preonly", "diff_pc_type": "ilu",
              "fp_ksp_type": "preonly", "fp_pc_type": "ilu"}
FGMRES_DB = dict(BLOCKS_ILU, global_ksp_type="fgmres", global_ksp_gmres_restart="300")
# (dim, N, pc type)
CASES = [(2, 12, "diagonal"), (2, 12, "diagonal 3-way"), (3, 4, "diagonal")]
IDS = ["2d12", "2d12_3way", "3d4"]
INNER = ("ksp_s", "ksp_fp", "ksp_f", "ksp_p")


def _handle(spec, params, db):
    from lib.handle import Handle, params_to_options
    opts = dict(db)
    opts.update(params_to_options(params))
    return Handle.synthetic(spec.dim, spec.N, spec.seed, spec.delta, opts)


def _oracle(spec, params, db, outer, inner_s=None):
    """The oracle with restatements installed: outer = ("fgmres",) or
    ("bcgs", right); inner_s likewise for the s block's KSP."""
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    o = OracleSolver(A, P, Pd, is_s, is_f, is_p, params, db, S.bcs_sub_pressure(spec))

    def install(ksp, kind, right=False):
        if kind == "fgmres":
            ksp.solve = lambda b: fgmres(ksp, b)
        else:
            ksp.solve = lambda b: bcgs(ksp, b, right)

    install(o.solver, *outer)
    if inner_s:
        install(o.block_pc.ksp_s, *inner_s)
    return A, o


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


def _compare(spec, params, db, outer, inner_s=None, b=None):
    b = S.rhs(spec) if b is None else b
    A, o = _oracle(spec, params, db, outer, inner_s)
    xo = o.solve(b)
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
    return A, o, h, x, r


# ------------------------------------------------------------- 1. FGMRES ----
@pytest.mark.parametrize("dim,N,pc_type", CASES, ids=IDS)
def test_fgmres_outer(gpu, dim, N, pc_type):
    _, _, _, _, r = _compare(S.SynthSpec(dim, N), dict(BASE, **{"pc type": pc_type}), FGMRES_DB, ("fgmres",))
    assert r.pc_applies == r.its  # no PC application in BuildSoln


def test_fgmres_restarted(gpu):
    spec = S.SynthSpec(2, 12)
    db = dict(FGMRES_DB, global_ksp_gmres_restart="7")
    A, o, _, x, r = _compare(spec, BASE, db, ("fgmres",))
    assert o.solver.restart == 7 and r.its == 38


# ---------------------------------------- 2. FGMRES over a variable PC ----
def test_fgmres_variable_inner_cg(gpu):
    """Inner CG at rtol 1e-1 is not a fixed operator: FGMRES's last estimate is
    the true residual (right GMRES's is off by > 1e3: tests/test_ksp_restatements.py)."""
    spec = S.SynthSpec(2, 12)
    db = dict(FGMRES_DB, s_ksp_type="cg", s_pc_type="jacobi", s_ksp_norm_type="unpreconditioned", s_ksp_rtol="1e-1")
    b = S.rhs(spec)
    _, o = _oracle(spec, BASE, db, ("fgmres",))
    o.solve(b)
    assert o.its == 15
    h = _handle(spec, BASE, db)
    x, r = h.solve(b)
    assert r.its == o.its and r.reason == o.reason
    res = np.linalg.norm(b - h.matmult(x))
    last = h.history()[-1]
    print(f"true residual {res:.6e}, last history entry {last:.6e}")
    assert res <= (1 + 1e-6) * last


# --------------------------------------------------------- 3. outer BCGS ----
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("dim,N,pc_type", CASES, ids=IDS)
def test_bcgs_outer(gpu, dim, N, pc_type, side):
    db = dict(BLOCKS_ILU, global_ksp_type="bcgs", global_ksp_pc_side=side)
    _compare(S.SynthSpec(dim, N), dict(BASE, **{"pc type": pc_type}), db, ("bcgs", side == "right"))


@pytest.mark.parametrize("side", ["left", "right"])
def test_bcgs_outer_max_it(gpu, side):
    db = dict(BLOCKS_ILU, global_ksp_type="bcgs", global_ksp_pc_side=side, global_ksp_max_it="3")
    _, _, h, _, r = _compare(S.SynthSpec(2, 12), BASE, db, ("bcgs", side == "right"))
    assert r.reason == -3 and r.its == 3 and h.history().size == 4


@pytest.mark.parametrize("side", ["left", "right"])
def test_bcgs_zero_rhs(gpu, side):
    spec = S.SynthSpec(2, 6)
    db = dict(BLOCKS_ILU, global_ksp_type="bcgs", global_ksp_pc_side=side)
    b = np.zeros(spec.n)
    _, o = _oracle(spec, BASE, db, ("bcgs", side == "right"))
    xo = o.solve(b)
    h = _handle(spec, BASE, db)
    x, r = h.solve(b)
    assert r.its == o.its == 0 and r.reason == o.reason
    assert not np.any(x) and not np.any(xo)


# --------------------------------------------------------- 4. inner BCGS ----
def test_bcgs_inner_s(gpu):
    """s_ksp_type bcgs (left, Jacobi) at s_ksp_rtol 1e-3 under outer FGMRES; the
    restatement's iteration counts are the same for all four seeds at 1e-3
    (checked on the CPU), so 1e-3 it is."""
    spec = S.SynthSpec(2, 12)
    db = dict(FGMRES_DB, s_ksp_type="bcgs", s_pc_type="jacobi", s_ksp_rtol="1e-3")
    totals = {"solves": 0, "its": 0}
    A, o = _oracle(spec, BASE, db, ("fgmres",), ("bcgs", False))
    ks = o.block_pc.ksp_s
    counted = ks.solve

    def solve(v):
        y = counted(v)
        totals["solves"] += 1
        totals["its"] += ks.its
        return y

    ks.solve = solve
    b = S.rhs(spec)
    xo = o.solve(b)
    want = dict(totals)
    its, reason, ho = o.its, o.reason, np.asarray(o.history)
    tol = max(1e-10, 10 * _noise_floor(o, b, ho, its))
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
    assert st[0] == want["solves"] and st[1] == want["its"]


# ------------------------------------------------------------ 5. bitwise ----
SETTINGS = [{"pls.bcgs_device": "0"},
            {"pls.bcgs_device": "1", "pls.bcgs_fused_reduce": "0"},
            {"pls.bcgs_device": "1", "pls.bcgs_fused_reduce": "1"}]
VARIANTS = {"plain": {}, "max_it3": {"s_ksp_max_it": "3"}, "rtol1e-8": {"s_ksp_rtol": "1e-8"},
            "rtol1e-13": {"s_ksp_rtol": "1e-13"}, "right": {"s_ksp_pc_side": "right"}}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_bcgs_drivers_bitwise(gpu, variant):
    """The host driver, the device loop with separate final sums and the device
    loop with single-launch reductions: the same x, history, iteration counts
    and reasons, bit for bit.  2-D N=32, 3-way: ns = 8450 rows give three
    reduction blocks (the last-arriver path sees more than one), np = 1089 is
    odd and fits one.  max_it3 ends at the iteration limit.  The device loop
    enqueues one iteration per read-back up to iteration 32, then i / 16 (at
    most 8): the s block's BiCGStab takes 21 to 24 iterations at rtol 1e-8 and
    34 to 40 at 1e-13 (restatement, CPU), so rtol1e-13 is the variant whose
    solves end inside a batch of 2, with the vector kernels and state phases
    enqueued behind the end skipped.  The outer GMRES stops after 4
    iterations: nothing here depends on its convergence."""
    spec = S.SynthSpec(2, 32)
    params = dict(BASE, **{"pc type": "diagonal 3-way", "solver maxiter": 4})
    db = dict(BLOCKS_ILU, global_ksp_type="gmres", global_ksp_pc_side="right", s_ksp_type="bcgs", p_ksp_type="bcgs",
              s_pc_type="jacobi", p_pc_type="jacobi", **{"pls.ksp_stats": "1"})
    db.update(VARIANTS[variant])
    b = S.rhs(spec)
    out = []
    for setting in SETTINGS:
        h = _handle(spec, params, dict(db, **setting))
        x, r = h.solve(b)
        out.append((x, h.history(), r.its, r.reason, np.array(h.ksp_stats("s_") + h.ksp_stats("p_"))))
    print("s_ / p_ stats", out[0][4])
    if variant == "max_it3":
        assert out[0][4][2] == 3 and out[0][4][4] == -3
    if variant == "rtol1e-13":
        assert out[0][4][2] > 33  # iterations 32 and 33 share a batch
    for x, hist, its, reason, st in out[1:]:
        assert its == out[0][2] and reason == out[0][3]
        assert np.array_equal(st, out[0][4])
        assert np.array_equal(hist, out[0][1])
        assert np.array_equal(x, out[0][0])


def test_bcgs_drivers_bitwise_long_solves(gpu):
    """The same three settings where a solve outlasts iteration 128, from which
    the device loop enqueues 8 iterations per read-back: the solid block of the
    2-D N=24 finite-element swelling system (4,802 rows, two reduction blocks)
    takes ~246 Jacobi-preconditioned BiCGStab iterations to rtol 1e-8
    (restatement, CPU; the synthetic blocks above take at most 40).  Two outer
    iterations are enough."""
    from lib import fe_swelling as F
    from lib.handle import Handle, params_to_options
    s = F.assemble_swelling(2, 24, "diagonal")
    params = dict(BASE, **{"solver maxiter": 2})
    db = {"global_ksp_type": "gmres", "global_ksp_pc_side": "right", "s_ksp_type": "bcgs", "s_pc_type": "jacobi",
          "s_ksp_rtol": "1e-8", "fp_ksp_type": "preonly", "fp_pc_type": "ilu"}
    out = []
    for setting in SETTINGS:
        opts = dict(db, **setting)
        opts.update(params_to_options(params))
        h = Handle.from_csr(s.A, s.P, s.P_diff, s.is_s, s.is_f, s.is_p, s.bcs_sub_pressure, opts)
        x, r = h.solve(s.b)
        out.append((x, h.history(), r.its, r.reason, np.array(h.ksp_stats("s_"))))
    print("s_ stats", out[0][4])
    assert out[0][4][2] > 136 and out[0][4][3] == 0  # a batch of 8 was entered; every s_ solve converged
    for x, hist, its, reason, st in out[1:]:
        assert its == out[0][2] and reason == out[0][3]
        assert np.array_equal(st, out[0][4])
        assert np.array_equal(hist, out[0][1])
        assert np.array_equal(x, out[0][0])


# ---------------------------------------------------------- 6. refusals ----
def test_fgmres_refuses_left(gpu):
    spec = S.SynthSpec(2, 4)
    h = _handle(spec, BASE, dict(FGMRES_DB, global_ksp_pc_side="left"))
    with pytest.raises(RuntimeError, match="KSPFGMRES"):
        h.solve(S.rhs(spec))


def test_unknown_ksp_type_lists_supported(gpu):
    spec = S.SynthSpec(2, 4)
    h = _handle(spec, BASE, dict(BLOCKS_ILU, global_ksp_type="tfqmr"))
    with pytest.raises(RuntimeError, match="gmres, fgmres, cg, bcgs, preonly"):
        h.solve(S.rhs(spec))


# ------------------------------------------------------------ 7. facade ----
def test_facade_solver_type_fgmres(gpu):
    """parameters["solver type"] = "fgmres" through the reference's call sequence."""
    from lib import options as popts
    from lib.IndexSet import IndexSet
    from lib.Parser import load_options_lines
    from lib.Preconditioner import Preconditioner
    from lib.Solver import Solver
    spec = S.SynthSpec(2, 8)
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    dofs = S.field_major_index_sets(spec)
    popts.DB.clear()
    load_options_lines([f"-{k} {v}" for k, v in BLOCKS_ILU.items()])
    params = dict(BASE, **{"solver type": "fgmres"})
    index_map = IndexSet(dofs, two_way=True)
    pc = Preconditioner(index_map, A, P, Pd, params, S.bcs_sub_pressure(spec)).get_pc()
    b = S.rhs(spec)
    solver = Solver(A, b, pc, params, index_map)
    solver.create_solver(A, b, pc)
    solver.set_up()
    x = np.zeros_like(b)
    solver.solve(b, x)
    _, o = _oracle(spec, params, BLOCKS_ILU, ("fgmres",))
    xo = o.solve(b)
    assert o.solver.restart == 30  # restart = maxiter only for "gmres"
    assert solver.getIterationNumber() == o.its
    assert np.linalg.norm(x - xo) <= 1e-8 * np.linalg.norm(xo)
    popts.DB.clear()
