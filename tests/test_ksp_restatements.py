"""The numpy restatements of KSPFGMRES / KSPBCGS (tests/ksp_restatements.py)
pinned against the CPU oracle: FGMRES with a fixed PC is right-preconditioned
GMRES; with a variable PC its estimate stays the true residual where GMRES's
does not; BiCGStab converges on the same systems with the iteration counts
recorded when the restatement was written."""
import numpy as np
import pytest

from ksp_restatements import bcgs, fgmres
from oracle import synthetic as S
from oracle.solver import OracleSolver

BASE = {"solver type": "gmres", "solver atol": 1e-8, "solver rtol": 1e-6, "solver maxiter": 300,
        "pc type": "diagonal", "inner ksp type": "preonly", "inner pc type": "ilu", "inner rtol": 1e-6,
        "inner atol": 0, "inner maxiter": 1000, "inner monitor": False, "solver monitor": False,
        "inner accel order": 0, "AAR order": 10, "AAR p": 5, "AAR omega": 1, "AAR beta": 1}
ILU_DB = {"global_ksp_type": "gmres", "global_ksp_pc_side": "right",
          "s_ksp_type": "preonly", "s_pc_type": "ilu", "f_ksp_type": "preonly", "f_pc_type": "ilu",
          "p_ksp_type": "preonly", "p_pc_type": "ilu", "diff_ksp_type": "preonly", "diff_pc_type": "ilu",
          "fp_ksp_type": "preonly", "fp_pc_type": "ilu"}  # BASE / ILU_DB of tests/test_gpu_parity.py

# (dim, N, pc type, GMRES its, BiCGStab its left, right)
CASES = [(2, 6, "diagonal", 12, 8, 8), (2, 12, "diagonal", 16, 13, 12), (2, 12, "diagonal 3-way", 16, 12, 12),
         (3, 4, "diagonal", 11, 7, 7)]
IDS = ["2d6", "2d12", "2d12_3way", "3d4"]
VARIABLE_DB = dict(ILU_DB, s_ksp_type="cg", s_pc_type="jacobi", s_ksp_norm_type="unpreconditioned")


def oracle(spec, params, db):
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    return A, OracleSolver(A, P, Pd, is_s, is_f, is_p, params, db, S.bcs_sub_pressure(spec))


@pytest.mark.parametrize("dim,N,pc_type,its,_l,_r", CASES, ids=IDS)
def test_fgmres_fixed_pc_is_right_gmres(dim, N, pc_type, its, _l, _r):
    spec = S.SynthSpec(dim, N)
    params = dict(BASE, **{"pc type": pc_type})
    b = S.rhs(spec)
    _, o = oracle(spec, params, ILU_DB)
    xg = o.solve(b)
    hg = np.asarray(o.history)
    assert o.its == its
    ksp = o.solver
    ksp.restart = 300
    xf = fgmres(ksp, b)
    assert ksp.its == its and ksp.reason == 2
    hf = np.asarray(ksp.history)
    assert hf.shape == hg.shape and np.max(np.abs(hf - hg) / hg) <= 1e-10
    assert np.linalg.norm(xf - xg) <= 1e-12 * np.linalg.norm(xg)


@pytest.mark.parametrize("rtol,its", [("1e-1", 15), ("1e-3", 14)])
def test_variable_pc_fgmres_estimate_is_true_residual(rtol, its):
    """Inner CG to a loose tolerance is not a fixed operator: right GMRES
    reports convergence and returns an x whose residual is > 1e3 times its
    estimate; FGMRES's estimate is the residual."""
    spec = S.SynthSpec(2, 12)
    b = S.rhs(spec)
    A, o = oracle(spec, BASE, dict(VARIABLE_DB, s_ksp_rtol=rtol))
    xg = o.solve(b)
    assert o.its == its and o.reason == 2
    assert np.linalg.norm(b - A @ xg) > 1e3 * o.history[-1]
    ksp = o.solver
    ksp.restart = 300
    xf = fgmres(ksp, b)
    assert ksp.its == its and ksp.reason == 2
    assert np.linalg.norm(b - A @ xf) <= (1 + 1e-6) * ksp.history[-1]


@pytest.mark.parametrize("right", [False, True], ids=["left", "right"])
@pytest.mark.parametrize("dim,N,pc_type,_g,its_l,its_r", CASES, ids=IDS)
def test_bcgs_converges(dim, N, pc_type, _g, its_l, its_r, right):
    spec = S.SynthSpec(dim, N)
    b = S.rhs(spec)
    A, o = oracle(spec, dict(BASE, **{"pc type": pc_type}), ILU_DB)
    ksp = o.solver
    x = bcgs(ksp, b, right)
    assert ksp.reason == 2
    assert ksp.its == (its_r if right else its_l)
    assert len(ksp.history) == ksp.its + 1
    if right:  # the recurrence's residual is the true one (left: the preconditioned one)
        res = np.linalg.norm(b - A @ x)
        assert abs(res - ksp.history[-1]) <= 1e-6 * ksp.history[-1]
