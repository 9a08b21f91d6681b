"""The numpy restatement of compressed-basis GMRES
(tests/cb_gmres_restatement.py) pinned on the CPU: with identity rounding and
both rules off it is ``oracle.petsc._gmres`` bit for bit; the iteration counts,
history lengths and rule counters of the cases the device tests use
(tests/test_gpu_cb_gmres.py) are the ones recorded when it was written; the
last history entry is the true residual; and without the rules an unrestarted
solve to rtol 1e-10 stagnates, which is why the rules exist."""
import numpy as np
import pytest

import cb_gmres_restatement as CB
import gmres_orthog_restatement as G
from oracle import petsc
from oracle import synthetic as S
from oracle.solver import OracleSolver

BASE = dict(G.PARAMS, **{"solver atol": 1e-8, "solver rtol": 1e-6, "solver maxiter": 300})


def oracle(spec, params, db):
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    return A, OracleSolver(A, P, Pd, is_s, is_f, is_p, params, db, S.bcs_sub_pressure(spec))


def true_residual(A, o, b, x, side):
    r = b - A @ x
    return float(np.linalg.norm(r if side == "right" else o.pc.apply(r)))


@pytest.mark.parametrize("side,restart", [("left", 300), ("right", 300), ("right", 7), ("left", 7)],
                         ids=["left", "right", "right_restart7", "left_restart7"])
def test_rules_off_identity_rounding_is_the_oracles_gmres_bitwise(side, restart):
    spec = S.SynthSpec(2, 12)
    db = dict(G.BLOCKS_ILU, global_ksp_type="gmres", global_ksp_pc_side=side, global_ksp_gmres_restart=str(restart))
    b = S.rhs(spec)
    _, o = oracle(spec, BASE, db)
    ksp = o.solver
    xo = petsc._gmres(ksp, b)
    its, reason, ho = ksp.its, ksp.reason, np.asarray(ksp.history)
    x = CB.gmres(ksp, b, rounding=CB.identity, drop=0.0, confirm=False)
    assert (ksp.its, ksp.reason) == (its, reason) and reason == 2
    assert np.array_equal(np.asarray(ksp.history), ho)
    assert np.array_equal(x, xo)
    assert (ksp.cb_forced, ksp.cb_confirm, ksp.cb_failed) == (0, 0, 0)


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", sorted(G.TABLE))
def test_recorded_table_and_true_last_entry(name, rtol):
    """its / history entries / rule counters as recorded; the last history entry
    is the true residual norm (right: ||b - A x||, left: ||B (b - A x)||) to
    1e-12 relative; no rule (a) decision is borderline."""
    dim, N, side, restart, n = G.TABLE[name][:5]
    spec = S.SynthSpec(dim, N)
    assert spec.n == n
    b = S.rhs(spec)
    A, o = oracle(spec, dict(G.PARAMS, **{"solver rtol": rtol}), G.table_db(name))
    ksp = o.solver
    petsc._gmres(ksp, b)
    double_its = ksp.its
    x = CB.gmres(ksp, b)
    got = (ksp.its, len(ksp.history), ksp.cb_forced, ksp.cb_confirm, ksp.cb_failed)
    true = true_residual(A, o, b, x, side)
    print(f"{name} rtol {rtol:g}: double its {double_its}, single {got}; estimate {ksp.history[-2]:.6e} "
          f"last {ksp.history[-1]:.6e} true {true:.6e}")
    assert ksp.reason == 2
    assert got == CB.RECORDED[name][rtol]
    assert abs(ksp.history[-1] - true) <= 1e-12 * true
    CB.check_ratios(name, ksp.cb_ratios)
    if rtol == 1e-6:
        assert ksp.its == double_its  # no cost in iterations at the reference drivers' tolerance


@pytest.mark.parametrize("name", ["2d12_left", "2d12_right", "3d4_right"])
def test_stagnation_without_the_rules(name):
    """Unrestarted, rtol 1e-10, both rules off: the estimate stalls above the
    tolerance (7.6e-10 / 3.9e-9 / 5.5e-9 when this was written) while the true
    residual stays more than 100 times larger (1.0e-7 / 7.6e-7 / 1.2e-6), and the
    solve ends at max_it with DIVERGED_ITS."""
    dim, N, side = G.TABLE[name][:3]
    spec = S.SynthSpec(dim, N)
    b = S.rhs(spec)
    A, o = oracle(spec, G.PARAMS, G.table_db(name))
    ksp = o.solver
    x = CB.gmres(ksp, b, drop=0.0, confirm=False)
    true = true_residual(A, o, b, x, side)
    print(f"{name}: its {ksp.its} reason {ksp.reason} estimate {ksp.history[-1]:.3e} true residual {true:.3e}")
    assert ksp.reason == petsc.DIVERGED_ITS and ksp.its == 400
    assert true > 100 * ksp.history[-1]


def test_norm_none_runs_max_it_steps_without_a_history():
    spec = S.SynthSpec(2, 12)
    db = dict(G.table_db("2d12_right"), global_ksp_norm_type="none", global_ksp_max_it="8")
    b = S.rhs(spec)
    A, o = oracle(spec, G.PARAMS, db)
    ksp = o.solver
    assert ksp.norm_type == "none" and ksp.maxit == 8
    x = CB.gmres(ksp, b)
    assert (ksp.its, ksp.reason, ksp.history) == (8, CB.CONVERGED_ITS, [])
    assert np.linalg.norm(b - A @ x) < 1e-2 * np.linalg.norm(b)
