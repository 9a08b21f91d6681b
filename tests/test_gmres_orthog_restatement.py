"""The numpy restatement of GMRES's orthogonalisation choices
(tests/gmres_orthog_restatement.py) pinned on the CPU: with classical
Gram-Schmidt and no refinement it is ``oracle.petsc._gmres`` bit for bit; a
second pass restores the basis' orthogonality to rounding; and the iteration
and second-pass counts of the cases the device tests use
(tests/test_gpu_gmres_orthog.py) are the ones recorded when it was written."""
import numpy as np
import pytest

import gmres_orthog_restatement as G
from oracle import petsc
from oracle import synthetic as S
from oracle.solver import OracleSolver

BASE = dict(G.PARAMS, **{"solver atol": 1e-8, "solver rtol": 1e-6, "solver maxiter": 300})  # tests/test_ksp_restatements.py


def oracle(spec, params, db):
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    return OracleSolver(A, P, Pd, is_s, is_f, is_p, params, db, S.bcs_sub_pressure(spec))


@pytest.mark.parametrize("side,restart", [("left", 300), ("right", 300), ("right", 7), ("left", 7)],
                         ids=["left", "right", "right_restart7", "left_restart7"])
def test_unrefined_cgs_is_the_oracles_gmres_bitwise(side, restart):
    spec = S.SynthSpec(2, 12)
    db = dict(G.BLOCKS_ILU, global_ksp_type="gmres", global_ksp_pc_side=side, global_ksp_gmres_restart=str(restart))
    b = S.rhs(spec)
    o = oracle(spec, BASE, db)
    ksp = o.solver
    assert ksp.type == "gmres" and ksp.pc_side == side and ksp.restart == restart
    xo = petsc._gmres(ksp, b)
    its, reason, ho = ksp.its, ksp.reason, np.asarray(ksp.history)
    x = G.gmres(ksp, b)
    assert (ksp.its, ksp.reason) == (its, reason) and reason == 2
    if restart == 7:
        assert its > 7  # restarted at least once
    assert np.array_equal(np.asarray(ksp.history), ho)
    assert np.array_equal(x, xo)
    assert ksp.orthog_steps == its and ksp.second_passes == 0


def test_second_pass_restores_orthogonality():
    """2-D N=12, ILU blocks, rtol 1e-6, right preconditioning: max |V^T V - I|
    was 2.1e-9 unrefined and 8.9e-16 refined when this was written."""
    spec = S.SynthSpec(2, 12)
    db = dict(G.BLOCKS_ILU, global_ksp_type="gmres", global_ksp_pc_side="right", global_ksp_gmres_restart="300")
    b = S.rhs(spec)
    ksp = oracle(spec, BASE, db).solver
    G.gmres(ksp, b)
    unrefined = ksp.orthogonality_loss
    G.gmres(ksp, b, refine="always")
    refined = ksp.orthogonality_loss
    print(f"max |V^T V - I|: unrefined {unrefined:.2e}, refine_always {refined:.2e}")
    assert ksp.second_passes == ksp.its == ksp.orthog_steps
    assert refined <= 1e-14
    assert unrefined >= 1e-11


@pytest.mark.parametrize("name", sorted(G.TABLE))
def test_recorded_counts(name):
    """Iterations (every scheme) and refine_ifneeded's second passes of the
    device tests' cases; no ifneeded decision nearer than 1e-3 to its threshold
    (the nearest were 4.6e-2, 2.9e-1, 2.3e-3 and 3.5e-2)."""
    dim, N, side, restart, n, its, second = G.TABLE[name]
    spec = S.SynthSpec(dim, N)
    assert spec.n == n
    b = S.rhs(spec)
    ksp = oracle(spec, G.PARAMS, G.table_db(name)).solver
    assert ksp.pc_side == side and ksp.restart == restart
    for scheme, (_, kw) in sorted(G.SCHEMES.items()):
        G.gmres(ksp, b, **kw)
        assert ksp.reason == 2 and ksp.its == its, (scheme, ksp.its, ksp.reason)
        assert ksp.orthog_steps == its
        want = {"cgs": 0, "mgs": 0, "refine_always": its, "refine_ifneeded": second}[scheme]
        assert ksp.second_passes == want, (scheme, ksp.second_passes)
        if scheme == "refine_ifneeded":
            print(f"{name}: nearest decision {ksp.nearest_decision:.2e}")
            assert ksp.nearest_decision >= 1e-3
        if scheme in ("refine_always", "refine_ifneeded") and restart == 400:
            assert ksp.orthogonality_loss <= 1e-14
