"""The restatement of KSPSolve with an initial guess and of Fischer's model 2
(tests/ksp_guess_restatement.py) pinned on the CPU: with nothing to add it is
the oracle's own solve bit for bit, the projection space keeps its invariants,
the guess is the least-squares minimiser, and the 12-step sequences of the
table cases take the recorded iteration counts with no borderline decision."""
import numpy as np
import pytest
import scipy.sparse as sp

import gmres_orthog_restatement as G
import ksp_guess_restatement as R
from oracle import petsc
from oracle import synthetic as S
from oracle.solver import OracleSolver

CASES = ("2d12_right", "3d4_right", "2d12_left")


def oracle(name, rtol=R.SEQ_RTOL):
    dim, N = G.TABLE[name][:2]
    spec = S.SynthSpec(dim, N)
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    params = dict(G.PARAMS, **{"solver rtol": rtol})
    return spec, A, OracleSolver(A, P, Pd, is_s, is_f, is_p, params, G.table_db(name), S.bcs_sub_pressure(spec))


class Watched(R.Fischer2):
    """Fischer2 that checks the space after every update and the guess against lstsq."""

    def __init__(self, ksp, A, **kw):
        super().__init__(ksp, **kw)
        self.A, self.anorm = A, float(abs(A).sum(axis=1).max())
        self.worst = {"orth": 0.0, "ax": 0.0, "lstsq": 0.0}

    def update(self, x, untouched=False):
        super().update(x, untouched)
        if self.m:
            X, B = np.array(self.X).T, np.array(self.B).T
            self.worst["orth"] = max(self.worst["orth"], float(np.max(np.abs(B.T @ B - np.eye(self.m)))))
            self.worst["ax"] = max(self.worst["ax"], float(np.max(np.abs(self.A @ X - B))) / self.anorm)

    def form(self, b):
        x0 = super().form(b)
        if self.m:
            X = np.array(self.X).T
            c = np.linalg.lstsq(self.A @ X, b, rcond=None)[0]
            ref = X @ c
            self.worst["lstsq"] = max(self.worst["lstsq"], float(np.linalg.norm(x0 - ref) / np.linalg.norm(ref)))
        return x0


@pytest.fixture(scope="module")
def sequences():
    out = {}
    for name in CASES:
        spec, A, o = oracle(name)
        k = o.solver
        b0 = S.rhs(spec)
        steps = R.RECORDED[name][0]
        zero = R.run_sequence(k, A, b0, steps, lambda b: petsc._gmres(k, b))
        g = Watched(k, A, size=R.SEQ_SIZE)
        fis = R.run_sequence(k, A, b0, steps, lambda b: R.guessed_solve(k, b, None, petsc._gmres, guess=g))
        out[name] = (zero, fis, g)
    return out


@pytest.mark.parametrize("name", CASES)
def test_zero_guess_zero_rule_is_the_oracles_gmres_bitwise(name):
    spec, A, o = oracle(name)
    k, b = o.solver, S.rhs(spec)
    x = petsc._gmres(k, b)
    want = (k.its, k.reason, list(k.history))
    y = R.guessed_solve(k, b, np.zeros(spec.n), petsc._gmres, rule="zero")
    assert (k.its, k.reason, list(k.history)) == want and np.array_equal(x, y)
    assert k.guess_reduction == 1.0 and k.guess_rnorm0 is None


@pytest.mark.parametrize("norm_type", ["preconditioned", "unpreconditioned"])
def test_zero_guess_zero_rule_is_the_oracles_cg_bitwise(norm_type):
    n = 400
    A = sp.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(n, n), format="csr")
    k = petsc.KSP(A, petsc.PCJacobi(A), "cg", rtol=1e-8, norm_type=norm_type)
    b = np.sin(np.arange(n) * 0.37) + 0.1
    x = petsc._cg(k, b)
    want = (k.its, k.reason, list(k.history))
    assert want[0] > 3
    y = R.guessed_solve(k, b, np.zeros(n), petsc._cg, rule="zero")
    assert (k.its, k.reason, list(k.history)) == want and np.array_equal(x, y)


@pytest.mark.parametrize("name", CASES)
def test_converged_solution_as_the_guess_takes_no_iteration(name):
    spec, A, o = oracle(name)
    k, b = o.solver, S.rhs(spec)
    x = petsc._gmres(k, b)
    assert k.its > 5
    y = R.guessed_solve(k, b, x, petsc._gmres)
    assert (k.its, k.reason, len(k.history)) == (0, 2, 1) and np.array_equal(x, y)
    assert k.guess_reduction <= 1e-6
    # measured against its own first residual the same start would iterate
    R.guessed_solve(k, b, x, petsc._gmres, rule="zero")
    assert k.its > 0


@pytest.mark.parametrize("name", CASES)
def test_columns_stay_orthonormal_and_the_guess_is_the_least_squares_minimiser(sequences, name):
    """After every update of the 12-step sequence max |B^T B - I| <= 1e-12, and every guess is
    the lstsq minimiser of ||b - A X c|| to 1e-10 relative (measured: 4e-16 and 2e-15)."""
    _, _, g = sequences[name]
    print(name, g.worst)
    assert g.worst["orth"] <= 1e-12
    assert g.worst["lstsq"] <= 1e-10


@pytest.mark.parametrize("name", CASES)
def test_stored_pairs_satisfy_B_equals_AX(sequences, name):
    """After every update max |A X - B| <= 1e-12 ||A||_inf (measured: 4e-16, 2e-15, 4e-16).  With
    the new pair taken as (x - X a, A x - B a) / nu alone it was 6.8e-11 and 2.8e-11 on the 2-D
    cases, at the update after the one-iteration solve of step 7: nu = 1e-6 ||A x|| there, and the
    rounding of A x, eps ||A x||, is eps / 1e-6 of the normalised column.  Hence the rule that
    forms B's column again as a product where nu < REFORM ||A x||."""
    _, _, g = sequences[name]
    print(name, g.worst)
    assert g.worst["ax"] <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_recorded_sequence(sequences, name):
    zero, fis, g = sequences[name]
    steps, want_f, want_z, want_stats = R.RECORDED[name]
    assert steps >= 9
    assert [s["its"] for s in fis] == want_f and [s["its"] for s in zero] == want_z
    assert all(s["reason"] == 2 for s in fis + zero)
    assert g.stats() == want_stats
    if name.startswith("2d12"):
        assert g.resets == 2  # (3d4_right: one; see RECORDED)
    tf, tz = sum(want_f), sum(want_z)
    print(f"{name}: {tf} iterations with the Fischer guess, {tz} from zero ({tf / tz:.2f})")
    assert tf < 0.6 * tz


@pytest.mark.parametrize("name", CASES)
def test_no_decision_is_borderline(sequences, name):
    _, fis, _ = sequences[name]
    m = [R.margin(s["history"], s["ttol"]) for s in fis]
    print(name, "margins", " ".join(f"{v:.3f}" for v in m))
    assert min(m) >= R.BAND, f"bad input: step {int(np.argmin(m))} of {name} decides within {min(m):.3e} of ttol"


def test_same_rhs_twice_second_solve_is_free_and_its_update_skipped():
    spec, A, o = oracle("2d12_right")
    k, b = o.solver, S.rhs(spec)
    g = R.Fischer2(k, size=4)
    solve = lambda bb: R.guessed_solve(k, bb, None, petsc._gmres, guess=g)  # noqa: E731
    x1 = solve(b)
    assert k.its > 5 and g.stats() == (1, 1, 4, 1, 0, 0) and k.guess_reduction == 1.0
    x2 = solve(b)
    assert (k.its, k.reason, len(k.history)) == (0, 2, 1)
    assert g.stats() == (1, 1, 4, 2, 1, 0)
    assert np.linalg.norm(x2 - x1) <= 1e-12 * np.linalg.norm(x1)
    # the same through the nu test itself (an update that is told nothing about the solve)
    g.update(x2)
    assert g.stats() == (1, 1, 4, 2, 2, 0)


def test_size_one_resets_at_every_update():
    spec, A, o = oracle("3d4_right")
    k, b0 = o.solver, S.rhs(spec)
    g = R.Fischer2(k, size=1)
    R.run_sequence(k, A, b0, 6, lambda b: R.guessed_solve(k, b, None, petsc._gmres, guess=g))
    assert g.stats() == (1, 1, 1, 6, 0, 5)


def test_nan_solution_leaves_the_space_alone():
    spec, A, o = oracle("2d12_right")
    k = o.solver
    g = R.Fischer2(k, size=1)
    g.update(S.rhs(spec))
    x = np.full(spec.n, np.nan)
    g.update(x)
    assert g.stats() == (1, 1, 1, 0, 0, 0)  # (a full space, and no reset either)


def test_inner_solves_of_the_pc_keep_their_own_rnorm0():
    """Only the guessed KSP's own ConvergedDefault takes the forced rnorm0: an
    inner CG inside the PC is the same solve as without the wrapper."""
    spec = S.SynthSpec(2, 12)
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    db = dict(G.table_db("2d12_right"), s_ksp_type="cg", s_pc_type="jacobi", s_ksp_rtol="1e-10")
    params = dict(G.PARAMS, **{"solver rtol": 1e-6})
    o = OracleSolver(A, P, Pd, is_s, is_f, is_p, params, db, S.bcs_sub_pressure(spec))
    k, b = o.solver, S.rhs(spec)
    x = petsc._gmres(k, b)
    want = (k.its, list(k.history))
    y = R.guessed_solve(k, b, np.zeros(spec.n), petsc._gmres)  # x0 = 0: rnorm0 = ||b|| is the first residual
    assert (k.its, list(k.history)) == want and np.array_equal(x, y)
    assert petsc.ConvergedDefault.__name__ == "ConvergedDefault"
