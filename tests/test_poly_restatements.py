"""The numpy restatements of KSPRICHARDSON / KSPCHEBYSHEV and of the eigenvalue
estimate (tests/poly_restatements.py) pinned without a GPU: the Chebyshev
recurrence against the closed form of its residual polynomial, Richardson's
against (1 - scale lambda)^k, the operation counts and reasons the device tests
rely on, the estimate against a dense eigenvalue computation, and the
library's Hessenberg eigenvalue routine (host code) against numpy."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import petsc
from oracle import synthetic as S
from oracle.solver import OracleSolver
from poly_restatements import chebyshev, esteig, esteig_vector, richardson

BASE = {"solver type": "gmres", "solver atol": 1e-8, "solver rtol": 1e-6, "solver maxiter": 300,
        "pc type": "diagonal", "inner ksp type": "preonly", "inner pc type": "ilu", "inner rtol": 1e-6,
        "inner atol": 0, "inner maxiter": 1000, "inner monitor": False, "solver monitor": False,
        "inner accel order": 0, "AAR order": 10, "AAR p": 5, "AAR omega": 1, "AAR beta": 1}
EMIN, EMAX = 0.3, 2.5
LAM = np.array([0.1, 0.3, 0.5, 0.9, 1.4, 1.9, 2.5, 2.9])  # inside, on and outside the bounds


def _diag_ksp(ktype, maxit, norm_type="none", **kw):
    return petsc.KSP(sp.diags(LAM).tocsr(), petsc.PCNone(), ktype, maxit=maxit, norm_type=norm_type, **kw)


def _cheb_T(k, t):
    """T_k(t) by the three-term recurrence"""
    a, b = np.ones_like(t), t
    if k == 0:
        return a
    for _ in range(k - 1):
        a, b = b, 2.0 * t * b - a
    return b


@pytest.mark.parametrize("k", [1, 2, 3, 6])
def test_chebyshev_residual_polynomial(k):
    """k iterations leave the residual T_k((emax + emin - 2 lambda) / (emax - emin)) /
    T_k((emax + emin) / (emax - emin)) times b."""
    ksp = _diag_ksp("chebyshev", k)
    b = np.ones(LAM.size)
    x = chebyshev(ksp, b, EMIN, EMAX)
    want = _cheb_T(k, (EMAX + EMIN - 2.0 * LAM) / (EMAX - EMIN)) / _cheb_T(k, np.array((EMAX + EMIN) / (EMAX - EMIN)))
    got = b - LAM * x
    print(k, np.max(np.abs(got - want)))
    assert np.max(np.abs(got - want)) <= 1e-14
    assert ksp.its == k and ksp.reason == petsc.CONVERGED_ITS and ksp.history == []


@pytest.mark.parametrize("k", [1, 2, 5])
def test_richardson_residual_polynomial(k):
    ksp = _diag_ksp("richardson", k)
    b = np.ones(LAM.size)
    x = richardson(ksp, b, 0.4)
    got = b - LAM * x
    assert np.max(np.abs(got - (1.0 - 0.4 * LAM) ** k)) <= 1e-14
    assert ksp.its == k and ksp.reason == petsc.CONVERGED_ITS and ksp.history == []


@pytest.mark.parametrize("kind", ["richardson", "chebyshev"])
@pytest.mark.parametrize("maxit", [1, 2, 5])
def test_counts_under_norm_none(kind, maxit):
    """exactly maxit PC applications and maxit - 1 operator products, no norm, no history"""
    ksp = _diag_ksp(kind, maxit)
    counts = {"pc": 0, "mv": 0, "norm": 0}
    pc_apply, matvec = ksp.pc.apply, ksp.matvec

    def count(name, f):
        def g(*a):
            counts[name] += 1
            return f(*a)
        return g

    ksp.pc.apply = count("pc", pc_apply)
    ksp.matvec = count("mv", matvec)
    ksp.norm = count("norm", ksp.norm)
    ksp.dot = count("norm", ksp.dot)
    b = np.ones(LAM.size)
    if kind == "richardson":
        richardson(ksp, b, 0.4)
    else:
        chebyshev(ksp, b, EMIN, EMAX)
    assert counts == {"pc": maxit, "mv": maxit - 1, "norm": 0}
    assert ksp.its == maxit and ksp.reason == petsc.CONVERGED_ITS and ksp.history == []


@pytest.mark.parametrize("norm_type", ["preconditioned", "unpreconditioned"])
@pytest.mark.parametrize("kind", ["richardson", "chebyshev"])
def test_tolerance_stop_and_diverged_its(kind, norm_type):
    """a tolerance that stops the solve at index i: Chebyshev counts its = i + 1 (PETSc's count),
    Richardson its = i; out of iterations with a norm: DIVERGED_ITS, maxit + 1 history entries"""
    b = np.ones(LAM.size)
    run = (lambda k: richardson(k, b, 0.4)) if kind == "richardson" else (lambda k: chebyshev(k, b, 0.05, 3.0))
    ksp = _diag_ksp(kind, 200, norm_type, rtol=1e-3)
    x = run(ksp)
    last = len(ksp.history) - 1
    assert ksp.reason == petsc.CONVERGED_RTOL and 1 < last < 200
    assert ksp.its == (last + 1 if kind == "chebyshev" else last)
    assert ksp.history[-1] <= 1e-3 * ksp.history[0] < ksp.history[-2]
    assert np.linalg.norm(b - LAM * x) <= 2e-3 * np.linalg.norm(b)
    ksp = _diag_ksp(kind, 3, norm_type, rtol=1e-12)
    run(ksp)
    assert ksp.reason == petsc.DIVERGED_ITS and ksp.its == 3 and len(ksp.history) == 4


def test_esteig_vector_is_exact():
    v = esteig_vector(np.arange(5))
    want = [((g + 1) * 2654435761 % 2 ** 32) / 2 ** 32 - 0.5 for g in range(5)]
    assert v.tolist() == want and np.all(np.abs(esteig_vector(np.arange(100000))) <= 0.5)
    big = esteig_vector(np.array([2 ** 31 + 7]))  # past 32 bits: the product stays below 2^64
    assert big[0] == ((2 ** 31 + 8) * 2654435761 % 2 ** 32) / 2 ** 32 - 0.5


def test_esteig_bounds_lambda_max():
    """2-D N = 12 solid block under Jacobi: 1.1 x the 10-step estimate lies above the largest
    eigenvalue of D^-1 A (dense eigvals): 1.593 against 1.477."""
    spec = S.SynthSpec(2, 12)
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    db = {"s_ksp_type": "chebyshev", "s_pc_type": "jacobi", "s_ksp_norm_type": "none", "s_ksp_max_it": "4",
          "fp_ksp_type": "preonly", "fp_pc_type": "ilu"}
    o = OracleSolver(A, P, Pd, is_s, is_f, is_p, BASE, db, S.bcs_sub_pressure(spec))
    ks = o.block_pc.ksp_s
    assert ks.type == "chebyshev" and ks.norm_type == "none" and ks.pc.type == "jacobi"
    emin, emax, lo, hi = esteig(ks, 10)
    true = np.linalg.eigvals(ks.pc.dinv[:, None] * ks.A.toarray()).real
    print(f"estimate [{lo:.4f}, {hi:.4f}], bounds [{emin:.4f}, {emax:.4f}], true [{true.min():.4f}, {true.max():.4f}]")
    assert emax == 1.1 * hi and emin == 0.1 * hi
    assert hi <= true.max() * (1 + 1e-12) <= emax
    assert abs(hi - 1.4480) < 5e-4 and abs(true.max() - 1.4769) < 5e-4


def test_inexact_chebyshev_option_set_parses():
    """options/inexact-chebyshev: the inexact set with no inner CG left, every polynomial solver
    without norms and with an iteration count; the preconditioners are options/inexact's"""
    import os
    from oracle import options
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    db = options.parse_options_file(os.path.join(root, "options", "inexact-chebyshev"))
    ref = options.parse_options_file(os.path.join(root, "options", "inexact"))
    for pre in ("s_", "f_", "p_", "fp_fieldsplit_0_"):
        assert ref[pre + "ksp_type"] == "cg" and db[pre + "ksp_type"] == "chebyshev"
        assert db[pre + "ksp_norm_type"] == "none" and int(db[pre + "ksp_max_it"]) >= 1
    assert "cg" not in db.values() and db["global_ksp_type"] == "gmres"
    same = {k: v for k, v in ref.items() if "_ksp_" not in k or k.startswith(("global_", "diff_", "fp_ksp", "fp_fieldsplit_1"))}
    assert all(db[k] == v for k, v in same.items()) and len(same) > 40


# ------------------------------------------- pls_hessenberg_eigenvalues ----
def _hess_cases():
    rng = np.random.default_rng(7)
    tri = np.diag(np.linspace(1.0, 3.0, 10)) + np.diag(0.5 * np.ones(9), 1) + np.diag(0.5 * np.ones(9), -1)
    rnd = np.triu(rng.standard_normal((10, 10)), -1)
    graded = np.triu(np.outer(np.logspace(0, -8, 8), np.ones(8)) * (1.0 + 0.1 * rng.random((8, 8))), -1)
    split = np.triu(rng.standard_normal((8, 8)), -1)
    split[4, 3] = 0.0
    return {"1x1": np.array([[2.5]]), "2x2_complex_pair": np.array([[1.0, -2.0], [3.0, 1.0]]),
            "tridiagonal_10": tri, "random_10": rnd, "graded_8": graded, "zero_subdiagonal_8": split}


def _match(ev, ref):
    """worst |ev_i - ref_i| / max |ref| over the pairing by nearest value, both sorted first"""
    ev, ref = list(np.sort_complex(ev)), np.sort_complex(ref)
    worst = 0.0
    for r in ref:
        j = int(np.argmin([abs(e - r) for e in ev]))
        worst = max(worst, abs(ev.pop(j) - r))
    return worst / np.max(np.abs(ref))


@pytest.mark.parametrize("name", sorted(_hess_cases()))
def test_hessenberg_eigenvalues(name):
    """Against numpy.linalg.eigvals.  The error is measured against the largest eigenvalue's
    modulus, the scale a backward-stable QR iteration answers for (neither routine promises the
    small eigenvalues of the graded matrix to relative accuracy).  Bound: 10 x numpy's own
    deviation when every entry of H is perturbed by 1e-15 relative, floor 1e-12."""
    import lib._native as N
    H = _hess_cases()[name]
    m = H.shape[0]
    if name == "random_10":
        assert np.any(np.abs(np.linalg.eigvals(H).imag) > 1e-3)  # it has complex pairs
    ref = np.linalg.eigvals(H)
    rng = np.random.default_rng(11)
    floor = max(_match(np.linalg.eigvals(H * (1 + 1e-15 * rng.standard_normal(H.shape))), ref) for _ in range(4))
    tol = max(1e-12, 10 * floor)
    ld = m + 3  # a leading dimension larger than m, garbage below the subdiagonal
    buf = np.full((ld, m), 1e30, order="F")
    buf[:m, :] = np.where(np.tril(np.ones((m, m)), -2) > 0, 1e30, H)
    re, im = np.zeros(m), np.zeros(m)
    rc = N.lib().pls_hessenberg_eigenvalues(m, N.ptr(buf), ld, N.ptr(re), N.ptr(im))
    assert rc == 0
    err = _match(re + 1j * im, ref)
    print(f"{name}: error {err:.2e}, tol {tol:.2e}")
    assert err <= tol


def test_hessenberg_eigenvalues_refuses_bad_sizes():
    import lib._native as N
    z = np.zeros(4)
    assert N.lib().pls_hessenberg_eigenvalues(0, N.ptr(z), 1, N.ptr(z), N.ptr(z)) != 0
    assert N.lib().pls_hessenberg_eigenvalues(65, N.ptr(z), 65, N.ptr(z), N.ptr(z)) != 0
