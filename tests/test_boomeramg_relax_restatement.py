"""tests/boomeramg_relax_restatement.py pinned on the CPU: the default type
is the oracle bit for bit, a Jacobi / l1scaled-Jacobi sweep is the dense formula, Chebyshev of
order k is the Chebyshev polynomial numpy.polynomial.chebyshev gives, the cycle of a symmetric
block is symmetric, and the iteration counts the feature's case rests on:

block solves (CG, unpreconditioned norm, b = default_rng(1), pls.hypre_relax_chunks 1, the inexact
set's BoomerAMG on the lifted block K'), iterations at rtol 1e-1 / 1e-6:

    block (rows)                  sym-SOR/Jacobi  Chebyshev 2  Chebyshev 3  l1scaled-Jacobi  Jacobi w = 0.7
    footing N = 10, s (3,690)         6 / 29        9 / 48       8 / 39        16 / 86       indefinite PC after 3
    swelling 2-D N = 8, s (578)       5 / 29        7 / 45       5 / 37        15 / 82       indefinite PC after 6
    footing N = 20, s (14,818)       10 / 54       15 / 95      11 / 77        27 / 160      indefinite PC after 3
    footing N = 10 / 20, f            1 / 5         1 / 5        1 / 4          2 / 11         2 / 9

whole solves (options/inexact, np_options(8), P with the s and f blocks' constrained columns
zeroed, every BoomerAMG with the same relax type): outer its, s_ its (solves, max):

    footing N = 10, undrained     sym-SOR/Jacobi 36, 224 (37, 8);  Chebyshev 2 36, 294 (37, 10);
                                  Chebyshev 3 36, 243 (37, 9);     l1scaled-Jacobi 37, 581 (38, 18)
    swelling N = 10, diagonal     sym-SOR/Jacobi 32, 472 (33, 22); Chebyshev 2 32, 603 (33, 28);
                                  Chebyshev 3 33, 497 (34, 23);    l1scaled-Jacobi 32, 1144 (33, 51)
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
from numpy.polynomial import chebyshev as NC

import bc_columns_restatement as R
import boomeramg_relax_restatement as BR
import oracle.boomeramg as OB
from oracle import petsc as OP
from oracle.amg import power_lambda

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "tools"), os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

TYPES = {
    "sor": {},
    "cheb2": {"pc_hypre_boomeramg_relax_type_all": "Chebyshev", "pls_boomeramg_chebyshev_order": "2"},
    "cheb3": {"pc_hypre_boomeramg_relax_type_all": "Chebyshev", "pls_boomeramg_chebyshev_order": "3"},
    "l1": {"pc_hypre_boomeramg_relax_type_all": "l1scaled-Jacobi"},
    "jac07": {"pc_hypre_boomeramg_relax_type_all": "Jacobi", "pc_hypre_boomeramg_relax_weight_all": "0.7"},
}
INDEFINITE = -8  # KSP_DIVERGED_INDEFINITE_PC


def _typed(db, t, prefixes):
    db = dict(db)
    for pre in prefixes:
        db.update({pre + k: v for k, v in TYPES[t].items()})
    return db


# ------------------------------------------------------------ hand matrix -----
def _hand():
    """7 rows, symmetric, constant diagonal 4 (so D^-1 A is symmetric), one zero diagonal added
    by the callers that need it; row 5 has a positive off-diagonal."""
    rows = [[0, 1, 3], [0, 1, 2], [1, 2, 3, 6], [0, 2, 3, 4], [3, 4, 5], [4, 5, 6], [2, 5, 6]]
    vals = [[4.0, -1.0, -0.5], [-1.0, 4.0, -2.0], [-2.0, 4.0, -0.25, -1.5], [-0.5, -0.25, 4.0, -1.0],
            [-1.0, 4.0, 0.75], [0.75, 4.0, -1.0], [-1.5, -1.0, 4.0]]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return sp.csr_matrix((np.concatenate(vals), np.concatenate(rows), rp), shape=(7, 7))


def _bare(rtype, no_cf=True, K=1, order=2, fraction=0.3, weight=1.0):
    """The restatement's _relax without a hierarchy."""
    pc = object.__new__(BR.PCBoomerAMGRelax)
    pc.relax_type, pc.no_cf, pc.K, pc.order, pc.fraction, pc.weight = rtype, no_cf, K, order, fraction, weight
    return pc


CF = np.array([OB.C, OB.F, OB.F, OB.C, OB.F, OB.C, OB.F])


@pytest.mark.parametrize("rtype", ["Jacobi", "l1scaled-Jacobi"])
@pytest.mark.parametrize("no_cf", [True, False])
def test_jacobi_sweep_is_the_dense_formula(rtype, no_cf):
    A = _hand().tolil()
    A[4, 4] = 0.0  # a stored zero diagonal: m_4 = 1
    A = A.tocsr()
    Ad = A.toarray()
    w = 0.7
    d = np.diag(Ad)
    if rtype == "Jacobi":
        m = np.array([w / d[i] if d[i] != 0.0 else 1.0 for i in range(7)])
    else:
        m = np.array([np.sign(d[i]) / np.abs(Ad[i]).sum() if d[i] != 0.0 else 1.0 for i in range(7)])
    assert m[4] == 1.0
    rng = np.random.default_rng(0)
    b, x0 = rng.standard_normal(7), rng.standard_normal(7)
    for order in ("CF", "FC"):
        for K in (1, 2):
            pc = _bare(rtype, no_cf=no_cf, K=K, weight=w)
            x = pc._relax({"A": A, "cf": CF}, b, x0.copy(), order)
            ref = x0.copy()
            for _ in range(K):
                masks = [np.ones(7, bool)] if no_cf else [CF == (OB.C if o == "C" else OB.F) for o in order]
                for mask in masks:
                    ref = ref + np.diag(np.where(mask, m, 0.0)) @ (b - Ad @ ref)
            assert np.max(np.abs(x - ref)) <= 1e-14 * np.max(np.abs(ref))
    if not no_cf:  # a C sweep leaves the F points where they were, bit for bit
        pc = _bare(rtype, no_cf=False, weight=w)
        L = {"A": A, "cf": np.where(CF == OB.C, OB.C, OB.F)}
        ms = pc._m_sets(L)
        xc = x0 + ms["C"][1] * (b - A @ x0)
        assert np.array_equal(xc[CF == OB.F], x0[CF == OB.F]) and not np.array_equal(xc[CF == OB.C], x0[CF == OB.C])


@pytest.mark.parametrize("fraction", [0.3, 0.1])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_chebyshev_is_the_chebyshev_polynomial(k, fraction):
    """x_k = p_k(D^-1 A) D^-1 b with 1 - t p_k(t) = T_k((theta - t) / delta) / T_k(sigma): to 1e-13
    against numpy.polynomial.chebyshev, and |1 - t p_k(t)| <= 1 / T_k(sigma) on [lmin, lmax]."""
    A = _hand()
    Ad = A.toarray()
    dinv = 1.0 / np.diag(Ad)
    lam = float(np.float32(power_lambda(A, dinv, 15)))
    lmax = 1.1 * lam
    lmin = fraction * lmax
    theta, delta = (lmax + lmin) / 2.0, (lmax - lmin) / 2.0
    sigma = theta / delta
    Tk = NC.Chebyshev.basis(k)
    mono = NC.cheb2poly(Tk.coef)  # T_k in powers of z
    B = np.diag(dinv) @ Ad
    Z = (theta * np.eye(7) - B) / delta
    TZ = np.zeros((7, 7))
    for c in mono[::-1]:  # Horner
        TZ = TZ @ Z + c * np.eye(7)
    resid = TZ / Tk(sigma)  # the residual polynomial at D^-1 A
    b = np.random.default_rng(4).standard_normal(7)
    ref = np.linalg.solve(B, (np.eye(7) - resid) @ (dinv * b))
    pc = _bare("Chebyshev", order=k, fraction=fraction)
    x = pc._relax({"A": A}, b, np.zeros(7), "CF")
    assert np.max(np.abs(x - ref)) <= 1e-13 * np.max(np.abs(ref))
    # from a nonzero start the error is multiplied by the same polynomial
    x0 = np.random.default_rng(5).standard_normal(7)
    xs = np.linalg.solve(Ad, b)
    x1 = pc._relax({"A": A}, b, x0, "FC")
    assert np.max(np.abs((x1 - xs) - resid @ (x0 - xs))) <= 1e-13 * np.max(np.abs(x0 - xs))
    # two rounds start the recurrence again: the polynomial squared
    x2 = _bare("Chebyshev", K=2, order=k, fraction=fraction)._relax({"A": A}, b, x0, "FC")
    assert np.max(np.abs((x2 - xs) - resid @ resid @ (x0 - xs))) <= 1e-13 * np.max(np.abs(x0 - xs))
    # the bound, on the restatement's own error propagation: with b = 0 a relax call maps an error
    # e to E e, E = r_k(D^-1 A); D^-1 A = A / 4 is symmetric here, so an eigenvector v with
    # eigenvalue t is multiplied by r_k(t) = v^T E v, and |r_k(t)| <= 1 / T_k(sigma) for t in
    # [lmin, lmax] (outside the interval the polynomial is larger: the bound's teeth)
    E = np.column_stack([pc._relax({"A": A}, np.zeros(7), e, "FC") for e in np.eye(7)])
    ev, V = np.linalg.eigh(Ad / 4.0)
    bound = 1.0 / Tk(sigma)
    inside = (ev >= lmin) & (ev <= lmax)
    assert inside.sum() >= 3, (ev, lmin, lmax)
    for t, v in zip(ev, V.T):
        f = v @ E @ v
        assert np.linalg.norm(E @ v - f * v) <= 1e-13
        assert abs(f - Tk((theta - t) / delta) * bound) <= 1e-13
        if lmin <= t <= lmax:
            assert abs(f) <= bound * (1 + 1e-12), (t, f, bound)
    below = ev < lmin
    if below.any():
        assert max(abs(v @ E @ v) for v in V.T[below]) > bound


def test_option_errors_name_the_key():
    A = _hand()
    for key, value, exc in (("s_pc_hypre_boomeramg_relax_type_all", "SOR", NotImplementedError),
                            ("s_pc_hypre_boomeramg_relax_weight_all", "heavy", ValueError),
                            ("s_pls_boomeramg_chebyshev_order", "5", ValueError),
                            ("s_pls_boomeramg_chebyshev_order", "0", ValueError),
                            ("s_pls_boomeramg_chebyshev_fraction", "1.0", ValueError),
                            ("s_pls_boomeramg_chebyshev_fraction", "0", ValueError)):
        with pytest.raises(exc) as e:
            BR.PCBoomerAMGRelax(A, {key: value}, "s_")
        assert key in str(e.value), str(e.value)


# ------------------------------------------------------------ FE blocks -------
def _system(name):
    if name.startswith("footing"):
        from lib.fe_footing import assemble_footing
        return assemble_footing(int(name[7:9]), "undrained")
    from lib.fe_swelling import assemble_swelling
    return assemble_swelling(2, 8, "diagonal")


_blocks = {}


def _block(name):
    """(K', prefix) of footing10_s / footing10_f / footing20_s / footing20_f / swelling08_s."""
    if name not in _blocks:
        s = _system(name)
        pre = "f_" if name.endswith("_f") else "s_"
        K = R.block_of(s.P, s.is_f if pre == "f_" else s.is_s)
        _blocks[name] = (R.split(K)[1], pre)
    return _blocks[name]


def _inexact_db():
    from robustness import load_set
    return dict(load_set("inexact"), **{"pls.hypre_relax_chunks": "1"})


def test_default_type_is_the_oracle_bit_for_bit():
    Kp, pre = _block("swelling08_s")
    for extra in ({}, {"s_pc_hypre_boomeramg_no_CF": "false"}, {"s_pc_hypre_boomeramg_grid_sweeps_all": "2"}):
        db = dict(_inexact_db(), **extra)
        b = np.random.default_rng(2).standard_normal(Kp.shape[0])
        assert np.array_equal(BR.PCBoomerAMGRelax(Kp, db, pre).apply(b), OB.PCBoomerAMG(Kp, db, pre).apply(b))
    old = BR.install()
    try:
        assert OB.PCBoomerAMG is BR.PCBoomerAMGRelax
    finally:
        BR.uninstall(old)
    assert OB.PCBoomerAMG is old and old is not BR.PCBoomerAMGRelax


@pytest.mark.parametrize("t", ["sor", "cheb2", "cheb3", "l1", "jac07"])
def test_symmetric_block_gives_a_symmetric_cycle(t):
    Kp, pre = _block("swelling08_s")
    n = Kp.shape[0]
    pc = BR.PCBoomerAMGRelax(Kp, _typed(_inexact_db(), t, [pre]), pre)
    Bm = np.column_stack([pc.apply(e) for e in np.eye(n)])
    asym = np.linalg.norm(Bm - Bm.T) / np.linalg.norm(Bm)
    print(f"{t}: |B - B^T| / |B| = {asym:.2e}")
    assert asym <= 1e-12


# block -> type -> ((its, reason > 0) at rtol 1e-1, at 1e-6); jac07 on the solid blocks: indefinite PC
BLOCK_TABLE = {
    "footing10_s": {"sor": (6, 29), "cheb2": (9, 48), "cheb3": (8, 39), "l1": (16, 86), "jac07": 3},
    "swelling08_s": {"sor": (5, 29), "cheb2": (7, 45), "cheb3": (5, 37), "l1": (15, 82), "jac07": 6},
    "footing20_s": {"sor": (10, 54), "cheb2": (15, 95), "cheb3": (11, 77), "l1": (27, 160), "jac07": 3},
    "footing10_f": {"sor": (1, 5), "cheb2": (1, 5), "cheb3": (1, 4), "l1": (2, 11), "jac07": (2, 9)},
    "footing20_f": {"sor": (1, 5), "cheb2": (1, 5), "cheb3": (1, 4), "l1": (2, 11), "jac07": (2, 9)},
}


@pytest.mark.parametrize("name", list(BLOCK_TABLE))
def test_block_solve_counts(name):
    Kp, pre = _block(name)
    b = np.random.default_rng(1).standard_normal(Kp.shape[0])
    for t, want in BLOCK_TABLE[name].items():
        pc = BR.PCBoomerAMGRelax(Kp, _typed(_inexact_db(), t, [pre]), pre)
        got = []
        for rtol in (1e-1, 1e-6):
            ksp = OP.KSP(Kp, pc, ksp_type="cg", rtol=rtol, atol=0.0, maxit=300, norm_type="unpreconditioned")
            ksp.solve(b)
            got.append((ksp.its, ksp.reason))
        print(name, t, got)
        if isinstance(want, int):
            assert got == [(want, INDEFINITE), (want, INDEFINITE)], (name, t, got)
        else:
            assert [g[0] for g in got] == list(want) and all(g[1] > 0 for g in got), (name, t, got)


# case -> type -> (outer its, s_ its, s_ solves, s_ max)
SOLVE_TABLE = {
    ("footing", 10, "undrained"): {"sor": (36, 224, 37, 8), "cheb2": (36, 294, 37, 10), "cheb3": (36, 243, 37, 9),
                                   "l1": (37, 581, 38, 18)},
    ("swelling", 10, "diagonal"): {"sor": (32, 472, 33, 22), "cheb2": (32, 603, 33, 28), "cheb3": (33, 497, 34, 23),
                                   "l1": (32, 1144, 33, 51)},
}


@pytest.mark.parametrize("case", list(SOLVE_TABLE), ids=lambda c: f"{c[0]}{c[1]}")
def test_whole_solve_counts(case):
    import make_golden_boomeramg_relax as G
    import robustness as RB
    for t, want in SOLVE_TABLE[case].items():
        db = RB.load_set("inexact")
        db.update(RB.np_options(8))
        db = _typed(db, t, ["s_", "f_", "p_", "diff_", "fp_fieldsplit_0_"])
        _, o, inner = G.run(*case, db)
        got = G.summary(o, inner)
        print(case, t, got)
        assert got["reason"] > 0 and got["s_negative"] == 0
        assert (got["its"], got["s_its"], got["s_solves"], got["s_max"]) == want, (case, t, got)


def test_options_file_is_inexact_lift_plus_fifteen_lines():
    lift = [ln for ln in open(os.path.join(ROOT, "options", "inexact-lift")).read().splitlines() if "#" not in ln]
    new = [ln for ln in open(os.path.join(ROOT, "options", "inexact-lift-chebyshev-relax")).read().splitlines()
           if "#" not in ln]
    assert new[:len(lift)] == lift
    want = []
    for pre in ("s_", "f_", "p_", "diff_", "fp_fieldsplit_0_"):
        want += [f"-{pre}pc_hypre_boomeramg_relax_type_all Chebyshev", f"-{pre}pls_boomeramg_chebyshev_order 3",
                 f"-{pre}pls_boomeramg_chebyshev_fraction 0.3"]
    assert new[len(lift):] == want
