"""numpy restatements of KSPRICHARDSON and KSPCHEBYSHEV and of Chebyshev's
eigenvalue estimate, for the tests (a helper, not a conftest).

Written only in terms of an ``oracle.petsc.KSP`` object's ``matvec``, ``dot``,
``norm``, ``pc.apply``, ``norm_type``, ``rtol/atol/dtol/maxit`` and
``oracle.petsc.ConvergedDefault`` (tests/ksp_restatements.py), so they inherit
the oracle's PCs and the rank-ordered sums of ``oracle/dist.py``.  Both types
are left-preconditioned with a zero initial guess; ``oracle.petsc.KSP``
constructs for both type strings (left, preconditioned norm by default,
``none`` honoured), and a test installs one with

    ksp.solve = lambda b: chebyshev(ksp, b, emin, emax)

PETSc's sources are not at hand: the recurrences are rich.c and cheby.c as the
project's DESIGN.md section 16 states them, and the Chebyshev one is pinned
independently by the closed form of its residual polynomial
(tests/test_poly_restatements.py).
"""
import numpy as np

from oracle import petsc

ESTEIG_DEFAULT = (0.0, 0.1, 0.0, 1.1)


def _rn(ksp, r):
    """(norm of the residual under ksp.norm_type, B r when it was formed for it)"""
    if ksp.norm_type == "preconditioned":
        z = ksp.pc.apply(r)
        return ksp.norm(z), z
    return ksp.norm(r), None


def richardson(ksp, b, scale=1.0):
    """KSPSolve_Richardson without self-scaling: x += scale B (b - A x)."""
    b = np.asarray(b, dtype=np.float64)
    conv = petsc.ConvergedDefault(ksp.rtol, ksp.atol, ksp.dtol)
    normed = ksp.norm_type != "none"
    x = np.zeros(b.size)
    r = b.copy()
    its, reason, hist = 0, 0, []
    for i in range(ksp.maxit):
        z = None
        if normed:
            dp, z = _rn(ksp, r)
            hist.append(dp)
            reason = conv(i, dp)
            if reason:
                break
        if z is None:
            z = ksp.pc.apply(r)
        x = x + scale * z
        its += 1
        if i + 1 < ksp.maxit or normed:
            r = b - ksp.matvec(x)
    if not reason:
        if not normed:
            reason = petsc.CONVERGED_ITS
        else:
            dp, _ = _rn(ksp, r)
            hist.append(dp)
            reason = conv(ksp.maxit, dp) or petsc.DIVERGED_ITS
    ksp.its, ksp.reason, ksp.history = its, reason, hist
    return x


def chebyshev(ksp, b, emin, emax):
    """KSPSolve_Chebyshev (first kind) on the bounds emin < emax."""
    b = np.asarray(b, dtype=np.float64)
    conv = petsc.ConvergedDefault(ksp.rtol, ksp.atol, ksp.dtol)
    normed = ksp.norm_type != "none"
    scale = 2.0 / (emax + emin)
    alpha = 1.0 - scale * emin
    mu = 1.0 / alpha
    omegaprod = 2.0 / alpha
    c_km1, c_k = 1.0, mu
    hist = []
    reason = 0
    z = None
    if normed:
        dp, z = _rn(ksp, b)
        hist.append(dp)
        reason = conv(0, dp)
    if not reason and ksp.maxit <= 0:
        reason = petsc.DIVERGED_ITS
    if reason:
        ksp.its, ksp.reason, ksp.history = 0, reason, hist
        return np.zeros(b.size)
    if z is None:
        z = ksp.pc.apply(b)
    p_km1 = None  # zero: its term is omitted
    p_k = scale * z
    its = 1
    i = 1
    while i < ksp.maxit:
        its += 1
        c_kp1 = 2.0 * mu * c_k - c_km1
        omega = omegaprod * c_k / c_kp1
        r = b - ksp.matvec(p_k)
        z = None
        if normed:
            dp, z = _rn(ksp, r)
            hist.append(dp)
            reason = conv(i, dp)
            if reason:
                break
        if z is None:
            z = ksp.pc.apply(r)
        p_kp1 = omega * p_k + (omega * scale) * z
        if p_km1 is not None:
            p_kp1 = (1.0 - omega) * p_km1 + p_kp1
        p_km1, p_k = p_k, p_kp1
        c_km1, c_k = c_k, c_kp1
        i += 1
    if not reason:
        if not normed:
            reason = petsc.CONVERGED_ITS
        else:
            dp, _ = _rn(ksp, b - ksp.matvec(p_k))
            hist.append(dp)
            reason = conv(i, dp) or petsc.DIVERGED_ITS
    ksp.its, ksp.reason, ksp.history = its, reason, hist
    return p_k


def esteig_vector(global_rows):
    """The estimate's right-hand side: v_g = ((g + 1) * 2654435761 mod 2^32) / 2^32 - 0.5
    for the block-global row indices g (exact in fp64, the same on every rank count)."""
    g = np.asarray(global_rows, dtype=np.uint64)
    h = ((g + np.uint64(1)) * np.uint64(2654435761)) % np.uint64(2 ** 32)
    return h.astype(np.float64) / 4294967296.0 - 0.5


def esteig(ksp, steps=10, global_rows=None, transform=ESTEIG_DEFAULT):
    """``steps`` Arnoldi steps (classical Gram-Schmidt, no refinement, as the
    GMRES cycle takes them) of the left-preconditioned operator B A on
    ``esteig_vector``; the extreme real parts of the Hessenberg matrix's
    eigenvalues (numpy.linalg.eigvals).  Returns (emin, emax, raw min, raw max).
    ``global_rows``: the operator's rows in the block's global numbering
    (default: 0 .. n - 1, a block held whole)."""
    n = ksp.A.shape[0]
    rows = np.arange(n) if global_rows is None else global_rows
    v = ksp.pc.apply(esteig_vector(rows))
    res = ksp.norm(v)
    V = [v * (1.0 / res)]
    steps = min(steps, n)
    H = np.zeros((steps + 1, steps))
    m = 0
    for k in range(steps):
        w = ksp.pc.apply(ksp.matvec(V[k]))
        h = np.array([ksp.dot(V[j], w) for j in range(k + 1)])
        for j in range(k + 1):
            w = w - h[j] * V[j]
        tt = ksp.norm(w)
        H[:k + 1, k] = h
        H[k + 1, k] = tt
        m = k + 1
        if tt < petsc.GMRES_HAPTOL:
            break
        V.append(w * (1.0 / tt))
    ev = np.linalg.eigvals(H[:m, :m])
    lo, hi = float(ev.real.min()), float(ev.real.max())
    a, b_, c, d = transform
    return a * lo + b_ * hi, c * lo + d * hi, lo, hi
