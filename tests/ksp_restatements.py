"""numpy restatements of KSPFGMRES and KSPBCGS for the tests (a helper, not a conftest).

Written only in terms of an ``oracle.petsc.KSP`` object's ``matvec``, ``dot``,
``norm``, ``pc.apply``, ``rtol/atol/dtol/maxit/restart`` and
``oracle.petsc.ConvergedDefault``, so they inherit the oracle's PCs and the
rank-ordered sums of ``oracle/dist.py``.  ``oracle.petsc.KSP(...)`` constructs
for any type string (only ``.solve`` raises), so a test installs one with

    ksp.solve = lambda b: fgmres(ksp, b)

the way ``_self_sensitivity`` of tests/test_gpu_parity.py patches ``pc.apply``.
"""
import math

import numpy as np

from oracle import petsc

HAPTOL = 1e-30


def fgmres(ksp, b):
    """KSPFGMRES: ``oracle.petsc._gmres`` with right preconditioning, the
    preconditioned vectors Z_k = M^-1 V_k kept, x += Z y in BuildSoln (no PC
    application there).  Restart ``ksp.restart``."""
    b = np.asarray(b, dtype=np.float64)
    n = b.size
    x = np.zeros(n)
    conv = petsc.ConvergedDefault(ksp.rtol, ksp.atol, ksp.dtol)
    max_k = ksp.restart
    its = 0
    reason = 0
    hist = []
    first = True
    while not reason:
        r = b.copy() if first else b - ksp.matvec(x)
        res = ksp.norm(r)
        V = [r * (1.0 / res) if res != 0.0 else r]
        Z = []
        hist.append(res)
        if res == 0.0:
            reason = petsc.CONVERGED_ATOL
            break
        reason = conv(its, res)
        HH = np.zeros((max_k + 1, max_k + 1))
        cc = np.zeros(max_k + 1)
        ss = np.zeros(max_k + 1)
        grs = np.zeros(max_k + 2)
        grs[0] = res
        loc_it = 0
        while not reason and loc_it < max_k and its < ksp.maxit:
            z = ksp.pc.apply(V[loc_it])
            Z.append(z)
            w = ksp.matvec(z)
            h = np.array([ksp.dot(V[j], w) for j in range(loc_it + 1)])
            for j in range(loc_it + 1):
                w = w - h[j] * V[j]
            HH[:loc_it + 1, loc_it] = h
            tt = ksp.norm(w)
            HH[loc_it + 1, loc_it] = tt
            hapbnd = min(abs(tt / grs[loc_it]), HAPTOL)
            hapend = tt < hapbnd
            if not hapend:
                w = w * (1.0 / tt)
            V.append(w)
            it = loc_it
            for j in range(it):
                t0 = HH[j, it]
                HH[j, it] = cc[j] * t0 + ss[j] * HH[j + 1, it]
                HH[j + 1, it] = cc[j] * HH[j + 1, it] - ss[j] * t0
            if not hapend:
                t0 = math.sqrt(HH[it, it] * HH[it, it] + HH[it + 1, it] * HH[it + 1, it])
                if t0 == 0.0:
                    reason = petsc.DIVERGED_NULL
                    break
                cc[it] = HH[it, it] / t0
                ss[it] = HH[it + 1, it] / t0
                grs[it + 1] = -(ss[it] * grs[it])
                grs[it] = cc[it] * grs[it]
                HH[it, it] = cc[it] * HH[it, it] + ss[it] * HH[it + 1, it]
                res = abs(grs[it + 1])
            else:
                res = 0.0
            loc_it += 1
            its += 1
            hist.append(res)
            reason = conv(its, res)
            if hapend and not reason:
                reason = petsc.DIVERGED_BREAKDOWN
                break
        it = loc_it - 1
        if it >= 0:
            if HH[it, it] == 0.0:
                reason = petsc.DIVERGED_BREAKDOWN
            else:
                nrs = np.zeros(it + 1)
                nrs[it] = grs[it] / HH[it, it]
                for k in range(it - 1, -1, -1):
                    t0 = grs[k]
                    for j in range(k + 1, it + 1):
                        t0 = t0 - HH[k, j] * nrs[j]
                    nrs[k] = t0 / HH[k, k]
                tmp = np.zeros(n)
                for j in range(it + 1):
                    tmp = tmp + nrs[j] * Z[j]
                x = x + tmp
        if its >= ksp.maxit:
            if not reason:
                reason = petsc.DIVERGED_ITS
            break
        first = False
    ksp.its, ksp.reason, ksp.history = its, reason, hist
    return x


def bcgs(ksp, b, right, norm="default"):
    """KSPSolve_BCGS, zero initial guess.  K = M^-1 A (left, preconditioned
    norm) or A M^-1 (right, unpreconditioned norm, x = M^-1 x after the loop).
    norm "none": no norms, no convergence test (history of zeros)."""
    b = np.asarray(b, dtype=np.float64)
    conv = petsc.ConvergedDefault(ksp.rtol, ksp.atol, ksp.dtol)
    test = norm != "none"
    if right:
        K = lambda u: ksp.matvec(ksp.pc.apply(u))
    else:
        K = lambda u: ksp.pc.apply(ksp.matvec(u))
    x = np.zeros(b.size)
    r = b.copy() if right else ksp.pc.apply(b)
    dp = ksp.norm(r) if test else 0.0
    hist = [dp]
    its = 0
    reason = conv(0, dp) if test else 0
    if reason:
        ksp.its, ksp.reason, ksp.history = its, reason, hist
        return x
    rp = r.copy()
    rhoold = alpha = omegaold = 1.0
    p = np.zeros(b.size)
    v = np.zeros(b.size)
    i = 0
    while True:
        rho = ksp.dot(r, rp)
        beta = (rho / rhoold) * (alpha / omegaold)
        p = r - (omegaold * beta) * v + beta * p
        v = K(p)
        d1 = ksp.dot(v, rp)
        if d1 == 0.0:
            reason = petsc.DIVERGED_BREAKDOWN
            break
        alpha = rho / d1
        s = r - alpha * v
        t = K(s)
        d1 = ksp.dot(s, t)
        d2 = ksp.dot(t, t)
        if d2 == 0.0:
            if ksp.dot(s, s) != 0.0:
                reason = petsc.DIVERGED_BREAKDOWN
                break
            x = x + alpha * p
            its += 1
            hist.append(0.0)
            reason = petsc.CONVERGED_RTOL
            break
        omega = d1 / d2
        x = x + alpha * p + omega * s
        r = s - omega * t
        dp = ksp.norm(r) if test else 0.0
        rhoold = rho
        omegaold = omega
        its += 1
        hist.append(dp)
        if test:
            reason = conv(i + 1, dp)
        if reason:
            break
        if rho == 0.0:
            reason = petsc.DIVERGED_BREAKDOWN
            break
        i += 1
        if i >= ksp.maxit:
            reason = petsc.DIVERGED_ITS
            break
    if right:
        x = ksp.pc.apply(x)
    ksp.its, ksp.reason, ksp.history = its, reason, hist
    return x
