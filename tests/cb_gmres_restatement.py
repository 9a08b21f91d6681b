"""numpy restatement of compressed-basis GMRES / FGMRES (a helper, not a
conftest): ``<prefix>pls_gmres_basis single``, the Krylov basis stored in fp32
with every sum, w and the Hessenberg matrix in fp64 (Aliaga, Anzt et al.,
"Compressed basis GMRES").

``gmres_orthog_restatement.gmres`` with the rules added; written, as that file
is, only in terms of ``ksp.matvec / dot / norm / pc.apply``, the tolerances and
``oracle.petsc.ConvergedDefault``, so the oracle's PCs and the rank-ordered
sums of ``oracle/dist.py`` carry over.  A test installs it with

    ksp.solve = lambda b: gmres(ksp, b)

The rules:

  rounding   v0 = fl32(r (1/res)), v_{k+1} = fl32(w (1/tt)) (no happy
             breakdown); fl32 rounds to nearest even to fp32 and promotes back.
             The operator and the PC are applied to the rounded vector, and
             h = V^T w, w -= V h, ||w|| and V y use the rounded vectors.
             FGMRES keeps Z in fp64.
  (a)        with a norm type other than none, a cycle also ends once the
             estimate res <= drop * res0c, res0c the residual recorded at the
             cycle's start (drop 0: off).  Counted only where the cycle would
             otherwise go on.
  (b)        a positive reason from a Givens estimate ends the cycle, not the
             solve: x is built, the next cycle start computes and records the
             true residual (right: ||b - A x||, left: ||B (b - A x)||) at the
             same its, and ConvergedDefault on that value ends the solve or
             the iteration goes on -- also at its == max_it, where a failed
             check is DIVERGED_ITS (confirm False: off).
  none       norm type none: nothing recorded or tested, max_it steps,
             CONVERGED_ITS.

With ``rounding=identity``, ``drop=0`` and ``confirm=False`` this is
``oracle.petsc._gmres`` bit for bit.

``gmres`` sets, besides ``ksp.its / reason / history`` and the counters of
gmres_orthog_restatement (orthog_steps, second_passes, nearest_decision):
  ksp.cb_forced     cycles ended by rule (a)
  ksp.cb_confirm    confirmations done under rule (b)
  ksp.cb_failed     confirmations that failed and led to another cycle
  ksp.cb_ratios     res / (drop * res0c) of every estimate rule (a) looked at
"""
import math

import numpy as np

import gmres_orthog_restatement as G
from oracle import petsc

CONVERGED_ITS = 4

# The TABLE cases of gmres_orthog_restatement (CGS refine_never, ILU blocks, drop 1e-6) as
# measured when this was written: name -> {rtol: (its, history entries, cycles ended by rule
# (a), confirmations, failed confirmations)}.  In double the same cases take 16 / 16 / 11 / 32
# iterations at rtol 1e-6 and 20 / 20 / 14 / 61 at 1e-10.
RECORDED = {"2d12_left": {1e-6: (16, 18, 0, 1, 0), 1e-10: (29, 32, 1, 1, 0)},
            "2d12_right": {1e-6: (16, 18, 0, 1, 0), 1e-10: (29, 32, 1, 1, 0)},
            "3d4_right": {1e-6: (11, 13, 0, 1, 0), 1e-10: (19, 22, 1, 1, 0)},
            "2d12_right_restart5": {1e-6: (32, 40, 0, 1, 0), 1e-10: (61, 75, 0, 1, 0)}}
# Rule (a) decisions must not be borderline: every res / (drop res0c) outside [0.9, 1.1] in
# the cases picked for that (BAND).  3d4_right, a case the device tests are asked to run, has
# one estimate at 1.047 (the step before the one that converges at rtol 1e-6 and is forced at
# 1e-10); 4.7 % is 1e6 times the device tests' history tolerance, so the decision cannot flip
# there either, and its margin is asserted against NEAR_3D4 instead.
BAND = (0.9, 1.1)
NOT_BORDERLINE = ("2d12_left", "2d12_right", "2d12_right_restart5")
NEAR_3D4 = 1e-2


def check_ratios(name, ratios):
    """Assert that no rule (a) decision of this case is borderline."""
    r = np.asarray(ratios, dtype=np.float64)
    if name in NOT_BORDERLINE:
        assert not np.any((r >= BAND[0]) & (r <= BAND[1])), f"bad input: a rule (a) decision of {name} is borderline"
    elif r.size:
        assert np.min(np.abs(r - 1.0)) >= NEAR_3D4, f"bad input: a rule (a) decision of {name} is borderline"


def fl32(v):
    with np.errstate(over="ignore"):
        return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def identity(v):
    return v


def basis_bytes(n, restart, single):
    """The device's basis allocation: restart + 1 columns, 512-byte aligned."""
    if single:
        return (restart + 1) * ((n + 127) // 128 * 128) * 4
    return (restart + 1) * ((n + 63) // 64 * 64) * 8


def gmres(ksp, b, orth="cgs", refine="never", flexible=False, rounding=fl32, drop=1e-6, confirm=True):
    assert orth in ("cgs", "mgs") and refine in ("never", "ifneeded", "always")
    assert 0.0 <= drop < 1.0
    b = np.asarray(b, dtype=np.float64)
    n = b.size
    x = np.zeros(n)
    conv = petsc.ConvergedDefault(ksp.rtol, ksp.atol, ksp.dtol)
    right = flexible or ksp.pc_side == "right"
    normed = getattr(ksp, "norm_type", None) != "none"
    max_k = ksp.restart
    its = 0
    reason = 0
    hist = []
    stats = {"steps": 0, "second": 0, "nearest": math.inf}
    forced_n = confirm_n = failed_n = 0
    ratios = []
    first = True
    confirming = False
    while True:
        r = b.copy() if first else b - ksp.matvec(x)
        if not right:
            r = ksp.pc.apply(r)
        res = ksp.norm(r)
        if normed:
            hist.append(res)
        if res == 0.0:
            reason = petsc.CONVERGED_ATOL
            break
        if normed:
            reason = conv(its, res)
            if confirming:
                confirm_n += 1
                if not reason:
                    failed_n += 1
        confirming = False
        if reason:
            break
        if its >= ksp.maxit:
            reason = petsc.DIVERGED_ITS if normed else CONVERGED_ITS
            break
        res0c = res
        V = [rounding(r * (1.0 / res))]
        Z = []
        HH = np.zeros((max_k + 1, max_k + 1))
        cc = np.zeros(max_k + 1)
        ss = np.zeros(max_k + 1)
        grs = np.zeros(max_k + 2)
        grs[0] = res
        loc_it = 0
        creason = 0
        forced = False
        while not creason and not forced and loc_it < max_k and its < ksp.maxit:
            v = V[loc_it]
            if right:
                z = ksp.pc.apply(v)
                if flexible:
                    Z.append(z)
                w = ksp.matvec(z)
            else:
                w = ksp.pc.apply(ksp.matvec(v))
            h, w, tt = G.orthogonalise(ksp, V, loc_it + 1, w, orth, refine, stats)
            HH[:loc_it + 1, loc_it] = h
            HH[loc_it + 1, loc_it] = tt
            hapbnd = min(abs(tt / grs[loc_it]), G.HAPTOL)
            hapend = tt < hapbnd
            if not hapend:
                with np.errstate(divide="ignore"):
                    inv = np.float64(1.0) / np.float64(tt)
                with np.errstate(invalid="ignore", over="ignore"):
                    w = rounding(w * inv)
            V.append(w)
            it = loc_it
            for j in range(it):
                t0 = HH[j, it]
                HH[j, it] = cc[j] * t0 + ss[j] * HH[j + 1, it]
                HH[j + 1, it] = cc[j] * HH[j + 1, it] - ss[j] * t0
            if not hapend:
                t0 = math.sqrt(HH[it, it] * HH[it, it] + HH[it + 1, it] * HH[it + 1, it])
                if t0 == 0.0:
                    creason = petsc.DIVERGED_NULL
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
            if normed:
                hist.append(res)
                creason = conv(its, res)
            if hapend and not creason:
                creason = petsc.DIVERGED_BREAKDOWN
                break
            if normed and not creason and drop > 0.0:
                ratios.append(res / (drop * res0c))
                forced = res <= drop * res0c and loc_it < max_k and its < ksp.maxit
        it = loc_it - 1
        if it >= 0:
            if HH[it, it] == 0.0:
                creason = petsc.DIVERGED_BREAKDOWN
            else:
                nrs = np.zeros(it + 1)
                nrs[it] = grs[it] / HH[it, it]
                for k in range(it - 1, -1, -1):
                    t0 = grs[k]
                    for j in range(k + 1, it + 1):
                        t0 = t0 - HH[k, j] * nrs[j]
                    nrs[k] = t0 / HH[k, k]
                tmp = np.zeros(n)
                B = Z if flexible else V
                for j in range(it + 1):
                    tmp = tmp + nrs[j] * B[j]
                if right and not flexible:
                    tmp = ksp.pc.apply(tmp)
                x = x + tmp
        first = False
        if creason < 0 or (creason > 0 and not confirm):
            reason = creason
            break
        if creason > 0:
            confirming = True
            continue
        if its >= ksp.maxit:
            reason = petsc.DIVERGED_ITS if normed else CONVERGED_ITS
            break
        if forced:
            forced_n += 1
    ksp.its, ksp.reason, ksp.history = its, reason, hist
    ksp.orthog_steps = stats["steps"]
    ksp.second_passes = stats["second"]
    ksp.nearest_decision = stats["nearest"]
    ksp.cb_forced, ksp.cb_confirm, ksp.cb_failed, ksp.cb_ratios = forced_n, confirm_n, failed_n, ratios
    return x
