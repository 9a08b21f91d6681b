"""numpy restatement of compressed-operator GMRES / FGMRES (a helper, not a
conftest): ``<prefix>pls_gmres_operator single`` on top of
``<prefix>pls_gmres_basis single``.

``cb_gmres_restatement.gmres`` with the two products inside the Arnoldi step
taken through ``matvec_low`` -- a product with A^, the operator whose stored
values were rounded to fp32 once (``low_matrix``), x and every sum in fp64.
The product at a cycle start, which gives the true residual that rule (b)
decides on, stays ``ksp.matvec``: a cycle is one step of iterative refinement
with an inexact inner operator.  Everything else -- the rounding of the basis,
rules (a) and (b), the history, ``its`` -- is the cb restatement's, and with
``matvec_low = ksp.matvec`` this is that function bit for bit.

``gmres`` sets what ``cb_gmres_restatement.gmres`` sets, and
  ksp.co_low        products with A^ (one per Arnoldi step: equal to its)
  ksp.co_double     products with A at cycle starts
  ksp.co_confirm    for every confirmation under rule (b): (true residual /
                    threshold, the estimate that asked for it / threshold),
                    threshold = max(rtol * rnorm0, atol)
"""
import math

import numpy as np
import scipy.sparse as sp

import cb_gmres_restatement as CB
import gmres_orthog_restatement as G
from oracle import petsc

# The TABLE cases of gmres_orthog_restatement with the low operator (pure fl32(A), drop 1e-6) as
# measured when this was written: (its, history entries, cycles ended by rule (a), confirmations,
# failed confirmations).  Every case equals cb_gmres_restatement.RECORDED except 3d4_right at
# rtol 1e-10, which takes 16 steps where the fp32 basis alone takes 19.
RECORDED = {name: dict(by_rtol) for name, by_rtol in CB.RECORDED.items()}
RECORDED["3d4_right"][1e-10] = (16, 19, 1, 1, 0)
# A confirmation is not borderline when the true residual is outside this band around the
# threshold, or when it equals the estimate's ratio to SAME relative (then a device deviation of
# 1e-10 moves both alike and the estimate has already decided).
CONFIRM_BAND = (0.99, 1.01)
SAME = 1e-6


def low_matrix(A_internal, reuse_mask=None, ns=None):
    """A^ of A (internal row and column order): every stored value rounded to nearest-even
    fp32 and promoted back, except -- with the coupling reuse -- the entries (i, j < ns) of the
    rows with reuse_mask[i], which enter the reduced product through the block PC's fp64 sums."""
    A = sp.csr_matrix(A_internal, dtype=np.float64, copy=True)
    A.sort_indices()
    data = CB.fl32(A.data)
    if reuse_mask is not None:
        mask = np.asarray(reuse_mask).astype(bool)
        assert ns is not None and mask.size == A.shape[0]
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        keep = mask[rows] & (A.indices < ns)
        data[keep] = A.data[keep]
    return sp.csr_matrix((data, A.indices.copy(), A.indptr.copy()), shape=A.shape)


def check_confirmations(name, confirms):
    """Assert that no rule (b) decision of this case is borderline."""
    for true, est in confirms:
        outside = not (CONFIRM_BAND[0] <= true <= CONFIRM_BAND[1])
        same = abs(true - est) <= SAME * abs(est)
        assert outside or same, f"bad input: a confirmation of {name} is borderline (true {true}, estimate {est})"


def gmres(ksp, b, matvec_low, orth="cgs", refine="never", flexible=False, rounding=CB.fl32, drop=1e-6,
          confirm=True):
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
    low_n = double_n = 0
    ratios = []
    confirms = []
    first = True
    confirming = False
    while True:
        if first:
            r = b.copy()
        else:
            r = b - ksp.matvec(x)
            double_n += 1
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
                confirms.append((res / conv.ttol, hist[-2] / conv.ttol))
                if not reason:
                    failed_n += 1
        confirming = False
        if reason:
            break
        if its >= ksp.maxit:
            reason = petsc.DIVERGED_ITS if normed else CB.CONVERGED_ITS
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
                w = matvec_low(z)
            else:
                w = ksp.pc.apply(matvec_low(v))
            low_n += 1
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
            reason = petsc.DIVERGED_ITS if normed else CB.CONVERGED_ITS
            break
        if forced:
            forced_n += 1
    ksp.its, ksp.reason, ksp.history = its, reason, hist
    ksp.orthog_steps = stats["steps"]
    ksp.second_passes = stats["second"]
    ksp.nearest_decision = stats["nearest"]
    ksp.cb_forced, ksp.cb_confirm, ksp.cb_failed, ksp.cb_ratios = forced_n, confirm_n, failed_n, ratios
    ksp.co_low, ksp.co_double, ksp.co_confirm = low_n, double_n, confirms
    return x
