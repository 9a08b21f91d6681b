"""numpy restatement of KSPGMRES / KSPFGMRES with PETSc's orthogonalisation
choices (a helper, not a conftest): classical Gram-Schmidt with
``-ksp_gmres_cgs_refinement_type`` refine_never / refine_ifneeded /
refine_always, and modified Gram-Schmidt.

``oracle.petsc._gmres`` (and ``ksp_restatements.fgmres``) with the
orthogonalisation step replaced.  Written, as tests/ksp_restatements.py is,
only in terms of the KSP object's ``matvec``, ``dot``, ``norm``, ``pc.apply``,
``rtol/atol/dtol/maxit/restart/pc_side`` and ``oracle.petsc.ConvergedDefault``,
so the oracle's PCs and the rank-ordered sums of ``oracle/dist.py`` carry
over.  A test installs it with

    ksp.solve = lambda b: gmres(ksp, b, orth="mgs")

The rules (PETSc's gborthog.c, restated from the published algorithm), with
k = loc_it + 1 basis vectors and w the new Krylov vector:

  mgs               for j = 0..k-1 in order: h_j = (w, v_j), w -= h_j v_j.
  cgs, never        h = V^T w, then w -= h_j v_j for j = 0..k-1.
  cgs, always       the same twice; H(j, it) = h_j + l_j (l: the second pass).
  cgs, ifneeded     a second pass exactly when ||w|| after the first is
                    smaller than sqrt(sum_j h_j^2) (summed in j order).

``gmres`` sets, besides ``ksp.its / reason / history``:
  ksp.orthog_steps        Arnoldi steps orthogonalised
  ksp.second_passes       second CGS passes performed
  ksp.nearest_decision    smallest |wnrm / hnrm - 1| over the ifneeded decisions (inf: none)
  ksp.orthogonality_loss  max |V^T V - I| over the cycles' bases (the last
                          vector of a cycle is left out when it was not normalised)
"""
import math

import numpy as np

from oracle import petsc

HAPTOL = 1e-30

# The cases of tests/test_gmres_orthog_restatement.py (CPU, recorded counts) and
# tests/test_gpu_gmres_orthog.py: BASE and BLOCKS_ILU of tests/test_gpu_ksp_types.py
# at rtol 1e-10, outer gmres never restarted unless the row says so, standard rhs.
PARAMS = {"solver type": "gmres", "solver atol": 0, "solver rtol": 1e-10, "solver maxiter": 400,
          "pc type": "diagonal", "inner ksp type": "preonly", "inner pc type": "ilu", "inner rtol": 1e-6,
          "inner atol": 0, "inner maxiter": 1000, "inner monitor": False, "solver monitor": False,
          "inner accel order": 0, "AAR order": 10, "AAR p": 5, "AAR omega": 1, "AAR beta": 1}
BLOCKS_ILU = {"s_ksp_type": "preonly", "s_pc_type": "ilu", "f_ksp_type": "preonly", "f_pc_type": "ilu",
              "p_ksp_type": "preonly", "p_pc_type": "ilu", "diff_ksp_type": "preonly", "diff_pc_type": "ilu",
              "fp_ksp_type": "preonly", "fp_pc_type": "ilu"}
# name: (dim, N, side, restart, n, its of every scheme, second passes of refine_ifneeded)
TABLE = {"2d12_left": (2, 12, "left", 400, 2669, 20, 19),
         "2d12_right": (2, 12, "right", 400, 2669, 20, 20),
         "3d4_right": (3, 4, "right", 400, 4499, 14, 13),
         "2d12_right_restart5": (2, 12, "right", 5, 2669, 61, 53)}
# option-database entries of a scheme (without the prefix) and the restatement's arguments
SCHEMES = {"mgs": ({"ksp_gmres_modifiedgramschmidt": None}, {"orth": "mgs"}),
           "refine_always": ({"ksp_gmres_cgs_refinement_type": "refine_always"}, {"refine": "always"}),
           "refine_ifneeded": ({"ksp_gmres_cgs_refinement_type": "refine_ifneeded"}, {"refine": "ifneeded"}),
           "cgs": ({}, {})}


def table_db(name, ksp_type="gmres"):
    _, _, side, restart = TABLE[name][:4]
    return dict(BLOCKS_ILU, global_ksp_type=ksp_type, global_ksp_pc_side=side, global_ksp_gmres_restart=str(restart))


def _cgs_pass(ksp, V, k, w):
    h = np.array([ksp.dot(V[j], w) for j in range(k)])
    for j in range(k):
        w = w - h[j] * V[j]
    return h, w


def orthogonalise(ksp, V, k, w, orth, refine, stats):
    """(h, w, ||w||) of one Arnoldi step against V[0..k)."""
    stats["steps"] += 1
    if orth == "mgs":
        h = np.zeros(k)
        for j in range(k):
            h[j] = ksp.dot(w, V[j])
            w = w - h[j] * V[j]
        return h, w, ksp.norm(w)
    h, w = _cgs_pass(ksp, V, k, w)
    wnrm = ksp.norm(w)
    again = refine == "always"
    if refine == "ifneeded":
        s = 0.0
        for j in range(k):
            s += h[j] * h[j]
        hnrm = math.sqrt(s)
        again = wnrm < hnrm
        if hnrm != 0.0:
            stats["nearest"] = min(stats["nearest"], abs(wnrm / hnrm - 1.0))
    if again:
        stats["second"] += 1
        l, w = _cgs_pass(ksp, V, k, w)
        h = h + l
        wnrm = ksp.norm(w)
    return h, w, wnrm


def _loss(V, m):
    if m < 1:
        return 0.0
    B = np.array(V[:m])
    return float(np.max(np.abs(B @ B.T - np.eye(m))))


def gmres(ksp, b, orth="cgs", refine="never", flexible=False):
    """KSPGMRES (side ``ksp.pc_side``) or, with flexible, KSPFGMRES (right, the
    preconditioned vectors kept, x += Z y)."""
    assert orth in ("cgs", "mgs") and refine in ("never", "ifneeded", "always")
    b = np.asarray(b, dtype=np.float64)
    n = b.size
    x = np.zeros(n)
    conv = petsc.ConvergedDefault(ksp.rtol, ksp.atol, ksp.dtol)
    right = flexible or ksp.pc_side == "right"
    max_k = ksp.restart
    its = 0
    reason = 0
    hist = []
    stats = {"steps": 0, "second": 0, "nearest": math.inf}
    loss = 0.0
    first = True
    while not reason:
        r = b.copy() if first else b - ksp.matvec(x)
        if not right:
            r = ksp.pc.apply(r)
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
        normalised = 1
        while not reason and loc_it < max_k and its < ksp.maxit:
            v = V[loc_it]
            if right:
                z = ksp.pc.apply(v)
                if flexible:
                    Z.append(z)
                w = ksp.matvec(z)
            else:
                w = ksp.pc.apply(ksp.matvec(v))
            h, w, tt = orthogonalise(ksp, V, loc_it + 1, w, orth, refine, stats)
            HH[:loc_it + 1, loc_it] = h
            HH[loc_it + 1, loc_it] = tt
            hapbnd = min(abs(tt / grs[loc_it]), HAPTOL)
            hapend = tt < hapbnd
            if not hapend:
                with np.errstate(divide="ignore"):
                    inv = np.float64(1.0) / np.float64(tt)
                with np.errstate(invalid="ignore", over="ignore"):
                    w = w * inv
                normalised = loc_it + 2
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
        loss = max(loss, _loss(V, normalised))
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
                B = Z if flexible else V
                for j in range(it + 1):
                    tmp = tmp + nrs[j] * B[j]
                if right and not flexible:
                    tmp = ksp.pc.apply(tmp)
                x = x + tmp
        if its >= ksp.maxit:
            if not reason:
                reason = petsc.DIVERGED_ITS
            break
        first = False
    ksp.its, ksp.reason, ksp.history = its, reason, hist
    ksp.orthog_steps = stats["steps"]
    ksp.second_passes = stats["second"]
    ksp.nearest_decision = stats["nearest"]
    ksp.orthogonality_loss = loss
    return x
