"""BoomerAMG relax types Jacobi, l1scaled-Jacobi and Chebyshev, restated (TEST
INFRASTRUCTURE ONLY): the specification of ``-<prefix>pc_hypre_boomeramg_relax_type_all``
that csrc/boomeramg.cpp follows and the GPU tests compare with.  Parity against
hypre is unpinned, as for the rest of the AMG (oracle/boomeramg.py).

``PCBoomerAMGRelax`` is ``oracle.boomeramg.PCBoomerAMG`` with ``_relax``
overridden; hierarchy, coarse solve and V-cycle are the oracle's.  Tests install
it with ``install()`` (oracle/petsc.py imports the class at call time).

On a level with operator A and diagonal d:
* ``symmetric-SOR/Jacobi`` (default): the oracle's ``_relax``, untouched.
* ``Jacobi``: m_i = w / d_i, w = ``relax_weight_all`` (default 1.0).
* ``l1scaled-Jacobi``: m_i = sign(d_i) / sum_j |a_ij| over the stored entries
  of row i (storage order, the diagonal included).
  For both a zero d_i (or a zero row sum) gives m_i = 1.  A sweep over a set I
  (all rows with no_CF; else C then F going down, F then C going up) is
  x <- x + M_I (b - A x), M_I = diag(m_i for i in I, 0 elsewhere);
  grid_sweeps_all K: K rounds over the sets.
* ``Chebyshev``: one set of all rows.  Each of the K rounds starts the
  recurrence of oracle/amg.py ``PCAMG._cheb`` again and runs ``order`` steps of
  it: dinv = 1 / d (1 where d = 0), lambda = float32(power_lambda(A, dinv, 15)),
  lmax = 1.1 lambda, lmin = fraction lmax, theta = (lmax + lmin) / 2,
  delta = (lmax - lmin) / 2, sigma = theta / delta, rho = 1 / sigma,
  d = (1 / theta) (dinv r); then x += d and, before every further step,
  rho' = 1 / (2 sigma - rho), d = (rho' rho) d + (2 rho' / delta) (dinv r),
  with r = b - A x formed from the current x before each step.
  ``pls_boomeramg_chebyshev_order`` 1..4 (default 2),
  ``pls_boomeramg_chebyshev_fraction`` in (0, 1) (default 0.3).
Every step is x_new = x + dn, dn = a d + g (m (b - A x)) with the a d term
absent (not multiplied by zero) where the rules above have none; g (m r) is
two rounded products in that order.
"""
from __future__ import annotations

import numpy as np

import oracle.boomeramg as OB
from oracle.amg import power_lambda
from oracle.options import get as opt

RELAX_TYPES = ("symmetric-SOR/Jacobi", "Jacobi", "l1scaled-Jacobi", "Chebyshev")


def jacobi_dinv(A):
    d = A.diagonal().astype(np.float64)
    return np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 1.0)


def jacobi_m(A, w):
    d = A.diagonal().astype(np.float64)
    return np.where(d != 0.0, w / np.where(d != 0.0, d, 1.0), 1.0)


def l1_m(A):
    A = A.tocsr()
    d = A.diagonal().astype(np.float64)
    n = A.shape[0]
    s = np.zeros(n)
    rp, v = A.indptr, A.data
    for i in range(n):
        acc = 0.0
        for a in v[rp[i]:rp[i + 1]].tolist():
            acc += abs(a)
        s[i] = acc
    ok = (d != 0.0) & (s != 0.0)
    return np.where(ok, np.sign(d) / np.where(ok, s, 1.0), 1.0)


class PCBoomerAMGRelax(OB.PCBoomerAMG):
    def __init__(self, A, db=None, prefix=""):
        db = db or {}
        pre = prefix + "pc_hypre_boomeramg_"
        self.relax_type = opt(db, prefix, "pc_hypre_boomeramg_relax_type_all", RELAX_TYPES[0], str)
        if self.relax_type not in RELAX_TYPES:
            raise NotImplementedError(f"{pre}relax_type_all {self.relax_type}: one of {', '.join(RELAX_TYPES)}")
        try:
            self.weight = float(opt(db, prefix, "pc_hypre_boomeramg_relax_weight_all", 1.0, str))
        except ValueError:
            raise ValueError(f"{pre}relax_weight_all must be a number")
        self.order = opt(db, prefix, "pls_boomeramg_chebyshev_order", 2, int)
        self.fraction = opt(db, prefix, "pls_boomeramg_chebyshev_fraction", 0.3, float)
        if not 1 <= self.order <= 4:
            raise ValueError(f"{prefix}pls_boomeramg_chebyshev_order must be 1, 2, 3 or 4")
        if not 0.0 < self.fraction < 1.0:
            raise ValueError(f"{prefix}pls_boomeramg_chebyshev_fraction must lie in (0, 1)")
        super().__init__(A, db, prefix)

    def lambdas(self):
        """The levels' eigenvalue estimates (0 for the other types)."""
        return [self._cheb_data(L)[1] if self.relax_type == "Chebyshev" else 0.0 for L in self.levels]

    def _cheb_data(self, L):
        if "cheb" not in L:
            dinv = jacobi_dinv(L["A"])
            L["cheb"] = (dinv, float(np.float32(power_lambda(L["A"], dinv, 15))))
        return L["cheb"]

    def _m_sets(self, L):
        """Per set name ("all" or "C" / "F"): the full-length vector m, zero off the set."""
        if "m" not in L:
            A = L["A"]
            m = jacobi_m(A, self.weight) if self.relax_type == "Jacobi" else l1_m(A)
            if self.no_cf:
                L["m"] = {"all": (A.shape[0], m)}
            else:
                L["m"] = {}
                for o in "CF":
                    mask = L["cf"] == (OB.C if o == "C" else OB.F)
                    L["m"][o] = (int(mask.sum()), np.where(mask, m, 0.0))
        return L["m"]

    def _relax(self, L, b, x, order):
        if self.relax_type == RELAX_TYPES[0]:
            return super()._relax(L, b, x, order)
        A = L["A"]
        if self.relax_type == "Chebyshev":
            dinv, lam = self._cheb_data(L)
            lmax = 1.1 * lam
            lmin = self.fraction * lmax
            theta, delta = (lmax + lmin) / 2.0, (lmax - lmin) / 2.0
            sigma = theta / delta
            for _ in range(self.K):
                rho = 1.0 / sigma
                d = (1.0 / theta) * (dinv * (b - A @ x))
                x = x + d
                for _k in range(1, self.order):
                    rho_n = 1.0 / (2.0 * sigma - rho)
                    d = (rho_n * rho) * d + (2.0 * rho_n / delta) * (dinv * (b - A @ x))
                    x = x + d
                    rho = rho_n
            return x
        ms = self._m_sets(L)
        sets = [ms["all"]] if self.no_cf else [ms[o] for o in order]
        for _ in range(self.K):
            for cnt, m in sets:
                if cnt == 0:
                    continue
                x = x + m * (b - A @ x)
        return x


def install():
    """Make oracle.petsc build this class for -pc_type hypre; returns the class it replaces."""
    old = OB.PCBoomerAMG
    OB.PCBoomerAMG = PCBoomerAMGRelax
    return old


def uninstall(old):
    OB.PCBoomerAMG = old
