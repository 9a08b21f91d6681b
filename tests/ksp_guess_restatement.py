"""numpy restatement of KSPSolve with an initial guess (a helper, not a conftest):
``-global_ksp_initial_guess_nonzero`` and ``-<prefix>ksp_guess_type fischer``
(PETSc's KSPGuess, Fischer's model 2: the least-squares projection, valid for a
nonsymmetric operator).

Written, as tests/cb_gmres_restatement.py is, only in terms of ``ksp.matvec /
dot / norm / pc.apply`` and ``oracle.petsc.ConvergedDefault``, so the oracle's
PCs and the rank-ordered sums of ``oracle/dist.py`` carry over.  A test installs
it with

    guess = Fischer2(ksp, size=4)
    ksp.solve = lambda b: guessed_solve(ksp, b, None, inner, guess=guess)

where ``inner(ksp, rhs)`` is any zero-guess solve (``oracle.petsc._gmres``,
``gmres_orthog_restatement.gmres``, ``ksp_restatements.bcgs`` ...).

The rules:

  guess      x0 = guess.form(b) when a guess object exists, else the x0 given.
  form       the solve is the zero-guess solve of A d = r0, r0 = b - A x0, and
             x = x0 + d.  A restart of the inner solve evaluates r0 - A d, which
             is b - A x to rounding.
  rnorm0     KSPConvergedDefault at iteration 0 takes rnorm0 = ||b|| (right
             preconditioning or norm unpreconditioned: rule "b") or ||B b|| (the
             preconditioned norm: rule "Bb", one more PC application) instead of
             the first residual norm; where that value is 0, and with rule
             "zero", the first residual norm stays.  ttol and the dtol test use
             it.  Norm type none needs none (rule "none").
  Fischer2   columns X[i], B[i] = A X[i], the B[i] orthonormal.
             form(b):   alpha_i = (B[i], b), x0 = sum_i alpha_i X[i], i ascending.
             update(x): nothing when x holds NaN or Inf; a full space is emptied
                        first (a reset); y = A x, nu0 = ||y||, alpha_i = (B[i], y),
                        x' = x - sum alpha_i X[i], y' = y - sum alpha_i B[i] (i
                        ascending), nu = ||y'||; (x', y') (1 / nu) appended when
                        nu > tol nu0 and nu > 0, else a skipped update.
             Additions to that, all about rounding:
             the projection runs twice (beta_i = (B[i], y'), x' -= beta_i X[i],
             y' -= beta_i B[i]) -- one pass leaves B^T y' at eps nu0 / nu, and the
             solutions of a time loop differ by 1e-3 .. 1e-6 -- and a solve that made
             no iteration (x is the guess, a combination of the columns: nu = 0 in
             exact arithmetic, rounding noise above tol when computed) counts as
             skipped, unless the space is full and about to be emptied.  A third:
             where nu < REFORM nu0 the new column of B is formed again as the product
             A x', projected once more and normalised again (y = A x carries a
             rounding of eps nu0, which is eps nu0 / nu of the normalised column).

``guessed_solve`` sets, besides what ``inner`` sets (``ksp.its / reason /
history``): ``ksp.guess_reduction`` = ||r0|| / ||b||, ``ksp.guess_rnorm0`` (None:
the first residual's) and ``ksp.guess_ttol``.
"""
import math

import numpy as np

from oracle import petsc

DBL_EPSILON = 2.220446049250313e-16
DEFAULT_SIZE = 10
DEFAULT_TOL = 32 * DBL_EPSILON
REFORM = 1e-2  # nu / nu0 below which the new column of B is formed again as A x' (see Fischer2.update)


def rnorm0_rule(ksp, flexible=False, right=None):
    """The rule of a gmres / cg oracle KSP (other types: say it yourself)."""
    norm_type = getattr(ksp, "norm_type", None)
    if norm_type == "none":
        return "none"
    if flexible or right or (right is None and ksp.pc_side == "right") or norm_type == "unpreconditioned":
        return "b"
    return "Bb"


class _Forced:
    """The next ``petsc.ConvergedDefault`` that is made takes rnorm0 = value at
    n == 0 (only that one: a PC's inner solves make their own afterwards)."""

    def __init__(self, value):
        self.value, self.orig, self.made = value, petsc.ConvergedDefault, None

    def __enter__(self):
        orig, value, me = self.orig, self.value, self

        class Forced(orig):
            def __call__(self, n, rnorm):
                if n == 0 and value is not None:
                    self.rnorm0 = value
                    self.ttol = max(self.rtol * self.rnorm0, self.atol)
                    return orig.__call__(self, 1, rnorm)  # the tests alone
                return orig.__call__(self, n, rnorm)

        def make(*a, **kw):
            petsc.ConvergedDefault = orig
            me.made = Forced(*a, **kw)
            return me.made

        petsc.ConvergedDefault = make
        return self

    def __exit__(self, *exc):
        petsc.ConvergedDefault = self.orig
        return False


def guessed_solve(ksp, b, x0, inner, guess=None, rule=None):
    b = np.asarray(b, dtype=np.float64)
    rule = rnorm0_rule(ksp) if rule is None else rule
    assert rule in ("b", "Bb", "none", "zero")
    if guess is not None:
        x0 = guess.form(b)
    x0 = np.asarray(x0, dtype=np.float64)
    r0 = b - ksp.matvec(x0)
    bn = ksp.norm(b)
    rn0 = None
    if rule == "b":
        rn0 = bn
    elif rule == "Bb":
        rn0 = ksp.norm(ksp.pc.apply(b))
    if rn0 is not None and not rn0 > 0.0:
        rn0 = None
    with np.errstate(divide="ignore", invalid="ignore"):
        ksp.guess_reduction = float(np.float64(ksp.norm(r0)) / np.float64(bn))
    ksp.guess_rnorm0 = rn0
    with _Forced(rn0) as f:
        d = inner(ksp, r0)
    ksp.guess_ttol = f.made.ttol if f.made is not None else None
    x = x0 + d
    if guess is not None:
        guess.update(x, untouched=ksp.its == 0)
    return x


class Fischer2:
    def __init__(self, ksp, size=DEFAULT_SIZE, tol=DEFAULT_TOL):
        assert 1 <= size <= 64
        self.ksp, self.size, self.tol = ksp, int(size), tol
        self.X, self.B = [], []
        self.formed = self.skipped = self.resets = self.reformed = 0

    @property
    def m(self):
        return len(self.X)

    def stats(self):
        """What pls_get_ksp_guess_stats reports."""
        return (1, self.m, self.size, self.formed, self.skipped, self.resets)

    def reset(self):
        self.X, self.B = [], []
        self.resets += 1

    def form(self, b):
        self.formed += 1
        alpha = [self.ksp.dot(self.B[i], b) for i in range(self.m)]
        x0 = np.zeros(b.size)
        for i in range(self.m):
            x0 = x0 + alpha[i] * self.X[i]
        return x0

    def update(self, x, untouched=False):
        k = self.ksp
        if not np.all(np.isfinite(x)):
            return
        if untouched and 0 < self.m < self.size:
            # the solve made no iteration: x is the guess, a combination of the stored columns, and
            # nu is 0 in exact arithmetic.  Computed, it is rounding noise that can pass tol.
            self.skipped += 1
            return
        if self.m == self.size:
            self.reset()
        y = k.matvec(x)
        nu0 = k.norm(y)
        alpha = [k.dot(self.B[i], y) for i in range(self.m)]
        xp, yp = np.array(x, dtype=np.float64), y
        for i in range(self.m):
            xp = xp - alpha[i] * self.X[i]
            yp = yp - alpha[i] * self.B[i]
        if self.m:  # the projection again: one pass leaves B^T y' at eps nu0 / nu
            beta = [k.dot(self.B[i], yp) for i in range(self.m)]
            for i in range(self.m):
                xp = xp - beta[i] * self.X[i]
                yp = yp - beta[i] * self.B[i]
        nu = k.norm(yp)
        if not (math.isfinite(nu0) and math.isfinite(nu)):
            return
        if nu > self.tol * nu0 and nu > 0.0:
            inv = 1.0 / nu
            xp, yp = xp * inv, yp * inv
            if nu < REFORM * nu0:
                # y' carries the rounding of y = A x, eps nu0, which is eps nu0 / nu of the normalised
                # column: B's column is formed again as a product, projected once more (the new y' is
                # orthogonal to eps nu0 / nu only) and normalised again
                self.reformed += 1
                yp = k.matvec(xp)
                beta = [k.dot(self.B[i], yp) for i in range(self.m)]
                for i in range(self.m):
                    xp = xp - beta[i] * self.X[i]
                    yp = yp - beta[i] * self.B[i]
                inv = 1.0 / k.norm(yp)
                xp, yp = xp * inv, yp * inv
            self.X.append(xp)
            self.B.append(yp)
        else:
            self.skipped += 1


# ------------------------------------------------------------ the sequence ----
def sequence_rhs(A, b0, t, x_prev, g=None):
    """b_t = b0 (1 + 0.5 sin 0.3t) + 0.2 cos(0.2t) s g1 + 0.05 t s g2 + 0.3 |diag A| . x_{t-1},
    g1, g2 = default_rng(0).standard_normal(n) twice, s = mean |b0|, x_{-1} = 0."""
    n = b0.size
    if g is None:
        rng = np.random.default_rng(0)
        g = (rng.standard_normal(n), rng.standard_normal(n))
    s = float(np.mean(np.abs(b0)))
    return (b0 * (1 + 0.5 * math.sin(0.3 * t)) + 0.2 * math.cos(0.2 * t) * s * g[0] + 0.05 * t * s * g[1]
            + 0.3 * np.abs(A.diagonal()) * x_prev)


def run_sequence(ksp, A, b0, steps, solve):
    """solve(b) over the sequence; per step (b, x, its, reason, history, ttol)."""
    rng = np.random.default_rng(0)
    g = (rng.standard_normal(b0.size), rng.standard_normal(b0.size))
    x = np.zeros(b0.size)
    out = []
    for t in range(steps):
        b = sequence_rhs(A, b0, t, x, g)
        x = solve(b)
        out.append({"b": b, "x": x, "its": ksp.its, "reason": ksp.reason, "history": list(ksp.history),
                    "ttol": getattr(ksp, "guess_ttol", None), "reduction": getattr(ksp, "guess_reduction", None)})
    return out


def margin(history, ttol):
    """min |res / ttol - 1| over the last estimate above ttol and the first at or below it."""
    h = np.asarray(history, dtype=np.float64)
    below = np.nonzero(h <= ttol)[0]
    picks = []
    if below.size:
        picks.append(h[below[0]])
        if below[0] > 0:
            picks.append(h[below[0] - 1])
    elif h.size:
        picks.append(h[-1])
    return min(abs(p / ttol - 1.0) for p in picks) if picks else math.inf


BAND = 1e-2
# The cases of gmres_orthog_restatement.TABLE at rtol 1e-6 with blocks ILU, Fischer size 4:
# name -> (steps, iterations per step with the Fischer guess, ... from a zero guess, the guess's
# counters after the last step), measured on the CPU: totals 93 / 182, 35 / 131,
# 91 / 182; the previous solution alone as the guess gives 181, 131, 181.  The 2-D cases empty
# the space twice.  The 3-D right-hand sides stay in the span of the first fill: from step 4 on
# every solve starts converged, nothing is added and the space is emptied once.  No case had to
# be shortened: no step decides within BAND of ttol.
RECORDED = {"2d12_right": (12, [16, 15, 15, 13, 12, 11, 6, 1, 0, 4, 0, 0], [16, 16] + [15] * 10, (1, 2, 4, 12, 2, 2)),
            "3d4_right": (12, [10, 11, 10, 4, 0, 0, 0, 0, 0, 0, 0, 0], [10] + [11] * 11, (1, 1, 4, 12, 7, 1)),
            "2d12_left": (12, [16, 15, 15, 13, 12, 10, 6, 1, 0, 3, 0, 0], [16, 16] + [15] * 10, (1, 2, 4, 12, 2, 2))}
SEQ_RTOL = 1e-6
SEQ_SIZE = 4
