"""The initial guess on the device -- ``-global_ksp_initial_guess_nonzero`` and
``-<prefix>ksp_guess_type fischer`` (Fischer's model 2) -- against the numpy
restatement (tests/ksp_guess_restatement.py, pinned on the CPU by
tests/test_ksp_guess_restatement.py) installed in ``OracleSolver``.

Tolerances, the project's rule (tests/test_gpu_ksp_types.py) applied per step of
a sequence of solves: iteration count, reason and history length exact; every
history entry within max(1e-10, 10 x the restatement's own worst deviation up
to that step over 4 seeds, when every inner PC output and every stored column
is perturbed by 1e-15 relative); the solution within max(1e-8, 10 x its own
deviation, measured the same way) relative.  Up to that step, not at it: a deviation lives on in the stored
columns, so two runs that differ at step t still differ afterwards, and four
seeds estimate a single step's figure only to a factor of ten (the existing
tests take the worst over a whole solve for the same reason).  A restatement whose iteration count moves with the seed is a bad
input.  Every step's right-hand side is formed from the restatement's previous
solution, so both sides solve the same systems.

Row counts (the ones of tests/test_gpu_cb_gmres.py) and what they exercise in
k_guess_update, which takes two rows per lane and two pairs per trip, 1,024
rows per trip and block: 2,669 (one block; two full trips, a tail loop, the odd
last row), 4,499 (two blocks of 2,250: odd n, even chunks), the s block of 2-D
N=32 3-way 8,450 (three reduction chunks of 2,818, 2,818 and 2,814 rows) and
its p block 1,089 (below two trips: the single-pair loop and the odd row).
"""
import numpy as np
import pytest

import gmres_orthog_restatement as G
import ksp_guess_restatement as R
import test_gpu_ksp_types as K
from oracle import petsc
from oracle import synthetic as S
from oracle.solver import OracleSolver

pytestmark = pytest.mark.gpu

PARAMS = dict(G.PARAMS, **{"solver rtol": R.SEQ_RTOL})


def fischer(size, prefix="global_"):
    return {prefix + "ksp_guess_type": "fischer", prefix + "ksp_guess_fischer_model": f"2,{size}"}


def _oracle(spec, params, db):
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    odb = {k: v for k, v in db.items() if "ksp_guess" not in k and "initial_guess" not in k}
    return A, OracleSolver(A, P, Pd, is_s, is_f, is_p, params, odb, S.bcs_sub_pressure(spec))


class Perturbed(R.Fischer2):
    """Fischer2 whose stored columns take a 1e-15 relative perturbation (rng set)."""
    rng = None

    def update(self, x, untouched=False):
        before = (self.m, self.resets)
        super().update(x, untouched)
        if self.rng is not None and self.m and (self.m, self.resets) != before:
            for cols in (self.X, self.B):
                cols[-1] = cols[-1] * (1 + 1e-15 * self.rng.standard_normal(x.size))


def _perturb_pcs(o, rng, eps=1e-15):
    saved = []
    for name in K.INNER:
        ksp = getattr(o.block_pc, name, None)
        if ksp is None:
            continue
        orig = ksp.pc.apply
        saved.append((ksp.pc, orig))
        ksp.pc.apply = (lambda f: lambda x: (lambda y: y * (1 + eps * rng.standard_normal(y.size)))(f(x)))(orig)
    return saved


def _sequence(o, A, b0, steps, make_guess, inner, rule=None, bs=None, seed=None):
    """The restatement over the sequence (bs given: over those right-hand sides)."""
    k = o.solver
    g = make_guess(k)
    saved = []
    if seed is not None:
        g.rng = np.random.default_rng(seed)
        saved = _perturb_pcs(o, g.rng)
    solve = lambda b: R.guessed_solve(k, b, None, inner, guess=g, rule=rule)  # noqa: E731
    try:
        if bs is None:
            out = R.run_sequence(k, A, b0, steps, solve)
        else:
            out = []
            for b in bs:
                x = solve(b)
                out.append({"b": b, "x": x, "its": k.its, "reason": k.reason, "history": list(k.history),
                            "ttol": k.guess_ttol, "reduction": k.guess_reduction})
    finally:
        for pc, orig in saved:
            pc.apply = orig
    return out, g


def _rel(h, ho):
    h, ho = np.asarray(h, dtype=np.float64), np.asarray(ho, dtype=np.float64)
    ok = ho > 0
    return float(np.max(np.abs(h[ok] - ho[ok]) / ho[ok])) if np.any(ok) else 0.0


def _reference(spec, params, db, steps, size, inner=petsc._gmres, rule=None, tol=R.DEFAULT_TOL, seeds=4):
    A, o = _oracle(spec, params, db)
    b0 = S.rhs(spec)
    make = lambda k: Perturbed(k, size=size, tol=tol)  # noqa: E731
    base, g = _sequence(o, A, b0, steps, make, inner, rule)
    bs = [s["b"] for s in base]
    floor, xfloor = np.zeros(steps), np.zeros(steps)
    for seed in range(seeds):
        other, g2 = _sequence(o, A, b0, steps, make, inner, rule, bs=bs, seed=seed)
        assert g2.stats() == g.stats(), f"bad input: counters {g2.stats()} with seed {seed}, {g.stats()} without"
        for t, (a, c) in enumerate(zip(base, other)):
            assert a["its"] == c["its"] and a["reason"] == c["reason"], \
                f"bad input: step {t} takes {c['its']} iterations with seed {seed}, {a['its']} without"
            floor[t] = max(floor[t], _rel(c["history"], a["history"]))
            xfloor[t] = max(xfloor[t], float(np.linalg.norm(c["x"] - a["x"]) / np.linalg.norm(a["x"])))
    for t, s in enumerate(base):
        m = R.margin(s["history"], s["ttol"])
        assert m >= R.BAND, f"bad input: step {t} decides within {m:.3e} of ttol"
    print("restatement: its", [s["its"] for s in base], "stats", g.stats())
    print("floors", " ".join(f"{v:.1e}" for v in floor))
    return {"A": A, "o": o, "base": base, "bs": bs, "guess": g,
            "floor": np.maximum.accumulate(floor), "xfloor": np.maximum.accumulate(xfloor)}


def _hold(h, ref, prefix="global_"):
    """The device over the restatement's right-hand sides, step by step."""
    xs = []
    for t, (s, b) in enumerate(zip(ref["base"], ref["bs"])):
        x, r = h.solve(b)
        hist = h.history()
        tol, xtol = max(1e-10, 10 * ref["floor"][t]), max(1e-8, 10 * ref["xfloor"][t])
        ho = np.asarray(s["history"])
        rel = _rel(hist, ho) if hist.shape == ho.shape else np.inf
        xerr = float(np.linalg.norm(x - s["x"]) / np.linalg.norm(s["x"]))
        print(f"step {t}: its {r.its} ({s['its']}) reason {r.reason} ({s['reason']}) entries {hist.size} ({ho.size}) "
              f"history {rel:.2e} (tol {tol:.1e}) x {xerr:.2e} (tol {xtol:.1e})")
        assert r.its == s["its"], f"step {t}: its {r.its} vs restatement {s['its']}"
        assert r.reason == s["reason"] and hist.shape == ho.shape
        assert rel <= tol, f"step {t}: residual history rel diff {rel:.3e} (tol {tol:.1e})"
        assert xerr <= xtol
        xs.append(x)
    st, red = h.ksp_guess_stats(prefix)
    print("ksp_guess_stats", st, red)
    assert st == ref["guess"].stats()
    return xs, st, red


# --------------------------- 1. the whole sequence, the table's three cases ----
@pytest.mark.parametrize("name", ["2d12_right", "3d4_right", "2d12_left"])
def test_sequence_of_the_table_cases(gpu, name):
    dim, N, side, restart, n = G.TABLE[name][:5]
    spec = S.SynthSpec(dim, N)
    assert spec.n == n
    steps, want, _, want_stats = R.RECORDED[name]
    db = dict(G.table_db(name), **fischer(R.SEQ_SIZE))
    ref = _reference(spec, PARAMS, db, steps, R.SEQ_SIZE)
    assert [s["its"] for s in ref["base"]] == want and ref["guess"].stats() == want_stats
    h = K._handle(spec, PARAMS, db)
    assert np.isnan(_first_stats(h)[1])
    xs, st, red = _hold(h, ref)
    want_red = ref["base"][-1]["reduction"]
    print(f"last reduction {red:.6e} (restatement {want_red:.6e})")
    assert abs(red - want_red) <= max(1e-10, 10 * ref["floor"][-1]) * want_red
    if side == "right":  # the first entry is ||b - A x0||, the last the residual of x = x0 + d
        b, x = ref["bs"][-1], xs[-1]
        true = np.linalg.norm(b - h.matmult(x))
        assert true <= PARAMS["solver rtol"] * np.linalg.norm(b) * (1 + 1e-6)
    assert h.ksp_stats("global_")[:2] == (steps, sum(want))  # every solve counted once, with its own iterations


def _first_stats(h):
    h.create_solver()
    return h.ksp_guess_stats("global_")


def test_size_one_resets_at_every_update(gpu):
    spec = S.SynthSpec(2, 12)
    db = dict(G.table_db("2d12_right"), **fischer(1))
    ref = _reference(spec, PARAMS, db, 6, 1)
    assert ref["guess"].stats() == (1, 1, 1, 6, 0, 5)
    _hold(K._handle(spec, PARAMS, db), ref)


def test_default_model_is_2_with_10_columns(gpu):
    spec = S.SynthSpec(2, 4)
    h = K._handle(spec, PARAMS, dict(G.table_db("2d12_right"), global_ksp_guess_type="fischer"))
    h.solve(S.rhs(spec))
    assert h.ksp_guess_stats("global_")[0] == (1, 1, 10, 1, 0, 0)
    h0 = K._handle(spec, PARAMS, G.table_db("2d12_right"))
    h0.solve(S.rhs(spec))
    st, red = h0.ksp_guess_stats("global_")
    assert st == (0, 0, 0, 0, 0, 0) and np.isnan(red)


# --------------------------------------- 2. every outer type, six steps ----
# Each type against its own zero-guess solve of A d = r0 under the rnorm0 rule, through handles of
# the same configuration: a host copy of the space (Fischer2 over the device's own products and
# solutions) gives x0, and a plain handle whose rtol is scaled by rnorm0 / (the first residual
# norm) -- the same ttol -- solves for d.
# cg: the synthetic A is symmetric positive definite, and so is the 3-way diagonal PC with ILU(0) blocks
THREE_WAY = dict(PARAMS, **{"pc type": "diagonal 3-way"})
TYPES = {
    "gmres_left": (dict(global_ksp_type="gmres", global_ksp_pc_side="left"), "Bb"),
    "gmres_right": (dict(global_ksp_type="gmres", global_ksp_pc_side="right"), "b"),
    "fgmres": (dict(global_ksp_type="fgmres", global_ksp_gmres_restart="300"), "b"),
    "bcgs": (dict(global_ksp_type="bcgs"), "Bb"),
    "bcgs_right": (dict(global_ksp_type="bcgs", global_ksp_pc_side="right"), "b"),
    "richardson": (dict(global_ksp_type="richardson", global_ksp_max_it="60", global_ksp_rtol="1e-2"), "Bb"),
    "chebyshev": (dict(global_ksp_type="chebyshev", global_ksp_chebyshev_eigenvalues="0.1,1.2", global_ksp_max_it="60",
                       global_ksp_rtol="1e-2"), "Bb"),
    "cg": (dict(global_ksp_type="cg"), "Bb", THREE_WAY),
    "cg_unpreconditioned_norm": (dict(global_ksp_type="cg", global_ksp_norm_type="unpreconditioned"), "b", THREE_WAY),
}


class _HostKsp:
    """What Fischer2 needs of a KSP, over a handle's own product."""

    def __init__(self, h):
        self.matvec, self.dot, self.norm = h.matmult, (lambda a, b: float(np.dot(a, b))), \
            (lambda a: float(np.linalg.norm(a)))


def _own_zero_guess(spec, params, db, rule, steps=6, size=2, fp32=False):
    kind_converges = db.get("global_ksp_type") == "cg"
    rtol = float(db.get("global_ksp_rtol", params["solver rtol"]))
    hf = K._handle(spec, params, dict(db, **fischer(size)))
    A = S.matrix(spec, 0)
    shadow = R.Fischer2(_HostKsp(hf), size=size)
    shadow.ksp.its = 1
    b0 = S.rhs(spec)
    rng = np.random.default_rng(0)
    g = (rng.standard_normal(spec.n), rng.standard_normal(spec.n))
    x = np.zeros(spec.n)
    total = 0
    for t in range(steps):
        b = R.sequence_rhs(A, b0, t, x, g)
        x, r = hf.solve(b)
        hist = hf.history()
        x0 = shadow.form(b)
        r0 = b - hf.matmult(x0)
        first = np.linalg.norm(hf.pc_apply(r0)) if rule == "Bb" else np.linalg.norm(r0)
        rn0 = np.linalg.norm(hf.pc_apply(b)) if rule == "Bb" else np.linalg.norm(b)
        assert abs(hist[0] - first) <= 1e-8 * first, f"step {t}: first entry {hist[0]:.6e}, ||r0|| {first:.6e}"
        assert abs(hf.ksp_guess_stats("global_")[1] - np.linalg.norm(r0) / np.linalg.norm(b)) <= 1e-8
        hz = K._handle(spec, params, dict(db, global_ksp_rtol=repr(float(rtol * rn0 / first))))
        d, rz = hz.solve(r0)
        hz_hist = hz.history()
        xerr = np.linalg.norm(x - (x0 + d)) / np.linalg.norm(x)
        print(f"step {t}: its {r.its} ({rz.its}) reason {r.reason} ({rz.reason}) history "
              f"{_rel(hist, hz_hist) if hist.shape == hz_hist.shape else np.inf:.2e} x {xerr:.2e}")
        assert (r.its, r.reason) == (rz.its, rz.reason) and hist.shape == hz_hist.shape
        # the decision against a ttol computed here: rtol x (||b|| or ||B b||), whatever r0 was
        ttol = max(rtol * rn0, float(params["solver atol"]))
        if not fp32:  # (there the entry before a confirmation is the estimate that met ttol)
            assert np.all(hist[:-1] > ttol * (1 - 1e-8)), f"step {t}: an entry before the last is below ttol {ttol:.6e}"
        assert (hist[-1] <= ttol * (1 + 1e-8)) == (r.reason in (2, 3)), f"step {t}: last entry {hist[-1]:.6e}, ttol {ttol:.6e}"
        if kind_converges:
            assert r.reason == 2
        if fp32:  # a basis entry may round the other way: one fp32 ulp of the cycle's first residual
            assert np.max(np.abs(hist - hz_hist)) <= 2.0 ** -24 * hist[0]
        else:  # (x0 is the host copy's here and the device's there: the deviations of section 1, 5e-10 at most)
            assert _rel(hist, hz_hist) <= 1e-8
        assert xerr <= 1e-8
        shadow.update(x, untouched=r.its == 0)
        assert hf.ksp_guess_stats("global_")[0] == shadow.stats()
        total += r.its
    return total


@pytest.mark.parametrize("kind", list(TYPES))
def test_every_outer_type_against_its_own_zero_guess_solve(gpu, kind):
    extra, rule, params = (TYPES[kind] + (PARAMS,))[:3]
    spec = S.SynthSpec(2, 12)
    total = _own_zero_guess(spec, params, dict(G.BLOCKS_ILU, **extra), rule)
    if kind.startswith("cg"):
        assert total > 30  # it converged by iterating (reason 2 at every step, asserted in _own_zero_guess)


# ------------------------------------------------- 3. compressed basis ----
def test_fp32_basis_with_the_fischer_guess(gpu):
    """pls_gmres_basis single: the confirmations evaluate r0 - A d; its own zero-guess solve again."""
    spec = S.SynthSpec(2, 12)
    db = dict(G.BLOCKS_ILU, global_ksp_type="gmres", global_ksp_pc_side="right", global_pls_gmres_basis="single")
    _own_zero_guess(spec, PARAMS, db, "b", fp32=True)


# ------------------------------------------ 4. initial_guess_nonzero alone ----
def test_previous_solution_of_the_same_rhs_takes_no_iteration(gpu):
    spec = S.SynthSpec(2, 12)
    db = dict(G.table_db("2d12_right"), global_ksp_initial_guess_nonzero="true")
    h = K._handle(spec, PARAMS, db)
    b = S.rhs(spec)
    x1, r1 = h.solve(b)
    assert r1.its == 16 and r1.reason == 2  # no x0: a zero guess
    x2, r2 = h.solve(b, x0=x1)
    hist = h.history()
    assert (r2.its, r2.reason, hist.size) == (0, 2, 1)
    assert np.array_equal(x2, x1)
    assert hist[0] <= 1e-6 * np.linalg.norm(b)
    st, red = h.ksp_guess_stats("global_")
    assert st == (0, 0, 0, 0, 0, 0) and abs(red - hist[0] / np.linalg.norm(b)) <= 1e-12 * red
    assert h.ksp_stats("global_")[:2] == (2, 16)
    plain = K._handle(spec, PARAMS, G.table_db("2d12_right"))
    with pytest.raises(ValueError, match="global_ksp_initial_guess_nonzero is not set"):
        plain.solve(b, x0=x1)
    x3, r3 = plain.solve(b)
    assert r3.its == 16 and np.array_equal(x3, x1)  # the default path is what it was


def test_solve_device_reads_d_x_as_the_guess(gpu):
    """pls_solve_device with the option: d_x is read.  The solution of the same b as the guess gives
    its = 0 and leaves d_x bitwise alone; zeros give the zero-guess solve; a Fischer guess replaces
    the incoming x (NaN in d_x is never read) and the host path then refuses an x0."""
    import lib._native as N
    spec = S.SynthSpec(2, 12)
    b = S.rhs(spec)
    h = K._handle(spec, PARAMS, dict(G.table_db("2d12_right"), global_ksp_initial_guess_nonzero="true"))
    assert h.initial_guess_nonzero()
    d_b, d_x = N.DeviceArray(spec.n), N.DeviceArray(spec.n)
    d_b.upload(b)
    d_x.upload(np.zeros(spec.n))
    r1 = h.solve_device(d_b.p, d_x.p)
    x1 = d_x.download()
    assert (r1.its, r1.reason) == (16, 2)
    r2 = h.solve_device(d_b.p, d_x.p)
    assert (r2.its, r2.reason, h.history().size) == (0, 2, 1) and np.array_equal(d_x.download(), x1)
    d_x.upload(10.0 * x1)
    r3 = h.solve_device(d_b.p, d_x.p)
    assert r3.reason == 2 and r3.its > 0 and h.history()[0] > 8 * np.linalg.norm(b)
    assert np.linalg.norm(b - h.matmult(d_x.download())) <= 1e-6 * np.linalg.norm(b) * (1 + 1e-6)
    hf = K._handle(spec, PARAMS, dict(G.table_db("2d12_right"), global_ksp_initial_guess_nonzero="true", **fischer(2)))
    assert not hf.initial_guess_nonzero()
    d_x.upload(np.full(spec.n, np.nan))
    r4 = hf.solve_device(d_b.p, d_x.p)
    assert (r4.its, r4.reason) == (16, 2) and np.array_equal(d_x.download(), x1)
    with pytest.raises(ValueError, match="libpls would not read it"):
        hf.solve(b, x0=x1)


def test_nonzero_guess_measures_rtol_against_b(gpu):
    """A poor guess (x0 = 10 x) does not loosen the tolerance: the solve ends at rtol ||b||."""
    spec = S.SynthSpec(2, 12)
    db = dict(G.table_db("2d12_right"), global_ksp_initial_guess_nonzero="1")
    h = K._handle(spec, PARAMS, db)
    b = S.rhs(spec)
    x1, _ = h.solve(b)
    x2, r = h.solve(b, x0=10.0 * x1)
    hist = h.history()
    bn = np.linalg.norm(b)
    assert r.reason == 2 and hist[0] > 8 * bn and hist[-1] <= 1e-6 * bn < hist[-2]
    assert np.linalg.norm(b - h.matmult(x2)) <= 1e-6 * bn * (1 + 1e-6)


def test_facade_passes_x_iff_the_option_is_set(gpu):
    """Solver.solve(b, x) through the options file: with the option x is the guess (the second
    solve of the same b starts converged), without it x's contents are never read."""
    from lib import options as popts
    from lib.IndexSet import IndexSet
    from lib.Parser import load_options_lines
    from lib.Preconditioner import Preconditioner
    from lib.Solver import Solver
    spec = S.SynthSpec(2, 12)
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    b = S.rhs(spec)
    out = {}
    for on in (True, False):
        db = dict(G.table_db("2d12_right"), **({"global_ksp_initial_guess_nonzero": "true"} if on else {}))
        popts.DB.clear()
        try:
            load_options_lines([f"-{k} {v}" for k, v in db.items()])
            index_map = IndexSet(S.field_major_index_sets(spec), two_way=True)
            pc = Preconditioner(index_map, A, P, Pd, PARAMS, S.bcs_sub_pressure(spec)).get_pc()
            solver = Solver(A, b, pc, PARAMS, index_map)
            solver.create_solver(A, b, pc)
            solver.set_up()
            x = np.zeros_like(b)
            solver.solve(b, x)
            first = (solver.getIterationNumber(), x.copy())
            solver.solve(b, x)  # x now holds the solution
            out[on] = (first, (solver.getIterationNumber(), x.copy()))
        finally:
            popts.DB.clear()
    (its_a, xa), (its_b, xb) = out[True]
    assert its_a == 16 and its_b == 0 and np.array_equal(xa, xb)
    (its_c, xc), (its_d, xd) = out[False]
    assert its_c == 16 and its_d == 16 and np.array_equal(xc, xd) and np.array_equal(xc, xa)


# ------------------------------------------------------- 5. properties ----
def _six_steps(spec, db, params=PARAMS, steps=6):
    h = K._handle(spec, params, db)
    A, b0 = S.matrix(spec, 0), S.rhs(spec)
    rng = np.random.default_rng(0)
    g = (rng.standard_normal(spec.n), rng.standard_normal(spec.n))
    x = np.zeros(spec.n)
    out = []
    for t in range(steps):
        x, r = h.solve(R.sequence_rhs(A, b0, t, x, g))
        out.append((x, r.its, h.history()))
    return h, out


def test_two_fresh_handles_give_the_same_bits(gpu):
    spec = S.SynthSpec(3, 4)
    db = dict(G.table_db("3d4_right"), **fischer(2))
    h1, a = _six_steps(spec, db)
    h2, c = _six_steps(spec, db)
    assert h1.ksp_guess_stats("global_") == h2.ksp_guess_stats("global_")
    for (x1, i1, hist1), (x2, i2, hist2) in zip(a, c):
        assert i1 == i2 and np.array_equal(hist1, hist2) and np.array_equal(x1, x2)


def test_debug_bounds_guards_the_columns(gpu):
    spec = S.SynthSpec(2, 12)
    db = dict(G.table_db("2d12_right"), **fischer(2))
    _, a = _six_steps(spec, db)
    _, c = _six_steps(spec, dict(db, **{"pls.debug_bounds": "1"}))
    for (x1, i1, hist1), (x2, i2, hist2) in zip(a, c):
        assert i1 == i2 and np.array_equal(hist1, hist2) and np.array_equal(x1, x2)


def test_update_matrices_with_A_empties_the_space(gpu):
    from lib.handle import Handle, params_to_options
    spec = S.SynthSpec(2, 8)
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    opts = dict(G.table_db("2d12_right"), **fischer(4))
    opts.update(params_to_options(PARAMS))
    h = Handle.from_csr(A, P, Pd, is_s, is_f, is_p, S.bcs_sub_pressure(spec), opts)
    b = S.rhs(spec)
    h.solve(b)
    h.solve(b * np.linspace(1.0, 2.0, b.size))
    assert h.ksp_guess_stats("global_")[0] == (1, 2, 4, 2, 0, 0)
    h.update_matrices(P=P)  # A untouched: the space stays
    assert h.ksp_guess_stats("global_")[0] == (1, 2, 4, 2, 0, 0)
    h.update_matrices(A=A)
    assert h.ksp_guess_stats("global_")[0] == (1, 0, 4, 2, 0, 1)
    _, r = h.solve(b)
    assert r.reason == 2 and h.ksp_guess_stats("global_")[0] == (1, 1, 4, 3, 0, 1)


# ------------------------ 6. inner prefixes: 8,450 and 1,089 rows, inner CG ----
def _inner_case(spec, params, db, target, prefix, size, inner, rule):
    """The restatement on an inner KSP of the block PC under a restated outer fgmres: the inner
    solves of one outer solve are the sequence."""
    A, o = _oracle(spec, params, db)
    b = S.rhs(spec)
    o.solver.solve = lambda bb: G.gmres(o.solver, bb, flexible=True)
    ksp = getattr(o.block_pc, target)
    runs = []

    def run(seed):
        g = Perturbed(ksp, size=size)
        log = []

        def solve(bb):
            x = R.guessed_solve(ksp, bb, None, inner, guess=g, rule=rule)
            log.append(ksp.its)
            return x

        ksp.solve = solve
        saved = []
        if seed is not None:
            g.rng = np.random.default_rng(seed)
            saved = _perturb_pcs(o, g.rng)
        try:
            xo = o.solve(b)
        finally:
            for pc, orig in saved:
                pc.apply = orig
        return xo, o.its, o.reason, np.asarray(o.history), log, g.stats()

    xo, its, reason, ho, log, stats = run(None)
    floor = xfloor = 0.0
    for seed in range(4):
        x2, its2, _, h2, log2, stats2 = run(seed)
        assert (its2, log2, stats2) == (its, log, stats), f"bad input: seed {seed} gives {log2} {stats2}, not {log} {stats}"
        floor = max(floor, _rel(h2, ho))
        xfloor = max(xfloor, float(np.linalg.norm(x2 - xo) / np.linalg.norm(xo)))
    tol, xtol = max(1e-10, 10 * floor), max(1e-8, 10 * xfloor)
    print(f"restatement: outer its {its}, inner its {log}, guess stats {stats}, tol {tol:.1e}")
    h = K._handle(spec, params, db)
    x, r = h.solve(b)
    hist = h.history()
    assert (r.its, r.reason) == (its, reason) and hist.shape == ho.shape
    assert _rel(hist, ho) <= tol and np.linalg.norm(x - xo) <= xtol * np.linalg.norm(xo)
    kst, gst = h.ksp_stats(prefix), h.ksp_guess_stats(prefix)[0]
    print(f"{prefix} solves {kst[0]} ({len(log)}) its {kst[1]} ({sum(log)}) guess stats {gst}")
    assert kst[:2] == (len(log), sum(log)) and gst == stats
    assert h.ksp_guess_stats("global_")[0][0] == 0
    return log, stats


def test_inner_s_cg_8450_rows(gpu):
    spec = S.SynthSpec(2, 32)
    params = dict(K.BASE, **{"pc type": "diagonal 3-way", "solver maxiter": 5})
    db = dict(K.FGMRES_DB, s_ksp_type="cg", s_pc_type="jacobi", s_ksp_norm_type="unpreconditioned", s_ksp_rtol="1e-2",
              s_ksp_max_it="40", **fischer(2, "s_"))
    assert S.field_major_index_sets(spec)[0].size == 8450
    log, stats = _inner_case(spec, params, db, "ksp_s", "s_", 2, petsc._cg, "b")
    assert stats[5] >= 1  # the space was emptied and filled again


def test_inner_p_gmres_1089_rows(gpu):
    spec = S.SynthSpec(2, 32)
    params = dict(K.BASE, **{"pc type": "diagonal 3-way", "solver maxiter": 5})
    db = dict(K.FGMRES_DB, p_ksp_type="gmres", p_pc_type="jacobi", p_ksp_rtol="1e-3", p_ksp_max_it="30",
              **fischer(2, "p_"))
    assert S.field_major_index_sets(spec)[2].size == 1089
    _inner_case(spec, params, db, "ksp_p", "p_", 2, petsc._gmres, None)


# ---------------------------------------------------------- 7. refusals ----
@pytest.mark.parametrize("extra,match", [
    ({"s_ksp_type": "cg", "s_ksp_initial_guess_nonzero": "true"}, "s_ksp_initial_guess_nonzero.*outer solver.*prefix 's_'"),
    ({"global_ksp_type": "preonly", "global_ksp_initial_guess_nonzero": None}, "KSPPREONLY cannot start from a nonzero"),
    ({"global_ksp_guess_type": "pod"}, "global_ksp_guess_type.*'pod'.*available: none, fischer"),
    ({"s_ksp_type": "cg", "s_ksp_guess_type": "pod"}, "s_ksp_guess_type.*available: none, fischer"),
    ({"global_ksp_guess_type": "fischer", "global_ksp_guess_fischer_model": "1,10"}, "model 1 is not available.*model 2"),
    ({"global_ksp_guess_type": "fischer", "global_ksp_guess_fischer_model": "3,10"}, "model 3 is not available.*model 2"),
    ({"global_ksp_guess_type": "fischer", "global_ksp_guess_fischer_model": "2,0"}, "size 0 is outside 1 <= size <= 64"),
    ({"global_ksp_guess_type": "fischer", "global_ksp_guess_fischer_model": "2,65"}, "size 65 is outside 1 <= size <= 64"),
    ({"global_ksp_guess_type": "fischer", "global_ksp_guess_fischer_model": "2"}, "takes <model>,<size>"),
    ({"pls.solver_type": "aar", "global_ksp_initial_guess_nonzero": "true"}, "global_ksp_initial_guess_nonzero.*aar"),
    ({"pls.solver_type": "aar", "global_ksp_guess_type": "fischer"}, "global_ksp_guess_type.*aar"),
    ({"pls.solver_type": "aar", "global_ksp_guess_fischer_model": "2,4"}, "global_ksp_guess_fischer_model.*aar"),
])
def test_refusals(gpu, extra, match):
    spec = S.SynthSpec(2, 4)
    extra = dict(extra)
    params = dict(PARAMS, **{"solver type": extra.pop("pls.solver_type", "gmres")})
    with pytest.raises(RuntimeError, match=match):
        h = K._handle(spec, params, dict(G.table_db("2d12_right"), **extra))
        h.solve(S.rhs(spec))


def test_unknown_prefix_is_refused(gpu):
    spec = S.SynthSpec(2, 4)
    h = K._handle(spec, PARAMS, G.table_db("2d12_right"))
    h.solve(S.rhs(spec))
    with pytest.raises(RuntimeError, match="pls_get_ksp_guess_stats: no inner solver with prefix 'nope_'"):
        h.ksp_guess_stats("nope_")
