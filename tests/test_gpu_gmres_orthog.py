"""GMRES's orthogonalisation choices on the device -- modified Gram-Schmidt
(``<prefix>ksp_gmres_modifiedgramschmidt``) and classical Gram-Schmidt with
``<prefix>ksp_gmres_cgs_refinement_type`` refine_ifneeded / refine_always, for
gmres and fgmres -- against their numpy restatement
(tests/gmres_orthog_restatement.py, pinned on the CPU by
tests/test_gmres_orthog_restatement.py).

Tolerances, the project's rule (tests/test_gpu_ksp_types.py): iteration count
and reason exact; every history entry within max(1e-10, 10 x the restatement's
own worst deviation over 4 seeds when every inner PC output is perturbed by
1e-15 relative); the solution within max(1e-8, that bound) relative.

Before the device runs, every comparison asserts on the CPU restatement that
the iteration count (and refine_ifneeded's second-pass count) is the same for
all seeds, that no refine_ifneeded decision is nearer than 1e-6 to its
threshold and, where the case is *discriminating*, that the scheme's history
differs from unrefined classical Gram-Schmidt's by at least 10 x the
tolerance: "option accepted, CGS run" cannot pass there.  A failure of one of
these means a bad input, not a wrong device.
"""
import numpy as np
import pytest

import gmres_orthog_restatement as G
import test_gpu_ksp_types as K
from oracle import synthetic as S
from oracle.solver import OracleSolver

pytestmark = pytest.mark.gpu

SCHEME_CODE = {"cgs": 0, "refine_ifneeded": 1, "refine_always": 2, "mgs": 3}


def _scheme_db(prefix, scheme):
    return {prefix + k: v for k, v in G.SCHEMES[scheme][0].items()}


def _oracle(spec, params, db):
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    return OracleSolver(A, P, Pd, is_s, is_f, is_p, params, db, S.bcs_sub_pressure(spec))


def _install(ksp, scheme, flexible=False, log=None):
    """ksp.solve = the restatement with this scheme; every solve appends
    (its, second passes, nearest decision) to log."""
    kw = dict(G.SCHEMES[scheme][1], flexible=flexible)

    def solve(b):
        x = G.gmres(ksp, b, **kw)
        if log is not None:
            log.append((ksp.its, ksp.second_passes, ksp.nearest_decision))
        return x

    ksp.solve = solve


def _reference(spec, params, db, scheme, flexible=False, discriminating=False, b=None, target="solver",
               outer_flexible=None):
    """The CPU side of a comparison: the oracle with the restatement installed
    on ``target`` ("solver": the outer KSP, else an attribute of the block PC;
    the outer KSP is then the oracle's own gmres, or the restated fgmres when
    outer_flexible), its solution, and the tolerance; asserts that the input is a good one."""
    b = S.rhs(spec) if b is None else b
    o = _oracle(spec, params, db)
    log = []
    if target == "solver":
        ksp = o.solver
    else:
        ksp = getattr(o.block_pc, target)
        if outer_flexible:
            _install(o.solver, "cgs", flexible=True)
    _install(ksp, scheme, flexible, log)
    xo = o.solve(b)
    first = list(log)
    its, reason, ho = o.its, o.reason, np.asarray(o.history)
    floor = K._noise_floor(o, b, ho, its)
    tol = max(1e-10, 10 * floor)
    if target == "solver":
        for entry in log[1:]:
            assert entry[:2] == log[0][:2], f"bad input: its / second passes {entry[:2]} with a seed, {log[0][:2]} without"
    nearest = min(e[2] for e in log)
    if scheme == "refine_ifneeded":
        assert nearest >= 1e-6, f"bad input: a refine_ifneeded decision {nearest:.1e} from its threshold"
    gap = None
    if discriminating:
        _install(ksp, "cgs", flexible)
        o.solve(b)
        hc = np.asarray(o.history)
        assert hc.shape == ho.shape, "bad input: unrefined CGS takes another number of iterations"
        gap = float(np.max(np.abs(hc - ho) / np.abs(ho)))
        assert gap >= 10 * tol, f"bad input: not discriminating, |CGS - {scheme}| {gap:.2e} < 10 x tol {tol:.2e}"
        _install(ksp, scheme, flexible)
    print(f"restatement: its {its} reason {reason} floor {floor:.2e} tol {tol:.2e} nearest {nearest:.2e} "
          f"|CGS - {scheme}| {gap}")
    return {"o": o, "b": b, "xo": xo, "its": its, "reason": reason, "ho": ho, "tol": tol, "first": first}


def _device(spec, params, db, ref):
    h = K._handle(spec, params, db)
    x, r = h.solve(ref["b"])
    hist = h.history()
    ho, xo, tol = ref["ho"], ref["xo"], ref["tol"]
    print(f"device: its {r.its} ({ref['its']}) reason {r.reason} ({ref['reason']})")
    assert r.its == ref["its"], f"its {r.its} vs restatement {ref['its']}"
    assert r.reason == ref["reason"], f"reason {r.reason} vs restatement {ref['reason']}"
    assert hist.shape == ho.shape
    rel = np.max(np.abs(hist - ho) / np.abs(ho))
    xerr = np.linalg.norm(x - xo) / np.linalg.norm(xo)
    print(f"history rel diff {rel:.3e} (tol {tol:.2e}); |x - x_o| / |x_o| {xerr:.3e}")
    assert rel <= tol, f"residual history rel diff {rel:.3e} (tol {tol:.1e})"
    assert xerr <= max(1e-8, tol)
    return h, x, r


def _table_case(name, scheme, discriminating):
    dim, N, _, _, n, its, second = G.TABLE[name]
    spec = S.SynthSpec(dim, N)
    db = dict(G.table_db(name), **_scheme_db("global_", scheme))
    ref = _reference(spec, G.PARAMS, db, scheme, discriminating=discriminating)
    assert ref["its"] == its and spec.n == n
    passes = {"mgs": 0, "refine_always": its, "refine_ifneeded": second}[scheme]
    assert ref["first"][0][1] == passes
    h, _, r = _device(spec, G.PARAMS, db, ref)
    st = h.gmres_orthog_stats("global_")
    print("gmres_orthog_stats", st)
    assert st == (its, passes, SCHEME_CODE[scheme])
    return h, r


# ---------------- 1. the schemes, never restarted (discriminating) ----
@pytest.mark.parametrize("scheme", ["mgs", "refine_always", "refine_ifneeded"])
@pytest.mark.parametrize("name", ["2d12_left", "2d12_right", "3d4_right"])
def test_scheme_outer_gmres(gpu, name, scheme):
    """In 2d12_left and 3d4_right refine_ifneeded skips one second pass: the
    not-needed branch ran."""
    _table_case(name, scheme, discriminating=True)


# ------------------------------------ 2. restarted, refine_ifneeded ----
def test_ifneeded_restart5(gpu):
    """61 iterations in cycles of 5, 53 second passes.  The restarted history's
    own floor is ~1e-6 here, so this case does not discriminate; the counts do."""
    _table_case("2d12_right_restart5", "refine_ifneeded", discriminating=False)


# ----------------------------------------------------------- 3. fgmres ----
@pytest.mark.parametrize("scheme", ["mgs", "refine_always"])
def test_scheme_outer_fgmres(gpu, scheme):
    spec = S.SynthSpec(2, 12)
    db = dict(G.table_db("2d12_right", "fgmres"), **_scheme_db("global_", scheme))
    ref = _reference(spec, G.PARAMS, db, scheme, flexible=True, discriminating=True)
    h, _, r = _device(spec, G.PARAMS, db, ref)
    assert r.pc_applies == r.its  # no PC application in BuildSoln
    its = ref["its"]
    assert h.gmres_orthog_stats("global_") == (its, its if scheme == "refine_always" else 0, SCHEME_CODE[scheme])


# ------------------------------------------------------ 4. inner prefix ----
def test_mgs_inner_s(gpu):
    """s_ksp_type gmres (left, Jacobi) at s_ksp_rtol 1e-3 with modified
    Gram-Schmidt under outer FGMRES (the pattern of test_bcgs_inner_s)."""
    spec = S.SynthSpec(2, 12)
    db = dict(K.FGMRES_DB, s_ksp_type="gmres", s_pc_type="jacobi", s_ksp_rtol="1e-3", **_scheme_db("s_", "mgs"))
    ref = _reference(spec, K.BASE, db, "mgs", target="ksp_s", outer_flexible=True)
    solves, its = len(ref["first"]), sum(e[0] for e in ref["first"])
    assert solves == ref["its"] and its > solves
    h, _, _ = _device(spec, K.BASE, db, ref)
    st, ost = h.ksp_stats("s_"), h.gmres_orthog_stats("s_")
    print(f"s_ solves {st[0]} ({solves}) its {st[1]} ({its}); orthog stats {ost}")
    assert st[0] == solves and st[1] == its
    assert ost == (its, 0, 3)
    assert h.gmres_orthog_stats("global_") == (ref["its"], 0, 0)


# ------------------------------------------- 5. the reference's own line ----
@pytest.mark.parametrize("N", [4, 8])
def test_reference_inexact_fp_gmres_mgs(gpu, N):
    """petsc-options-inexact's fp block with fp_ksp_type switched from preonly
    to gmres, its -fp_ksp_gmres_modifiedgramschmidt kept."""
    import test_gpu_parity as P
    spec = S.SynthSpec(2, N)
    db = dict(P.FS_INEXACT, fp_ksp_type="gmres")
    assert "fp_ksp_gmres_modifiedgramschmidt" in db
    params = dict(P.BASE, **P.FS_PARAMS)
    params["solver maxiter"] = 200
    ref = _reference(spec, params, db, "mgs", target="ksp_fp")
    fp_its = sum(e[0] for e in ref["first"])
    assert fp_its > len(ref["first"])  # the fp solves take more than one step: there is something to orthogonalise
    h, _, _ = _device(spec, params, db, ref)
    st = h.gmres_orthog_stats("fp_")
    print("fp_ orthog stats", st, "restatement its", fp_its)
    assert st == (fp_its, 0, 3)


# ------------------------------------------ 6. more than one block ----
def test_mgs_multi_block_fused_bitwise(gpu):
    """3-D N=6: n = 13525 rows (odd) in 4 reduction blocks, so the last-arriving
    block of a step sums parts of others (n = 2669 above is one block).  The
    single-launch sums (pls.gmres_mgs_fused 1) and k_final after every step (0)
    add in the same order: bitwise the same history and x."""
    spec = S.SynthSpec(3, 6)
    assert spec.n == 13525
    db = dict(G.BLOCKS_ILU, global_ksp_type="gmres", global_ksp_pc_side="right", global_ksp_gmres_restart="400",
              **_scheme_db("global_", "mgs"))
    ref = _reference(spec, G.PARAMS, db, "mgs")
    assert ref["its"] == 16
    out = []
    for fused in ("1", "0"):
        dbf = dict(db, **{"pls.gmres_mgs_fused": fused})
        h, x, r = _device(spec, G.PARAMS, dbf, ref)
        assert h.gmres_orthog_stats("global_") == (16, 0, 3)
        out.append((x, h.history()))
    assert np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][0], out[1][0])


# --------------------------------------------------------- 7. defaults ----
def test_default_spellings_bitwise_and_both_flags(gpu):
    """ksp_gmres_classicalgramschmidt and refine_never are the default, bit for
    bit; with both Gram-Schmidt flags the modified one wins (PETSc reads the
    classical flag first)."""
    spec = S.SynthSpec(2, 12)
    db = G.table_db("2d12_right")
    b = S.rhs(spec)

    def run(extra):
        h = K._handle(spec, G.PARAMS, dict(db, **extra))
        x, r = h.solve(b)
        return x, h.history(), h.gmres_orthog_stats("global_"), r

    x0, h0, st0, r0 = run({})
    assert st0 == (r0.its, 0, 0)
    for extra in ({"global_ksp_gmres_classicalgramschmidt": None},
                  {"global_ksp_gmres_cgs_refinement_type": "refine_never"}):
        x, hist, st, _ = run(extra)
        assert st == st0 and np.array_equal(hist, h0) and np.array_equal(x, x0)
    both = {"global_ksp_gmres_classicalgramschmidt": None, "global_ksp_gmres_modifiedgramschmidt": None,
            "global_ksp_gmres_cgs_refinement_type": "refine_always"}  # (ignored under MGS)
    xm, hm, stm, rm = run({"global_ksp_gmres_modifiedgramschmidt": None})
    xb, hb, stb, _ = run(both)
    assert stm == (rm.its, 0, 3) and stb == stm
    assert np.array_equal(hb, hm) and np.array_equal(xb, xm)
    assert not np.array_equal(hm, h0)


def test_other_types_ignore_the_options(gpu):
    """A bcgs outer KSP takes all three options (even a refinement type that
    gmres would refuse) and has no orthogonalisation to report."""
    spec = S.SynthSpec(2, 4)
    db = dict(G.BLOCKS_ILU, global_ksp_type="bcgs", global_ksp_gmres_modifiedgramschmidt=None,
              global_ksp_gmres_classicalgramschmidt=None, global_ksp_gmres_cgs_refinement_type="refine_sometimes")
    h = K._handle(spec, K.BASE, db)
    _, r = h.solve(S.rhs(spec))
    assert r.reason > 0
    with pytest.raises(RuntimeError, match="not gmres or fgmres"):
        h.gmres_orthog_stats("global_")
    with pytest.raises(RuntimeError, match="no inner solver with prefix 'nope_'"):
        h.gmres_orthog_stats("nope_")


# ---------------------------------------------------------- 8. refusal ----
def test_unknown_refinement_type_is_refused(gpu):
    spec = S.SynthSpec(2, 4)
    db = dict(G.table_db("2d12_right"), global_ksp_gmres_cgs_refinement_type="refine_sometimes")
    with pytest.raises(RuntimeError, match="global_ksp_gmres_cgs_refinement_type.*refine_never, refine_ifneeded, refine_always"):
        h = K._handle(spec, G.PARAMS, db)
        h.solve(S.rhs(spec))
