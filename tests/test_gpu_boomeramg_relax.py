"""BoomerAMG relax types Jacobi, l1scaled-Jacobi and Chebyshev on the device
(-<prefix>pc_hypre_boomeramg_relax_type_all; csrc/boomeramg.cpp) against
tests/boomeramg_relax_restatement.py:

1. one block-preconditioner application <= 1e-12 relative in the max norm (tests/test_gpu_amg.py's
   bar) for every type, with no_CF and with C/F relaxation, grid_sweeps_all 1 and 2, Chebyshev
   orders 1-4, a Jacobi weight of 0.7 and Chebyshev fractions 0.1 and 0.6 (each checked to give
   another vector than the default value), and the same with pls.amg_csr_below 0 (the small levels then take D16 layouts and
   the fused step);
2. pls_get_boomeramg_relax: lambda equal to the restatement's, the fused / unfused launch counts,
   fused and unfused the same bits, two handles the same bits;
3. pls_relax_step on the adversarial patterns of tests/spmv_layout_cases.py with data on which
   every operation is exact: bit for bit the int64 formula, fused and unfused;
4. whole solves under options/inexact-lift-chebyshev-relax against tests/golden/boomeramg_relax;
5. refusals name their key; pls_update_matrices builds m / lambda again.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import boomeramg_relax_restatement as BR
import spmv_layout_cases as C
from oracle import synthetic as S
from test_gpu_amg import PREFIXES, _amg_db, _boomer_db
from test_gpu_parity import BASE, _handle, _oracle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

SPECS = {"2d16": S.SynthSpec(2, 16), "3d5": S.SynthSpec(3, 5)}
# (relax type, no_CF, Chebyshev order[, Jacobi weight, Chebyshev fraction]); weight and fraction
# are set only where given (else the defaults 1.0 and 0.3 are not named)
CONFIGS = [("Jacobi", True, 0), ("Jacobi", False, 0), ("l1scaled-Jacobi", True, 0), ("l1scaled-Jacobi", False, 0),
           ("Chebyshev", True, 1), ("Chebyshev", True, 2), ("Chebyshev", True, 3), ("Chebyshev", True, 4),
           ("Chebyshev", False, 2),
           ("Jacobi", True, 0, "0.7", None), ("Jacobi", False, 0, "0.7", None),
           ("Chebyshev", True, 2, None, "0.1"), ("Chebyshev", True, 3, None, "0.6")]


def _relax_db(rtype, no_cf, order, sweeps, extra=None, weight=None, fraction=None):
    keys = dict(_boomer_db(no_cf))
    for pre in PREFIXES:
        keys[pre + "pc_hypre_boomeramg_relax_type_all"] = rtype
        keys[pre + "pc_hypre_boomeramg_grid_sweeps_all"] = str(sweeps)
        if order:
            keys[pre + "pls_boomeramg_chebyshev_order"] = str(order)
        if weight:
            keys[pre + "pc_hypre_boomeramg_relax_weight_all"] = weight
        if fraction:
            keys[pre + "pls_boomeramg_chebyshev_fraction"] = fraction
    keys.update(extra or {})
    return _amg_db("hypre", keys)


def _restated(spec, params, db):
    old = BR.install()
    try:
        return _oracle(spec, params, db)
    finally:
        BR.uninstall(old)


@functools.lru_cache(maxsize=None)
def _reference(spec_id, pc_type, rtype, no_cf, order, sweeps, weight=None, fraction=None):
    """(x, the restatement's application to x, its s_ block's lambdas), computed once."""
    spec = SPECS[spec_id]
    params = dict(BASE, **{"pc type": pc_type, "inner pc type": "lu"})
    o = _restated(spec, params, _relax_db(rtype, no_cf, order, sweeps, weight=weight, fraction=fraction))
    x = np.random.default_rng(3).standard_normal(spec.n)
    yo = o.block_pc.apply(x)
    yo.setflags(write=False)
    return x, yo, o.block_pc.ksp_s.pc.lambdas()


# ------------------------------------------------ 1. pc_apply vs restatement --
@pytest.mark.parametrize("csr_below", ["default", "0"])
@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"{c[0]}-{'nocf' if c[1] else 'cf'}-o{c[2]}" + (
    f"-w{c[3]}-f{c[4]}" if len(c) > 3 else ""))
@pytest.mark.parametrize("pc_type", ["diagonal", "diagonal 3-way"])
@pytest.mark.parametrize("spec_id", list(SPECS))
def test_pc_apply_matches_restatement(gpu, spec_id, pc_type, config, sweeps, csr_below):
    rtype, no_cf, order = config[:3]
    weight, fraction = config[3:] if len(config) > 3 else (None, None)
    x, yo, _ = _reference(spec_id, pc_type, rtype, no_cf, order, sweeps, weight, fraction)
    assert np.all(np.isfinite(yo))
    if weight or fraction:  # the value is read: the default's application is another vector, 1e6 x the bar apart
        yd = _reference(spec_id, pc_type, rtype, no_cf, order, sweeps)[1]
        assert np.max(np.abs(yd - yo)) > 1e-6 * np.max(np.abs(yo))
    extra = {} if csr_below == "default" else {"pls.amg_csr_below": csr_below}
    params = dict(BASE, **{"pc type": pc_type, "inner pc type": "lu"})
    h = _handle(SPECS[spec_id], params, _relax_db(rtype, no_cf, order, sweeps, extra, weight, fraction))
    y = h.pc_apply(x)
    st, _ = h.boomeramg_relax("s_")
    h.destroy()
    err = np.max(np.abs(y - yo)) / np.max(np.abs(yo))
    print(f"{spec_id} {pc_type} {config} sweeps {sweeps} csr_below {csr_below}: rel max err {err:.2e}, s_ stats {st}")
    assert err <= 1e-12


# ---------------------------------------------------- 2. stats and lambda -----
@pytest.mark.parametrize("config", [("Chebyshev", True, 3), ("l1scaled-Jacobi", False, 0), ("Jacobi", True, 0)],
                         ids=lambda c: c[0])
def test_stats_lambda_and_fused_bits(gpu, config):
    rtype, no_cf, order = config
    spec, pc_type = SPECS["2d16"], "diagonal"
    x, yo, lam_o = _reference("2d16", pc_type, rtype, no_cf, order, 1)
    params = dict(BASE, **{"pc type": pc_type, "inner pc type": "lu"})
    out = {}
    for tag, extra in (("fused", {"pls.amg_csr_below": "0"}), ("again", {"pls.amg_csr_below": "0"}),
                       ("unfused", {"pls.amg_csr_below": "0", "pls.amg_relax_fused": "0"})):
        h = _handle(spec, params, _relax_db(rtype, no_cf, order, 1, extra))
        y = h.pc_apply(x)
        st, lam = h.boomeramg_relax("s_")
        h.destroy()
        out[tag] = (y, st, lam)
        print(tag, st, lam)
    st, lam = out["fused"][1:]
    assert st[0] == BR.RELAX_TYPES.index(rtype) and st[1] == len(lam_o) and st[1] >= 1
    if order:
        assert st[2] == order
    assert np.array_equal(lam, np.asarray(lam_o))
    assert (np.all(lam > 0) if rtype == "Chebyshev" else np.all(lam == 0))
    assert st[3] > 0 and st[4] > 0
    stu = out["unfused"][1]
    assert stu[3] == 0 and stu[4] == 0 and stu[5] == st[4] + st[5]
    assert np.array_equal(out["fused"][0], out["unfused"][0])
    assert np.array_equal(out["fused"][0], out["again"][0])
    assert np.max(np.abs(out["fused"][0] - yo)) <= 1e-12 * np.max(np.abs(yo))


# ------------------------------------------- 3. one step, exact arithmetic ----
# (case id, was_fused expected with fused = 1)
STEP_CASES = [("edges-3", True), ("edges-65", True), ("edges-130", True), ("wide-1100-lpr4", True),
              ("sigma-lpr2", True), ("sigma-lpr16", True), ("ramp", True), ("dense-row", True), ("delta-edge", True),
              ("segments-8", True), ("b3-mixed", False), ("b3-all", False), ("rcm-forced-uniform", False),
              ("edges-65-sell", False)]


def _step_data(case):
    A, x = C.matrix(case, "int")
    n = A.shape[0]
    rng = np.random.default_rng(case.seed + 77)
    b = rng.integers(-16, 17, n).astype(np.float64)
    d = rng.integers(-16, 17, n).astype(np.float64)
    m = 2.0 ** rng.integers(-2, 3, n) * rng.choice((-1.0, 1.0), n)
    return A, x, b, d, m


def _exact_step(A, x, b, d, m, a, g):
    """(x_new, dn) by the formula in int64, everything scaled by 4 (m is +-2^k, k >= -2)."""
    res = b.astype(np.int64) - C.exact_product(A, x)
    m4 = (4 * m).astype(np.int64)
    assert np.array_equal(m4 / 4.0, m)
    dn4 = int(g) * m4 * res + (0 if d is None else 4 * int(a) * d.astype(np.int64))
    xn4 = 4 * x.astype(np.int64) + dn4
    assert np.max(np.abs(xn4)) < 2 ** 52
    return xn4 / 4.0, dn4 / 4.0


@pytest.mark.parametrize("with_d", [True, False], ids=["d", "no-d"])
@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "unfused"])
@pytest.mark.parametrize("name,expect_fused", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_relax_step_is_exact_on_layout_cases(gpu, name, expect_fused, fused, with_d):
    from lib.handle import Handle
    case = C.BY_ID[name]
    A, x, b, d, m = _step_data(case)
    n = A.shape[0]
    is_s, is_f, is_p, _ = C.index_sets(case, n)
    h = Handle.from_csr(A, sp.identity(n, format="csr"), None, is_s, is_f, is_p, [], case.options)
    try:
        xn, dn, was = h.relax_step(m, b, x, d if with_d else None, a=2.0, g=1.0, fused=bool(fused))
    finally:
        h.destroy()
    ex, ed = _exact_step(A, x, b, d if with_d else None, m, 2, 1)
    print(f"{name} fused {fused} d {with_d}: was_fused {was}, rows wrong {np.count_nonzero(xn != ex)}")
    assert was == (expect_fused and bool(fused))
    assert np.array_equal(xn, ex)
    if with_d:
        assert np.array_equal(dn, ed)
    else:
        assert dn is None


# --------------------------------------------------------- 4. whole solves ----
@pytest.mark.parametrize("name", ["footing_N10", "swelling_N10"])
def test_whole_solve_matches_golden(gpu, name):
    import robustness as R
    ref = json.load(open(os.path.join(HERE, "golden", "boomeramg_relax", name + "_inexact-lift-chebyshev-relax.json")))
    r = R.run_case(ref["problem"], ref["N"], ref["pc_type"], ref["options"], ref["np"], history=True)
    inner = r["inner"]["s_"]
    pert = ref["perturbed_its"] + [ref["its"]]
    k = min(ref["first_dev"])
    h, ho = np.asarray(r["history"]), np.asarray(ref["history"])
    assert k >= 3 and h.size >= k and ho.size >= k, (k, h.size, ho.size)
    m = k
    dev = np.max(np.abs(h[:m] - ho[:m]) / ho[:m])
    print(f"{name}: outer its {r['its']} reason {r['reason']} (restatement {ref['its']}, perturbed {pert}); s_ {inner} "
          f"(restatement {ref['s_its']} its over {ref['s_solves']} solves, max {ref['s_max']}); history over the "
          f"first {m} entries within {dev:.2e}; setup {r['setup_s']} s, solve {r['solve_s']} s")
    assert r["reason"] > 0
    assert all(v["negative_reason"] == 0 for v in r["inner"].values()), r["inner"]
    assert min(pert) <= r["its"] <= max(pert), (r["its"], pert)
    assert np.all(np.abs(h[:m] - ho[:m]) <= 1e-10 * ho[:m]), dev


# ---------------------------------------------------- 5. errors and updates ---
@pytest.mark.parametrize("key,value,also,words", [
    ("s_pc_hypre_boomeramg_relax_type_all", "SOR/Jacobi", {}, "symmetric-SOR/Jacobi, Jacobi, l1scaled-Jacobi and Chebyshev"),
    ("s_pc_hypre_boomeramg_relax_weight_all", "heavy", {"s_pc_hypre_boomeramg_relax_type_all": "Jacobi"}, "number"),
    ("s_pls_boomeramg_chebyshev_order", "0", {"s_pc_hypre_boomeramg_relax_type_all": "Chebyshev"}, "1, 2, 3 or 4"),
    ("s_pls_boomeramg_chebyshev_order", "5", {"s_pc_hypre_boomeramg_relax_type_all": "Chebyshev"}, "1, 2, 3 or 4"),
    ("s_pls_boomeramg_chebyshev_fraction", "0", {"s_pc_hypre_boomeramg_relax_type_all": "Chebyshev"}, "(0, 1)"),
    ("s_pls_boomeramg_chebyshev_fraction", "1.0", {"s_pc_hypre_boomeramg_relax_type_all": "Chebyshev"}, "(0, 1)"),
    # the keys are read and checked whatever the type, as the restatement does
    ("s_pls_boomeramg_chebyshev_order", "7", {}, "1, 2, 3 or 4"),
    ("s_pc_hypre_boomeramg_relax_weight_all", "heavy", {}, "number"),
])
def test_refusals_name_the_key(gpu, key, value, also, words):
    db = _amg_db("hypre", dict(_boomer_db(), **also, **{key: value}))
    h = _handle(S.SynthSpec(2, 8), dict(BASE, **{"pc type": "diagonal", "inner pc type": "lu"}), db)
    with pytest.raises(RuntimeError) as e:
        h.setup()
    h.destroy()
    assert key in str(e.value) and words in str(e.value), str(e.value)


def test_query_refusals(gpu):
    db = _amg_db("hypre", _boomer_db())
    h = _handle(S.SynthSpec(2, 8), dict(BASE, **{"pc type": "diagonal", "inner pc type": "lu"}), db)
    with pytest.raises(RuntimeError, match="nope_"):
        h.boomeramg_relax("nope_")
    with pytest.raises(RuntimeError, match="fp_.*ilu"):  # the 2-way fp block keeps ILU(0)
        h.boomeramg_relax("fp_")
    st, lam = h.boomeramg_relax("s_")  # the default smoother: type 0, nothing fused, no estimates
    assert st[0] == 0 and st[3] == 0 and st[4] == 0 and st[5] == 0 and np.all(lam == 0)
    h.destroy()


@pytest.mark.parametrize("config", [("Chebyshev", True, 2), ("Jacobi", True, 0)], ids=lambda c: c[0])
def test_update_matrices_builds_the_smoother_again(gpu, config):
    """1.25 P: the Jacobi m scales by 1 / 1.25 and Chebyshev's lambda is the restatement's on 1.25 P."""
    from lib.handle import Handle, params_to_options
    rtype, no_cf, order = config
    spec = S.SynthSpec(2, 9)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    bcs = S.bcs_sub_pressure(spec)
    params = dict(BASE, **{"pc type": "diagonal", "inner pc type": "lu"})
    db = _relax_db(rtype, no_cf, order, 1)
    opts = dict(db)
    opts.update(params_to_options(params))
    A, P, Pd = (S.matrix(spec, v) for v in (0, 1, 2))
    P2 = (1.25 * P).tocsr()
    x = np.random.default_rng(5).standard_normal(spec.n)
    from oracle.solver import OracleSolver
    old = BR.install()
    try:
        o1 = OracleSolver(A, P, Pd, is_s, is_f, is_p, params, db, bcs)
        o2 = OracleSolver(A, P2, Pd, is_s, is_f, is_p, params, db, bcs)
    finally:
        BR.uninstall(old)
    h = Handle.from_csr(A, P, Pd, is_s, is_f, is_p, bcs, opts)
    y1 = h.pc_apply(x)
    lam1 = h.boomeramg_relax("s_")[1]
    h.update_matrices(None, P2, None)
    y2 = h.pc_apply(x)
    lam2 = h.boomeramg_relax("s_")[1]
    h.destroy()
    yo1, yo2 = o1.block_pc.apply(x), o2.block_pc.apply(x)
    assert np.array_equal(lam1, np.asarray(o1.block_pc.ksp_s.pc.lambdas()))
    assert np.array_equal(lam2, np.asarray(o2.block_pc.ksp_s.pc.lambdas()))
    assert np.max(np.abs(y1 - yo1)) <= 1e-12 * np.max(np.abs(yo1))
    assert np.max(np.abs(y2 - yo2)) <= 1e-12 * np.max(np.abs(yo2))
    assert np.max(np.abs(yo2 - yo1)) > 1e-3 * np.max(np.abs(yo1))  # (the two differ: the update's teeth)
