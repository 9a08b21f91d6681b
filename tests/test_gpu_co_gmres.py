"""Compressed-operator GMRES on the device -- ``<prefix>pls_gmres_operator
single`` on top of ``<prefix>pls_gmres_basis single``: the product inside the
Arnoldi step reads the operator's values from an fp32 stream -- against its
numpy restatement (tests/co_gmres_restatement.py, pinned on the CPU by
tests/test_co_gmres_restatement.py) installed in ``OracleSolver`` with
``low_matrix`` of the internal-order operator.

The bar is the one of tests/test_gpu_cb_gmres.py, whose helpers are used:
iteration count, reason and history length exact; every history entry within
max(1e-10, 10 x the restatement's own worst deviation over 4 seeds when every
inner PC output is perturbed by 1e-15 relative); the solution within max(1e-8,
that bound) relative.

With ``pls.reuse_coupling 0`` the low operator is fl32(A).  With the coupling
reuse (the default where eligible) the reuse rows start from the block PC's
fp64 raw sums, so their entries (i >= ns, j < ns) keep their fp64 values: the
restatement's matrix is then built from ``Handle.reuse_rows()``.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import cb_gmres_restatement as CB
import co_gmres_restatement as CO
import gmres_orthog_restatement as G
import spmv_layout_cases as C
import spmv_layout_restatement as R
import test_gpu_cb_gmres as T
import test_gpu_ksp_types as K
from oracle import synthetic as S

pytestmark = pytest.mark.gpu

BASIS = {"global_pls_gmres_basis": "single"}
LOW = dict(BASIS, global_pls_gmres_operator="single")
NO_REUSE = {"pls.reuse_coupling": "0"}


def _low_bytes(A_internal, mask=None, ns=None):
    """Bytes of the fp32 value streams: 4 per stored entry of A's layout, and with the coupling
    reuse of the reduced layout (A without the coupling entries of the reuse rows, on A's plan)."""
    A = sp.csr_matrix(A_internal)
    L = R.layout(A)
    assert L.d16 and not L.b3 and L.rcm is None
    total = 4 * L.stored
    if mask is not None:
        assert L.plan.rowmap is None
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        keep = ~(mask.astype(bool)[rows] & (A.indices < ns))
        lens = np.bincount(rows[keep], minlength=A.shape[0]).astype(np.int64)
        total += 4 * R.plan_stored(lens, L.plan)
    return total


def _reference(spec, params, db, target="solver", name=None, mask=None, ns=None, **kw):
    """tests/test_gpu_cb_gmres._reference with the compressed-operator restatement installed."""
    b = S.rhs(spec)
    odb = {k: v for k, v in db.items() if "pls_gmres" not in k and not k.startswith("pls.")}
    A, o = T._oracle(spec, params, odb)
    log = []
    if target == "solver":
        ksp = o.solver
    else:
        o.solver.solve = lambda bb: G.gmres(o.solver, bb, flexible=True)
        ksp = getattr(o.block_pc, target)
    A_low = CO.low_matrix(ksp.A, mask, ns)

    def solve(bb):
        x = CO.gmres(ksp, bb, lambda v: A_low @ v, **kw)
        log.append((ksp.its, ksp.cb_forced, ksp.cb_confirm, ksp.cb_failed, ksp.co_low, ksp.co_double,
                    list(ksp.cb_ratios), list(ksp.co_confirm)))
        return x

    ksp.solve = solve
    xo = o.solve(b)
    first = list(log)
    its, reason, ho = o.its, o.reason, np.asarray(o.history)
    tol = max(1e-10, 10 * K._noise_floor(o, b, ho, its))
    if target == "solver":
        for e in log[1:]:
            assert e[:6] == log[0][:6], f"bad input: counters {e[:6]} with a seed, {log[0][:6]} without"
        if name:
            CB.check_ratios(name, log[0][6])
            CO.check_confirmations(name, log[0][7])
    print(f"restatement: its {its} reason {reason} entries {ho.size} tol {tol:.2e} counters {first[0][:6]}")
    return {"A": A, "o": o, "b": b, "xo": xo, "its": its, "reason": reason, "ho": ho, "tol": tol, "first": first,
            "bytes": _low_bytes(ksp.A, mask, ns), "n": ksp.A.shape[0]}


def _check_stats(h, ref, prefix, restart):
    """gmres_operator_stats and gmres_basis_stats against the restatement's counters (summed over
    the solves of an inner KSP)."""
    f = ref["first"]
    ost, bst = h.gmres_operator_stats(prefix), h.gmres_basis_stats(prefix)
    print(f"gmres_operator_stats {ost} (bytes {ref['bytes']}); gmres_basis_stats {bst}")
    assert ost == (1, ref["bytes"], sum(e[4] for e in f), sum(e[5] for e in f))
    assert bst == (1, CB.basis_bytes(ref["n"], restart, True)) + tuple(sum(e[i] for e in f) for i in (1, 2, 3))


def _true_last_entry(ref, x, hist, side):
    r = ref["b"] - ref["A"] @ x
    true = float(np.linalg.norm(r if side == "right" else ref["o"].pc.apply(r)))
    print(f"last history entry {hist[-1]:.6e}, ||b - A x|| in numpy {true:.6e}")
    assert abs(hist[-1] - true) <= ref["tol"] * true


def _low_path_ran(spec, params, db, b, hist):
    """The history differs from the device's own with the fp32 basis alone by more than 1e-9."""
    hb = K._handle(spec, params, {k: v for k, v in db.items() if "pls_gmres_operator" not in k})
    hb.solve(b)
    histb = hb.history()
    assert hb.gmres_operator_stats("global_")[:3] == (0, 0, 0)
    m = min(hist.size, histb.size)
    gap = float(np.max(np.abs(hist[:m] - histb[:m]) / histb[:m]))
    print(f"basis single alone: entries {histb.size}; |low - fp64 operator| history {gap:.2e}")
    assert gap > 1e-9


# ------------------------------------------------- 1. the table, fl32(A) ----
@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", ["2d12_right", "2d12_left", "3d4_right", "2d12_right_restart5"])
def test_table_cases(gpu, name, rtol):
    dim, N, side, restart, n = G.TABLE[name][:5]
    spec = S.SynthSpec(dim, N)
    params = dict(G.PARAMS, **{"solver rtol": rtol})
    db = dict(G.table_db(name), **LOW, **NO_REUSE)
    ref = _reference(spec, params, db, name=name)
    assert (ref["its"], ref["ho"].size) + ref["first"][0][1:4] == CO.RECORDED[name][rtol]
    h, x, r, hist = T._device(spec, params, db, ref)
    _check_stats(h, ref, "global_", restart)
    assert not h.reuse_rows().any() and h.reuse_stats()[0] == 0
    _true_last_entry(ref, x, hist, side)
    _low_path_ran(spec, params, db, ref["b"], hist)


# ------------------------------------------- 2. with the coupling reuse ----
@pytest.mark.parametrize("name", ["2d12_right", "3d4_right"])
def test_with_coupling_reuse(gpu, name):
    """The default reuse: the low product is the reduced launch over A' with fp32 values, started
    from the PC's fp64 raw sums -- the mixed operator that low_matrix builds from reuse_rows()."""
    dim, N, side, restart, n = G.TABLE[name][:5]
    spec = S.SynthSpec(dim, N)
    params = dict(G.PARAMS, **{"solver rtol": 1e-6})
    db = dict(G.table_db(name), **LOW)
    ns = S.field_major_index_sets(spec)[0].size
    probe = K._handle(spec, params, db)
    probe.create_solver()
    mask = probe.reuse_rows()
    assert probe.reuse_stats()[2] == 1
    probe.destroy()
    print(f"reuse rows {int(mask.sum())} of {n - ns} fp rows")
    assert mask.any() and not mask[:ns].any()
    ref = _reference(spec, params, db, name=name, mask=mask, ns=ns)
    h, x, r, hist = T._device(spec, params, db, ref)
    _check_stats(h, ref, "global_", restart)
    its, cycles = ref["its"], ref["first"][0][5]
    assert h.reuse_stats() == (its, cycles, 1)  # every in-cycle product reduced, the cycle starts full
    _true_last_entry(ref, x, hist, side)
    _low_path_ran(spec, params, db, ref["b"], hist)
    # and the mixed operator is not fl32(A): the pure restatement's history differs
    pure = _reference(spec, params, db, name=name)
    m = min(pure["ho"].size, hist.size)
    assert np.max(np.abs(pure["ho"][:m] - hist[:m]) / hist[:m]) > ref["tol"]


# ----------------------------------------------------------- 3. fgmres ----
def test_fgmres(gpu):
    spec = S.SynthSpec(2, 12)
    db = dict(K.FGMRES_DB, **LOW, **NO_REUSE)
    ref = _reference(spec, K.BASE, db, flexible=True)
    h, x, r, hist = T._device(spec, K.BASE, db, ref)
    _check_stats(h, ref, "global_", 300)
    assert r.pc_applies == r.its
    _true_last_entry(ref, x, hist, "right")
    _low_path_ran(spec, K.BASE, db, ref["b"], hist)


# ----------------------------------------------------- 4. inner prefix ----
def test_inner_s_gmres(gpu):
    """s_ksp_type gmres (left, Jacobi, rtol 1e-3) with the low operator on the 8,450-row s block of
    2-D N=32 3-way under outer fgmres (double): the block's own matrix carries the fp32 stream."""
    spec = S.SynthSpec(2, 32)
    params = dict(K.BASE, **{"pc type": "diagonal 3-way", "solver maxiter": 4})
    db = dict(K.FGMRES_DB, s_ksp_type="gmres", s_pc_type="jacobi", s_ksp_rtol="1e-3", s_ksp_max_it="30",
              s_pls_gmres_basis="single", s_pls_gmres_operator="single")
    ref = _reference(spec, params, db, target="ksp_s")
    assert ref["n"] == 8450
    solves, its = len(ref["first"]), sum(e[0] for e in ref["first"])
    assert its > solves
    h, _, _, hist = T._device(spec, params, db, ref)
    st = h.ksp_stats("s_")
    assert st[0] == solves and st[1] == its
    _check_stats(h, ref, "s_", 30)
    assert h.gmres_operator_stats("global_")[:3] == (0, 0, 0)


# ---------------------------------------------------------- 5. refusals ----
@pytest.mark.parametrize("extra,match", [
    ({"global_pls_gmres_operator": "single"}, "global_pls_gmres_operator single requires global_pls_gmres_basis single"),
    ({"global_pls_gmres_operator": "single", "global_pls_gmres_basis": "double"},
     "global_pls_gmres_operator single requires global_pls_gmres_basis single"),
    (dict(LOW, global_pls_gmres_operator="half"), "global_pls_gmres_operator.*'half'.*double, single"),
    (dict(LOW, **{"pls.sell_d16": "0"}), "global_pls_gmres_operator single.*int32 SELL-64"),
    ({"s_ksp_type": "gmres", "s_pls_gmres_basis": "single", "s_pls_gmres_operator": "single", "pls.sell_d16": "0"},
     "s_pls_gmres_operator single.*int32 SELL-64"),
])
def test_refusals(gpu, extra, match):
    spec = S.SynthSpec(2, 4)
    with pytest.raises(RuntimeError, match=match):
        h = K._handle(spec, G.PARAMS, dict(G.table_db("2d12_right"), **extra))
        h.create_solver()


def test_refused_on_a_b3_layout(gpu):
    """pls.spmv_b3 1 on a pattern of row triples: the outer operator keeps a B3 part."""
    from lib.handle import Handle, params_to_options
    case = C.BY_ID["b3-mixed"]
    A, _ = C.matrix(case, "normal")
    n = A.shape[0]
    A = (A + 50.0 * sp.identity(n)).tocsr()
    is_s, is_f, is_p, _ = C.index_sets(case, n)
    opts = dict(G.table_db("2d12_right"), **LOW, **case.options)
    opts.update(params_to_options(G.PARAMS))
    h = Handle.from_csr(A, sp.identity(n, format="csr"), None, is_s, is_f, is_p, [], opts)
    try:
        with pytest.raises(RuntimeError, match="global_pls_gmres_operator single.*SELL/B3"):
            h.create_solver()
    finally:
        h.destroy()


def test_other_types_ignore_the_option_and_have_no_stats(gpu):
    spec = S.SynthSpec(2, 4)
    db = dict(G.BLOCKS_ILU, global_ksp_type="bcgs", global_pls_gmres_operator="half")
    h = K._handle(spec, K.BASE, db)
    _, r = h.solve(S.rhs(spec))
    assert r.reason > 0
    with pytest.raises(RuntimeError, match="not gmres or fgmres"):
        h.gmres_operator_stats("global_")
    with pytest.raises(RuntimeError, match="no inner solver with prefix 'nope_'"):
        h.gmres_operator_stats("nope_")
