"""The numpy restatement of compressed-operator GMRES
(tests/co_gmres_restatement.py) pinned on the CPU: with the fp64 product as the
low one it is ``cb_gmres_restatement.gmres`` bit for bit; with A^ = fl32(A) the
iteration counts, history lengths and rule counters of the cases the device
tests use (tests/test_gpu_co_gmres.py) are the ones recorded when it was
written; the last history entry is the true residual of the fp64 operator; at
rtol 1e-6 the low operator costs no iteration; and no decision of rule (a) or
rule (b) is borderline."""
import os

import numpy as np
import pytest

import cb_gmres_restatement as CB
import co_gmres_restatement as CO
import gmres_orthog_restatement as G
from oracle import petsc
from oracle import synthetic as S
from oracle.solver import OracleSolver


def oracle(spec, params, db):
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    return A, OracleSolver(A, P, Pd, is_s, is_f, is_p, params, db, S.bcs_sub_pressure(spec))


def true_residual(A, o, b, x, side):
    r = b - A @ x
    return float(np.linalg.norm(r if side == "right" else o.pc.apply(r)))


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", ["2d12_left", "2d12_right_restart5"])
def test_fp64_low_product_is_the_cb_restatement_bitwise(name, rtol):
    dim, N = G.TABLE[name][:2]
    spec = S.SynthSpec(dim, N)
    b = S.rhs(spec)
    _, o = oracle(spec, dict(G.PARAMS, **{"solver rtol": rtol}), G.table_db(name))
    ksp = o.solver
    xc = CB.gmres(ksp, b)
    want = (ksp.its, ksp.reason, list(ksp.history), ksp.cb_forced, ksp.cb_confirm, ksp.cb_failed, list(ksp.cb_ratios),
            ksp.orthog_steps)
    x = CO.gmres(ksp, b, ksp.matvec)
    got = (ksp.its, ksp.reason, list(ksp.history), ksp.cb_forced, ksp.cb_confirm, ksp.cb_failed, list(ksp.cb_ratios),
           ksp.orthog_steps)
    assert got == want
    assert np.array_equal(x, xc)
    assert ksp.co_low == ksp.its and ksp.co_double == len(ksp.history) - ksp.its - 1


def test_library_and_handle_carry_the_interface():
    """What the device tests drive, present without a GPU: the entry points in libpls.so and
    include/pls.h, and their Handle methods."""
    import lib._native as N
    from lib.handle import Handle
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pls.h")).read()
    L = N.lib()
    for sym in ("pls_matmult_single", "pls_matmult_single_device", "pls_spmv_layout_single", "pls_bench_spmv_single",
                "pls_get_gmres_operator_stats", "pls_get_reuse_rows"):
        assert hasattr(L, sym) and sym in N.EXPORTS and f"int {sym}(" in header, sym
    for method in ("matmult_single", "matmult_single_device", "spmv_layout_single", "bench_spmv_single",
                   "gmres_operator_stats", "reuse_rows"):
        assert callable(getattr(Handle, method)), method


def test_low_matrix_rounds_every_value_but_the_reuse_rows_coupling():
    spec = S.SynthSpec(2, 4)
    A = S.matrix(spec, 0).tocsr()
    ns = S.field_major_index_sets(spec)[0].size
    L = CO.low_matrix(A)
    assert np.array_equal(L.indptr, A.indptr) and np.array_equal(L.indices, A.indices)
    assert np.array_equal(L.data, A.data.astype(np.float32).astype(np.float64))
    assert np.any(L.data != A.data)
    mask = np.zeros(spec.n, dtype=np.uint8)
    mask[ns::2] = 1
    M = CO.low_matrix(A, mask, ns)
    rows = np.repeat(np.arange(spec.n), np.diff(A.indptr))
    keep = (mask[rows] == 1) & (A.indices < ns)
    assert keep.any()
    assert np.array_equal(M.data[keep], A.data[keep]) and np.array_equal(M.data[~keep], L.data[~keep])


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", sorted(G.TABLE))
def test_recorded_table_true_last_entry_and_no_borderline_decision(name, rtol):
    """its / history entries / rule counters as recorded (the cb restatement's
    except 3d4_right at 1e-10); one low product per step and one fp64 product
    per later cycle start; the last history entry is the true residual norm of
    the fp64 operator to 1e-12 relative; no decision is borderline."""
    dim, N, side, restart, n = G.TABLE[name][:5]
    spec = S.SynthSpec(dim, N)
    assert spec.n == n
    b = S.rhs(spec)
    A, o = oracle(spec, dict(G.PARAMS, **{"solver rtol": rtol}), G.table_db(name))
    ksp = o.solver
    petsc._gmres(ksp, b)
    double_its = ksp.its
    A_low = CO.low_matrix(A)
    x = CO.gmres(ksp, b, lambda v: A_low @ v)
    got = (ksp.its, len(ksp.history), ksp.cb_forced, ksp.cb_confirm, ksp.cb_failed)
    true = true_residual(A, o, b, x, side)
    print(f"{name} rtol {rtol:g}: double its {double_its}, low operator {got}; products low {ksp.co_low} "
          f"double {ksp.co_double}; estimate {ksp.history[-2]:.6e} last {ksp.history[-1]:.6e} true {true:.6e}; "
          f"confirmations (true, estimate) / threshold {ksp.co_confirm}")
    assert ksp.reason == 2
    assert got == CO.RECORDED[name][rtol]
    if not (name == "3d4_right" and rtol == 1e-10):
        assert got == CB.RECORDED[name][rtol]
    assert ksp.co_low == ksp.its
    assert ksp.co_double == len(ksp.history) - ksp.its - 1
    assert abs(ksp.history[-1] - true) <= 1e-12 * true
    CB.check_ratios(name, ksp.cb_ratios)
    assert len(ksp.co_confirm) == ksp.cb_confirm
    CO.check_confirmations(name, ksp.co_confirm)
    if rtol == 1e-6:
        assert ksp.its == double_its  # no cost in iterations at the reference drivers' tolerance
