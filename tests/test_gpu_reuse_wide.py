"""Coupling reuse on rows served by several lanes (option pls.reuse_wide, DESIGN.md "Coupling
reuse"): the block PC's coupling launches store the raw sum of every lane of a wide row before the
shuffle combine, and the reduced outer launch starts each lane from it.  A' leaves the rows'
s-columns out and keeps every remaining entry on the lane it has in A (the phase rule), so each
lane's chain of operations is the full product's and everything here is compared bitwise.

Hand-built systems (tests/reuse_wide_restatement.py, pinned on the CPU by
tests/test_reuse_wide_restatement.py): wide groups beside a lane-per-row group and a final partial
group, s-part lengths over every residue mod 8, empty and short s-parts, a row without fp columns;
ns = 1160 cuts A's 64-row groups 8 rows off the coupling block's, ns = 1152 cuts them alike.  The
inner PCs are jacobi (s) and none (fp): a row without a diagonal has no ILU factor, and the PC's
quality does not matter to the product.

Synthetic 3-D N=6 (13,525 rows; 8-lane pressure rows, ns / np ~ 19): solves with pls.reuse_wide
-1 against 0, as tests/test_gpu_coupling_reuse.py compares pls.reuse_coupling 1 against 0; one case
at 3-D N=16 with 24 blocks, where the fp pipeline engages and its heavy slices are the wide rows.
"""
import numpy as np
import pytest

import reuse_wide_restatement as W
from oracle import synthetic as S

pytestmark = pytest.mark.gpu

PARAMS = {"solver type": "gmres", "solver atol": 1e-8, "solver rtol": 1e-6, "solver maxiter": 200,
          "pc type": "diagonal", "inner ksp type": "preonly", "inner pc type": "ilu", "inner rtol": 1e-6,
          "inner atol": 0, "inner maxiter": 1000, "inner monitor": False, "solver monitor": False,
          "inner accel order": 0, "AAR order": 10, "AAR p": 5, "AAR omega": 1, "AAR beta": 1}


# ------------------------------------------------------------- hand-built systems --
def _hand_options(wide):
    from lib.handle import params_to_options
    opts = {"global_ksp_pc_side": "right", "s_ksp_type": "preonly", "s_pc_type": "jacobi",
            "fp_ksp_type": "preonly", "fp_pc_type": "none", "pls.d16_share": "0",
            "pls.reuse_coupling": "1", "pls.reuse_coupling_probe": "1", "pls.reuse_wide": str(wide)}
    opts.update(W.OPTIONS)
    opts.update(params_to_options(PARAMS))
    return opts


def _hand_products(gpu, A, ns, nf, np_, wide):
    """(z, reduced A z, full A z, reuse_wide()) of one handle"""
    from lib.handle import Handle
    n = A.shape[0]
    is_s, is_f, is_p = np.arange(ns), ns + np.arange(nf), ns + nf + np.arange(np_)
    h = Handle.from_csr(A, A, None, is_s, is_f, is_p, [], _hand_options(wide))
    try:
        h.create_solver()
        assert np.array_equal(h.permutation(), np.arange(n))  # the library's rows are the restatement's
        d = [gpu.DeviceArray(n) for _ in range(4)]
        d[0].upload(np.random.default_rng(8).standard_normal(n))
        h.pc_apply_device(d[0].p, d[1].p)
        h.reset_timings()
        h.matmult_device(d[1].p, d[2].p)
        assert h.reuse_stats() == (1, 0, 1)
        h.matmult_device(d[1].p, d[3].p)
        assert h.reuse_stats() == (1, 1, 1)
        out = d[1].download(), d[2].download(), d[3].download(), h.reuse_wide()
        for a in d:
            a.free()
    finally:
        h.destroy()
    return out


@pytest.mark.parametrize("ns", [1160, 1152])
def test_hand_built_reduced_product(gpu, ns):
    """The reduced product after a PC application == pls_matmult_device, bitwise; pls.reuse_wide 0
    == -1; the kinds of reuse rows and the bytes of A' are the restatement's for both settings."""
    A, ns, nf, np_ = W.wide_system(ns)
    z1, red1, full1, st1 = _hand_products(gpu, A, ns, nf, np_, -1)
    z0, red0, full0, st0 = _hand_products(gpu, A, ns, nf, np_, 0)
    R1, R0 = W.reduced(A, ns), W.reduced(A, ns, reuse_wide=False)
    print(f"ns {ns}: reuse_wide() on {st1} off {st0}; restated on "
          f"{(R1.wide_rows, 8, R1.lane_rows, R1.bytes)} off {(0, 0, R0.lane_rows, R0.bytes)}")
    assert np.array_equal(z1, z0) and np.all(np.isfinite(z1)) and np.any(z1[:ns] != 0.0)
    assert np.any(full1 != 0.0) and np.array_equal(full1, full0)
    # (against scipy's order of the sums: rows of <= 90 entries of size O(10): 90 eps * 1e3 ~ 2e-11)
    assert np.allclose(full1, A @ z1, rtol=0.0, atol=1e-10)
    assert np.array_equal(red1, full1)
    assert np.array_equal(red0, full0)
    assert np.array_equal(red1, red0)
    assert R1.wide_rows > 0 and R1.stored < R0.stored
    assert st1 == (R1.wide_rows, 8, R1.lane_rows, R1.bytes)
    assert st0 == (0, 0, R0.lane_rows, R0.bytes)


# ------------------------------------------------------------------ synthetic solves --
def _db(blocks=4):
    db = {"global_ksp_pc_side": "right"}
    for pre in ("s_", "fp_"):
        db.update({pre + "ksp_type": "preonly", pre + "pc_type": "bjacobi", pre + "pc_bjacobi_blocks": str(blocks)})
    return db


def _options(db, params, wide, extra=None):
    from lib.handle import params_to_options
    opts = dict(db, **(extra or {}))
    opts.update({"pls.reuse_coupling": "1", "pls.reuse_wide": str(wide)})
    opts.update(params_to_options(params))
    return opts


def _rhs(n):
    return np.random.default_rng(8).standard_normal(n)


def _solve(h, b):
    """(x, its, reason, history, reuse stats of this solve, reuse_wide(), d16_share of A')"""
    h.create_solver()
    h.reset_timings()
    x, r = h.solve(b)
    return x, r.its, r.reason, h.history().copy(), h.reuse_stats(), h.reuse_wide(), h.d16_share(1)


def _same(a, b):
    assert a[1] == b[1] and a[2] == b[2], (a[1:3], b[1:3])
    assert np.array_equal(a[3], b[3])
    assert np.array_equal(a[0], b[0])


def _paths_ran(on, off, restart):
    """The counters: both solves took the reduced product; only `on` has wide reuse rows, and
    its A' stores fewer entries."""
    its = on[1]
    assert its > 0
    cycles = -(-its // restart)
    assert on[4] == (its, cycles - 1, 1) and off[4] == on[4]
    assert on[5][0] > 0 and on[5][1] == 8 and off[5][:2] == (0, 0)
    assert on[5][2] == off[5][2] > 0          # the lane-per-row reuse rows do not change
    assert on[5][3] < off[5][3]               # bytes of A'
    assert on[6][1] == off[6][1]              # the same slices


def _on_equals_off(spec, params, db, restart, extra=None):
    from lib.handle import Handle
    b = _rhs(spec.n)
    out = {}
    for wide in (-1, 0):
        h = Handle.synthetic(spec.dim, spec.N, spec.seed, spec.delta, _options(db, params, wide, extra))
        out[wide] = _solve(h, b)
        h.destroy()
    on, off = out[-1], out[0]
    print("its", on[1], "reason", on[2], "stats", on[4], "reuse_wide on", on[5], "off", off[5])
    _same(on, off)
    _paths_ran(on, off, restart)
    return on


@pytest.mark.parametrize("pipeline", ["1", "0"])
@pytest.mark.parametrize("ksp", ["gmres", "fgmres"])
def test_on_equals_off_bitwise(gpu, ksp, pipeline):
    params = dict(PARAMS, **{"solver type": ksp})
    db = dict(_db(), global_ksp_gmres_restart="100")
    _on_equals_off(S.SynthSpec(3, 6), params, db, 100, {"pls.fp_pipeline": pipeline})


def test_on_equals_off_across_restarts(gpu):
    """restart 5: the full-A residual and the reduced product alternate within one solve"""
    params = dict(PARAMS, **{"solver maxiter": 40})
    db = dict(_db(), global_ksp_gmres_restart="5")
    on = _on_equals_off(S.SynthSpec(3, 6), params, db, 5)
    assert on[4][1] >= 1


@pytest.mark.parametrize("share", ["0", "1"])
def test_on_equals_off_with_shared_deltas(gpu, share):
    """The shared delta stream is built from the filled plain stream, phase rule included."""
    db = dict(_db(), global_ksp_gmres_restart="100")
    on = _on_equals_off(S.SynthSpec(3, 6), PARAMS, db, 100, {"pls.d16_share": share})
    assert on[6][0] == int(share)


def test_on_equals_off_fp_pipeline_engaged(gpu, capfd):
    """24 blocks at 3-D N=16: the fp pipeline engages, and its heavy launch covers the 8-lane
    pressure slices -- the per-lane sums are stored by two launches on two streams."""
    db = dict(_db(blocks=24), global_ksp_gmres_restart="200")
    capfd.readouterr()
    _on_equals_off(S.SynthSpec(3, 16), PARAMS, db, 200, {"pls.fp_pipeline": "1", "pls.ilu_view": "1"})
    assert "[pls fp pipeline]" in capfd.readouterr().err


def test_on_equals_off_after_update_matrices(gpu):
    """pls_update_matrices rebuilds A' and the per-lane sums' buffer; the next solve is bitwise the
    one without wide reuse rows, and not the first solve's."""
    from lib.handle import Handle
    spec = S.SynthSpec(3, 6)
    A, P = S.matrix(spec, 0), S.matrix(spec, 1)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    bcs = S.bcs_sub_pressure(spec)
    A2, P2 = (1.5 * A).tocsr(), (1.5 * P).tocsr()
    b = _rhs(spec.n)
    db = dict(_db(), global_ksp_gmres_restart="100")
    out = {}
    for wide in (-1, 0):
        h = Handle.from_csr(A, P, None, is_s, is_f, is_p, bcs, _options(db, PARAMS, wide))
        first = _solve(h, b)
        h.update_matrices(A=A2, P=P2)
        out[wide] = (first, _solve(h, b))
        h.destroy()
    for k in (0, 1):
        _same(out[-1][k], out[0][k])
        _paths_ran(out[-1][k], out[0][k], 100)
    assert not np.array_equal(out[-1][0][0], out[-1][1][0])
