"""Coupling reuse (option pls.reuse_coupling, DESIGN.md "Coupling reuse"): in
right-preconditioned GMRES / FGMRES the outer product w = A z continues the raw
row sums of the 2-way block PC's product P_fp,s z_s instead of reading A_fp,s
again.  The reduced product is the full one's chain of operations per row, so
everything here is compared bitwise (np.array_equal; a sum that is exactly zero
may differ in sign, which array_equal does not see).

Shapes: synthetic 3-D N=6 (13,525 rows: lane-per-row s / f rows and 8-lane
pressure rows) and 2-D N=8 (1,237 rows, the recorded goldens' shape),
BJACOBI(ILU(0)) with 4 blocks per inner PC.  4 blocks never engage the fp
pipeline (it needs 8), so one more case runs 3-D N=16 with 24 blocks, where the
pipeline engages (as in test_gpu_sweeps.test_fp_pipeline_bitwise).
"""
import numpy as np
import pytest

from oracle import synthetic as S

pytestmark = pytest.mark.gpu

PARAMS = {"solver type": "gmres", "solver atol": 1e-8, "solver rtol": 1e-6, "solver maxiter": 200,
          "pc type": "diagonal", "inner ksp type": "preonly", "inner pc type": "ilu", "inner rtol": 1e-6,
          "inner atol": 0, "inner maxiter": 1000, "inner monitor": False, "solver monitor": False,
          "inner accel order": 0, "AAR order": 10, "AAR p": 5, "AAR omega": 1, "AAR beta": 1}
SHAPES = [(3, 6), (2, 8)]


def _db(blocks=4, three_way=False, right=True):
    db = {"global_ksp_pc_side": "right"} if right else {}
    for pre in (("s_", "f_", "p_", "diff_") if three_way else ("s_", "fp_")):
        db[pre + "ksp_type"] = "preonly"
        db[pre + "pc_type"] = "bjacobi"
        db[pre + "pc_bjacobi_blocks"] = str(blocks)
    return db


def _options(db, params, reuse, extra=None):
    from lib.handle import params_to_options
    opts = dict(db, **(extra or {}))
    if reuse is not None:
        opts["pls.reuse_coupling"] = str(reuse)
    opts.update(params_to_options(params))
    return opts


def _rhs(n):
    return np.random.default_rng(8).standard_normal(n)


def _solve(h, b):
    """(x, its, reason, history, reuse stats of this solve)"""
    h.create_solver()
    h.reset_timings()
    x, r = h.solve(b)
    return x, r.its, r.reason, h.history().copy(), h.reuse_stats()


def _same(a, b):
    assert a[1] == b[1] and a[2] == b[2], (a[1:3], b[1:3])
    assert np.array_equal(a[3], b[3])
    assert np.array_equal(a[0], b[0])


def _on_equals_off(spec, params, db, restart, extra=None):
    from lib.handle import Handle
    b = _rhs(spec.n)
    out = {}
    for reuse in (1, 0):
        h = Handle.synthetic(spec.dim, spec.N, spec.seed, spec.delta, _options(db, params, reuse, extra))
        out[reuse] = _solve(h, b)
        h.destroy()
    on, off = out[1], out[0]
    print("its", on[1], "reason", on[2], "stats on", on[4], "off", off[4])
    _same(on, off)
    its = on[1]
    assert its > 0
    # every Arnoldi step forms one product after a PC application (reduced); every cycle but
    # the first starts with the residual b - A x (full): ceil(its / restart) cycles
    cycles = -(-its // restart)
    assert on[4] == (its, cycles - 1, 1)
    assert off[4] == (0, its + cycles - 1, 0)
    return on


@pytest.mark.parametrize("restart,maxit", [(100, 200), (5, 40)])
@pytest.mark.parametrize("pipeline", ["1", "0"])
@pytest.mark.parametrize("ksp", ["gmres", "fgmres"])
@pytest.mark.parametrize("dim,N", SHAPES)
def test_on_equals_off_bitwise(gpu, dim, N, ksp, pipeline, restart, maxit):
    """pls.reuse_coupling 1 == 0: x, history, its, reason; and the reduced path ran (stats).
    With restart 5 the full-A residual and the reduced product alternate within one solve."""
    params = dict(PARAMS, **{"solver type": ksp, "solver maxiter": maxit})
    db = dict(_db(), global_ksp_gmres_restart=str(restart))
    on = _on_equals_off(S.SynthSpec(dim, N), params, db, restart, {"pls.fp_pipeline": pipeline})
    if restart == 5:
        assert on[4][1] >= 1  # the two kinds of product did alternate


def test_on_equals_off_fp_pipeline_engaged(gpu, capfd):
    """The same with the pressure-first pipeline engaged (24 blocks at 3-D N=16): both of its
    coupling launches store their raw sums, on two streams."""
    params = dict(PARAMS, **{"solver maxiter": 200})
    db = dict(_db(blocks=24), global_ksp_gmres_restart="200")
    capfd.readouterr()
    _on_equals_off(S.SynthSpec(3, 16), params, db, 200, {"pls.fp_pipeline": "1", "pls.ilu_view": "1"})
    assert "[pls fp pipeline]" in capfd.readouterr().err


@pytest.mark.parametrize("dim,N", SHAPES)
def test_reduced_product_equals_full(gpu, dim, N):
    """After pls_pc_apply_device, the reduced product of the returned z == pls_matmult_device(z).
    pls.reuse_coupling_probe 1 lets pls_matmult_device form the product as GMRES does after a PC
    application: the first call continues the PC's sums (reduced), the second finds them used."""
    from lib.handle import Handle
    spec = S.SynthSpec(dim, N)
    h = Handle.synthetic(spec.dim, spec.N, spec.seed, spec.delta,
                         _options(_db(), PARAMS, 1, {"pls.reuse_coupling_probe": "1"}))
    h.create_solver()
    d = [gpu.DeviceArray(spec.n) for _ in range(4)]
    d[0].upload(_rhs(spec.n))
    h.pc_apply_device(d[0].p, d[1].p)
    h.reset_timings()
    h.matmult_device(d[1].p, d[2].p)
    assert h.reuse_stats() == (1, 0, 1)
    h.matmult_device(d[1].p, d[3].p)
    assert h.reuse_stats() == (1, 1, 1)
    reduced, full = d[2].download(), d[3].download()
    # the probe's full product is the plain entry point's
    h0 = Handle.synthetic(spec.dim, spec.N, spec.seed, spec.delta, _options(_db(), PARAMS, 0))
    h0.matmult_device(d[1].p, d[0].p)
    plain = d[0].download()
    assert np.any(full != 0.0)
    assert np.array_equal(full, plain)
    assert np.array_equal(reduced, full)
    h.destroy()
    h0.destroy()


def _csr_system(spec, scale_coupling=1.0):
    """(A, P with its fp x s block scaled, index sets, bcs) in field-major order"""
    import scipy.sparse as sp
    A, P = S.matrix(spec, 0), S.matrix(spec, 1)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    ns = len(is_s)
    if scale_coupling != 1.0:
        C = P.tocoo()
        v = C.data.copy()
        v[(C.row >= ns) & (C.col < ns)] *= scale_coupling
        P = sp.csr_matrix((v, (C.row, C.col)), shape=P.shape)
    return A, P, is_s, is_f, is_p, S.bcs_sub_pressure(spec)


def _fallback(make, b):
    """auto: not eligible; == pls.reuse_coupling 0 bitwise; pls.reuse_coupling 1 throws"""
    out = {}
    for reuse in (None, 0):
        h = make(reuse)
        out[reuse] = _solve(h, b)
        h.destroy()
    assert out[None][4][0] == 0 and out[None][4][2] == 0, out[None][4]
    assert out[0][4][0] == 0 and out[0][4][2] == 0
    _same(out[None], out[0])
    h = make(1)
    with pytest.raises(RuntimeError, match="reuse_coupling"):
        h.solve(b)
    h.destroy()


@pytest.mark.parametrize("case", ["scaled P", "3-way", "left", "inner accel", "aar"])
def test_fallbacks(gpu, case):
    from lib.handle import Handle
    spec = S.SynthSpec(3, 6)
    b = _rhs(spec.n)
    params, db = dict(PARAMS), _db()
    if case == "3-way":
        params["pc type"], db = "diagonal 3-way", _db(three_way=True)
    elif case == "left":
        db = _db(right=False)
    elif case == "inner accel":
        params["inner accel order"] = 1
    elif case == "aar":
        params["solver type"] = "aar"
    if case == "scaled P":
        A, P, is_s, is_f, is_p, bcs = _csr_system(spec, 1.25)

        def make(reuse):
            return Handle.from_csr(A, P, None, is_s, is_f, is_p, bcs, _options(db, params, reuse))
    else:
        def make(reuse):
            return Handle.synthetic(spec.dim, spec.N, spec.seed, spec.delta, _options(db, params, reuse))
    _fallback(make, b)


def test_update_matrices_switches_eligibility(gpu):
    """A solve, pls_update_matrices with 1.25 P, a solve: eligible 1 -> 0; back to P: eligible
    again, and the solve is bitwise the first one."""
    from lib.handle import Handle
    spec = S.SynthSpec(3, 6)
    b = _rhs(spec.n)
    A, P, is_s, is_f, is_p, bcs = _csr_system(spec)
    P125 = (1.25 * P).tocsr()
    h = Handle.from_csr(A, P, None, is_s, is_f, is_p, bcs, _options(_db(), PARAMS, None))
    first = _solve(h, b)
    assert first[4] == (first[1], 0, 1)
    h.update_matrices(P=P125)
    second = _solve(h, b)
    assert second[4][0] == 0 and second[4][2] == 0
    h.update_matrices(P=P)
    third = _solve(h, b)
    assert third[4] == (third[1], 0, 1)
    _same(first, third)
    h.destroy()
