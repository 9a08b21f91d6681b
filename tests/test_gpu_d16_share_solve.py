"""Solves over shared delta streams (option pls.d16_share): every D16 layout of the handle -- the
outer operator A, its reduced layout A' of the coupling reuse, the inner blocks and the block
PC's coupling block -- built with pls.d16_share 1 against 0.  The shared stream decodes to the
same columns, and the values and the order of the sums do not change, so x, the residual history,
the iteration count and the reason are compared bitwise.

Shape: synthetic 3-D N=6 (13,525 rows: lane-per-row s / f rows and 8-lane pressure rows), right-
preconditioned GMRES, 2-way block PC, BJACOBI(ILU(0)) with 4 blocks per inner PC, as in
tests/test_gpu_coupling_reuse.py.  pls.reuse_coupling 1 runs the slice-list launches and the raw-sum
store / initial value (D16_AUX_STORE / D16_AUX_INIT) over shared streams; the reuse counters prove
the reduced path ran and ``d16_share(1)`` that A' has a shared stream.
"""
import numpy as np
import pytest

from oracle import synthetic as S

pytestmark = pytest.mark.gpu

PARAMS = {"solver type": "gmres", "solver atol": 1e-8, "solver rtol": 1e-6, "solver maxiter": 200,
          "pc type": "diagonal", "inner ksp type": "preonly", "inner pc type": "ilu", "inner rtol": 1e-6,
          "inner atol": 0, "inner maxiter": 1000, "inner monitor": False, "solver monitor": False,
          "inner accel order": 0, "AAR order": 10, "AAR p": 5, "AAR omega": 1, "AAR beta": 1}
SPEC = S.SynthSpec(3, 6)


def _options(share, reuse, pipeline="1", extra=None):
    from lib.handle import params_to_options
    opts = {"global_ksp_pc_side": "right", "global_ksp_gmres_restart": "100"}
    for pre in ("s_", "fp_"):
        opts.update({pre + "ksp_type": "preonly", pre + "pc_type": "bjacobi", pre + "pc_bjacobi_blocks": "4"})
    opts.update({"pls.d16_share": str(share), "pls.reuse_coupling": str(reuse), "pls.fp_pipeline": pipeline})
    opts.update(extra or {})
    opts.update(params_to_options(PARAMS))
    return opts


def _rhs():
    return np.random.default_rng(8).standard_normal(SPEC.n)


def _solve(h, b):
    """(x, its, reason, history, reuse stats, d16_share of A, of A')"""
    h.create_solver()
    h.reset_timings()
    x, r = h.solve(b)
    return x, r.its, r.reason, h.history().copy(), h.reuse_stats(), h.d16_share(0), h.d16_share(1)


def _same(a, b):
    assert a[1] == b[1] and a[2] == b[2], (a[1:3], b[1:3])
    assert np.array_equal(a[3], b[3])
    assert np.array_equal(a[0], b[0])


@pytest.mark.parametrize("pipeline", ["1", "0"])
@pytest.mark.parametrize("reuse", [1, 0])
def test_share_equals_plain_bitwise(gpu, reuse, pipeline):
    from lib.handle import Handle
    b = _rhs()
    out = {}
    for share in (1, 0):
        h = Handle.synthetic(SPEC.dim, SPEC.N, SPEC.seed, SPEC.delta, _options(share, reuse, pipeline))
        out[share] = _solve(h, b)
        h.destroy()
    on, off = out[1], out[0]
    print("its", on[1], "reason", on[2], "reuse", on[4], "d16_share A", on[5], "A'", on[6], "plain", off[5], off[6])
    _same(on, off)
    assert on[1] > 0 and on[4] == off[4]
    assert on[4] == ((on[1], 0, 1) if reuse else (0, on[1], 0))
    assert on[5][0] == 1 and on[5][2] > 0 and on[5][3] < off[5][3]
    assert off[5][0] == 0 and off[5][4] == 0
    assert on[5][4] >= 1 + reuse  # layouts built with a shared stream: A at least, and A' with the reuse
    if reuse:
        assert on[6][0] == 1 and on[6][1] == on[5][1] and on[6][3] < off[6][3]
        assert off[6][0] == 0 and off[6][1] == off[5][1]


def test_after_update_matrices(gpu):
    """The layouts are built again after pls_update_matrices, shared again, and the solve is bitwise
    the plain one's."""
    from lib.handle import Handle
    A, P = S.matrix(SPEC, 0), S.matrix(SPEC, 1)
    is_s, is_f, is_p = S.field_major_index_sets(SPEC)
    bcs = S.bcs_sub_pressure(SPEC)
    A2, P2 = (1.5 * A).tocsr(), (1.5 * P).tocsr()
    b = _rhs()
    out = {}
    for share in (1, 0):
        h = Handle.from_csr(A, P, None, is_s, is_f, is_p, bcs, _options(share, 1))
        first = _solve(h, b)
        h.update_matrices(A=A2, P=P2)
        out[share] = (first, _solve(h, b))
        h.destroy()
    for k in (0, 1):
        _same(out[1][k], out[0][k])
        assert out[1][k][4] == (out[1][k][1], 0, 1)
        assert out[1][k][5][0] == 1 and out[1][k][6][0] == 1 and out[0][k][5][0] == 0
    assert out[1][1][5][4] > out[1][0][5][4]  # layouts were built with a shared stream once more
    assert not np.array_equal(out[1][0][0], out[1][1][0])


def test_auto_rule_in_a_solve(gpu):
    """pls.d16_share -1 with pls.d16_share_min_bytes 1 engages on A and A' (their shared layouts
    are smaller); with the default threshold it leaves them as they are.  Bitwise the same solve."""
    from lib.handle import Handle
    b = _rhs()
    h = Handle.synthetic(SPEC.dim, SPEC.N, SPEC.seed, SPEC.delta,
                         _options(-1, 1, extra={"pls.d16_share_min_bytes": "1"}))
    auto = _solve(h, b)
    lay_auto = h.spmv_layout()
    h.destroy()
    h = Handle.synthetic(SPEC.dim, SPEC.N, SPEC.seed, SPEC.delta, _options(-1, 1))
    default = _solve(h, b)
    lay_default = h.spmv_layout()
    h.destroy()
    print("auto", auto[5], auto[6], lay_auto, "default", default[5], default[6], lay_default)
    _same(auto, default)
    assert auto[5][0] == 1 and auto[6][0] == 1 and lay_auto[1] < lay_default[1]
    assert default[5][0] == 0 and default[6][0] == 0 and default[5][4] == 0
