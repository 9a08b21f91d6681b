"""Compressed-basis GMRES (``global_pls_gmres_basis single``) in the outer gmres
on two ranks (sharing the box's one GPU through the host-staged communicator)
against ``OracleSolver(dist_size=2)`` with the numpy restatement
(tests/cb_gmres_restatement.py) installed as its ``solver.solve``: the rounding
to fp32 is local to a rank and the sums go through the global sum, so nothing
but the rank-ordered sums differs from one rank.  2-D N=12, right, at rtol 1e-6
and 1e-10.  Built as tests/test_dist_gpu_gmres_orthog.py is: the block options
of the first case of tests/test_dist_gpu.py.  The bar is the one of
tests/test_gpu_cb_gmres.py: iteration count, reason and history length exact on
every rank, every history entry within max(1e-10, 10 x the restatement's own
deviation under 1e-15 perturbations of the inner PC outputs, 4 seeds), the
assembled solution within max(1e-8, that bound).  The ranks' history length is
its + 1 + forced cycle ends + confirmations, so it pins the rule counters of
the restatement, asserted here to be the recorded ones."""
import numpy as np
import pytest

import cb_gmres_restatement as CB
import test_dist_gpu as T
import test_gpu_ksp_types as K
from distutil import launch

pytestmark = pytest.mark.gpu

_BLOCKS = {k: v for k, v in T.CASES[0]["db"].items() if not k.startswith("global_")}
_OUTER = dict(_BLOCKS, global_ksp_type="gmres", global_ksp_pc_side="right", global_pls_gmres_basis="single")
CASES = [
    {"name": "cb_gmres_rtol6_2d", "dim": 2, "N": 12, "db": _OUTER,
     "params": dict(T.BASE, **{"solver rtol": 1e-6, "solver atol": 0}), "counters": (0, 1, 0)},
    {"name": "cb_gmres_rtol10_2d", "dim": 2, "N": 12, "db": _OUTER,
     "params": dict(T.BASE, **{"solver rtol": 1e-10, "solver atol": 0}), "counters": (1, 1, 0)},
]


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    return 2, launch("gpu", CASES, 2, str(tmp_path_factory.mktemp("dist_cb_gmres")), timeout=300)


_plain_oracle = T._oracle


def _restated_oracle(case, G_):
    spec, A, o = _plain_oracle(case, G_)
    ksp = o.solver
    ksp.solve = lambda b: CB.gmres(ksp, b)
    return spec, A, o


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_dist_cb_gmres(ranks, case):
    from oracle import synthetic as S
    G_, res = ranks
    parts = res[case["name"]]
    spec, A, o = _restated_oracle(case, G_)
    b = S.rhs(spec)
    xo = o.solve(b)
    k = o.solver
    its, reason, ho = o.its, o.reason, np.asarray(o.history)
    assert (k.cb_forced, k.cb_confirm, k.cb_failed) == case["counters"]
    assert ho.size == its + 1 + k.cb_forced + k.cb_confirm
    r = np.asarray(k.cb_ratios)
    assert not np.any((r >= CB.BAND[0]) & (r <= CB.BAND[1])), "bad input: a borderline rule (a) decision"
    tol = max(1e-10, 10 * K._noise_floor(o, b, ho, its))
    for p in parts:
        assert np.array_equal(p["b_dev"], p["b"])
        assert int(p["its"]) == its, (int(p["its"]), its)
        assert int(p["reason"]) == reason
        h = p["hist"]
        assert h.shape == ho.shape
        rel = float(np.max(np.abs(h - ho) / ho))
        print(f"{case['name']}: its {its} entries {ho.size} history rel diff {rel:.3e} (tol {tol:.2e})")
        assert rel <= tol
    x = T.assemble(parts)
    assert np.linalg.norm(x - xo) <= max(1e-8, tol) * np.linalg.norm(xo)
