"""Modified Gram-Schmidt and refine_ifneeded classical Gram-Schmidt in the outer
gmres on two ranks (sharing the box's one GPU through the host-staged
communicator) against ``OracleSolver(dist_size=2)`` with the numpy restatement
(tests/gmres_orthog_restatement.py) installed as its ``solver.solve``: with
more than one rank every modified Gram-Schmidt step's sum goes through k_final
and the global sum before the next step reads it.  Built as
tests/test_dist_gpu_ksp_types.py is: the block options of the first case of
tests/test_dist_gpu.py, that file's ``_check_dist_solve`` (rhs bitwise, SpMV
and PC application <= 1e-13, iteration count and reason exact, history within
1e-10 h_k + 100 eps h_0, solution within 1e-8)."""
import pytest

import gmres_orthog_restatement as G
import test_dist_gpu as T
from distutil import launch

pytestmark = pytest.mark.gpu

_BLOCKS = {k: v for k, v in T.CASES[0]["db"].items() if not k.startswith("global_")}
_OUTER = dict(_BLOCKS, global_ksp_type="gmres", global_ksp_pc_side="right")
CASES = [
    {"name": "gmres_mgs_2d", "dim": 2, "N": 12, "params": T.BASE, "restated": "mgs",
     "db": dict(_OUTER, global_ksp_gmres_modifiedgramschmidt=None)},
    {"name": "gmres_refine_ifneeded_2d", "dim": 2, "N": 12, "params": T.BASE, "restated": "refine_ifneeded",
     "db": dict(_OUTER, global_ksp_gmres_cgs_refinement_type="refine_ifneeded")},
]


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    return 2, launch("gpu", CASES, 2, str(tmp_path_factory.mktemp("dist_gmres_orthog")), timeout=300)


_plain_oracle = T._oracle


def _restated_oracle(case, G_):
    spec, A, o = _plain_oracle(case, G_)
    ksp = o.solver
    kw = G.SCHEMES[case["restated"]][1]
    ksp.solve = lambda b: G.gmres(ksp, b, **kw)
    return spec, A, o


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_dist_gmres_orthog(ranks, case, monkeypatch):
    monkeypatch.setattr(T, "_oracle", _restated_oracle)
    T._check_dist_solve(ranks, case)
    _, _, o = _restated_oracle(case, 2)
    from oracle import synthetic as S
    o.solve(S.rhs(S.SynthSpec(case["dim"], case["N"])))
    if case["restated"] == "refine_ifneeded":  # a good input: second passes happen, no decision near its threshold
        assert o.solver.nearest_decision >= 1e-6
        assert 0 < o.solver.second_passes <= o.its
