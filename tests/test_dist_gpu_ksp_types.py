"""fgmres and bcgs as the outer KSP on two ranks (sharing the box's one GPU
through the host-staged communicator) against ``OracleSolver(dist_size=2)``
with the numpy restatement (tests/ksp_restatements.py) installed as its
``solver.solve``.  Block options: the first case of tests/test_dist_gpu.py;
the comparison is that file's ``_check_dist_solve`` (rhs bitwise, SpMV and PC
application <= 1e-13, iteration count and reason exact, history within
1e-10 h_k + 100 eps h_0, solution within 1e-8)."""
import pytest

import test_dist_gpu as T
from distutil import launch
from ksp_restatements import bcgs, fgmres

pytestmark = pytest.mark.gpu

_BLOCKS = {k: v for k, v in T.CASES[0]["db"].items() if not k.startswith("global_")}
CASES = [
    {"name": "fgmres_2d", "dim": 2, "N": 12, "params": T.BASE, "restated": "fgmres",
     "db": dict(_BLOCKS, global_ksp_type="fgmres", global_ksp_gmres_restart="300")},
    {"name": "bcgs_right_2d", "dim": 2, "N": 12, "params": T.BASE, "restated": "bcgs",
     "db": dict(_BLOCKS, global_ksp_type="bcgs", global_ksp_pc_side="right")},
]


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    return 2, launch("gpu", CASES, 2, str(tmp_path_factory.mktemp("dist_ksp_types")), timeout=300)


def _restated_oracle(case, G):
    spec, A, o = _plain_oracle(case, G)
    ksp = o.solver
    if case["restated"] == "fgmres":
        ksp.solve = lambda b: fgmres(ksp, b)
    else:
        ksp.solve = lambda b: bcgs(ksp, b, True)
    return spec, A, o


_plain_oracle = T._oracle


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_dist_ksp_type(ranks, case, monkeypatch):
    monkeypatch.setattr(T, "_oracle", _restated_oracle)
    T._check_dist_solve(ranks, case)
