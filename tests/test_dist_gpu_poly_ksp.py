"""The s block solved by Chebyshev/Jacobi without norms (s_ksp_norm_type none,
four iterations) on two ranks (sharing the box's one GPU through the
host-staged communicator) against ``OracleSolver(dist_size=2)`` with the numpy
restatement (tests/poly_restatements.py) installed as the s block's solve: once
with explicit eigenvalue bounds, once with estimated ones -- the estimate's
right-hand side is a function of the block-global row index, so the sharded
estimate is the whole block's.  Other block options: the first case of
tests/test_dist_gpu.py; the comparison is that file's ``_check_dist_solve``
(rhs bitwise, SpMV and PC application <= 1e-13, iteration count and reason
exact, history within 1e-10 h_k + 100 eps h_0, solution within 1e-8)."""
import pytest

import test_dist_gpu as T
from distutil import launch
from poly_restatements import chebyshev, esteig

pytestmark = pytest.mark.gpu

_CHEB = {"s_ksp_type": "chebyshev", "s_pc_type": "jacobi", "s_ksp_norm_type": "none", "s_ksp_max_it": "4"}
_BASE_DB = {k: v for k, v in T.CASES[0]["db"].items() if not k.startswith("s_")}
CASES = [
    {"name": "cheb_explicit_2d", "dim": 2, "N": 12, "params": T.BASE, "bounds": (0.15, 1.6),
     "db": dict(_BASE_DB, **_CHEB, s_ksp_chebyshev_eigenvalues="0.15,1.6")},
    {"name": "cheb_estimated_2d", "dim": 2, "N": 12, "params": T.BASE, "bounds": None, "db": dict(_BASE_DB, **_CHEB)},
]


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    return 2, launch("gpu", CASES, 2, str(tmp_path_factory.mktemp("dist_poly_ksp")), timeout=300)


_plain_oracle = T._oracle


def _restated_oracle(case, G):
    spec, A, o = _plain_oracle(case, G)
    ksp = o.block_pc.ksp_s
    assert ksp.type == "chebyshev" and ksp.norm_type == "none"
    state = {}

    def solve(b):
        if "bounds" not in state:  # (the block is held whole here: its rows are the global ones)
            state["bounds"] = case["bounds"] or esteig(ksp, 10)[:2]
        return chebyshev(ksp, b, *state["bounds"])

    ksp.solve = solve
    return spec, A, o


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_dist_chebyshev_inner(ranks, case, monkeypatch):
    monkeypatch.setattr(T, "_oracle", _restated_oracle)
    T._check_dist_solve(ranks, case)
