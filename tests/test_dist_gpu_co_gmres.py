"""Compressed-operator GMRES (``global_pls_gmres_operator single`` on the fp32
basis) in the outer gmres on two ranks (sharing the box's one GPU through the
host-staged communicator) against ``OracleSolver(dist_size=2)`` with the numpy
restatement (tests/co_gmres_restatement.py) installed as its ``solver.solve``.
The low product of a sharded operator is the D16 kernel's halo instantiation
over the rank's fp32 value stream: once as the overlapped interior / halo pair
of launches (``pls.halo_overlap 1``, the default) and once as the plain launch
after the exchange.  More than one rank has no coupling reuse, so the low
operator is fl32(A); the rounding is local to a rank and changes no value, so
nothing but the rank-ordered sums of oracle/dist.py differs from one rank.

2-D N=12, right, rtol 1e-6; the block options of the first case of
tests/test_dist_gpu.py.  The bar is the one of tests/test_gpu_co_gmres.py:
iteration count, reason and history length exact on every rank, every history
entry within max(1e-10, 10 x the restatement's own deviation under 1e-15
perturbations of the inner PC outputs, 4 seeds), the assembled solution within
max(1e-8, that bound); the operator stats equal the restatement's counters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cb_gmres_restatement as CB
import co_gmres_restatement as CO
import test_dist_gpu as T
import test_gpu_ksp_types as K
from distutil import free_port

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_BLOCKS = {k: v for k, v in T.CASES[0]["db"].items() if not k.startswith("global_")}
_OUTER = dict(_BLOCKS, global_ksp_type="gmres", global_ksp_pc_side="right", global_pls_gmres_basis="single",
              global_pls_gmres_operator="single")
_PARAMS = dict(T.BASE, **{"solver rtol": 1e-6, "solver atol": 0})
CASES = [
    {"name": "co_gmres_overlap", "dim": 2, "N": 12, "db": dict(_OUTER, **{"pls.halo_overlap": "1"}), "params": _PARAMS},
    {"name": "co_gmres_plain", "dim": 2, "N": 12, "db": dict(_OUTER, **{"pls.halo_overlap": "0"}), "params": _PARAMS},
]


def _launch(cases, world, tmp, timeout=300):
    """distutil.launch with the worker that returns the operator stats."""
    cf = os.path.join(tmp, "cases.json")
    with open(cf, "w") as f:
        json.dump(cases, f)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}",
           os.path.join(HERE, "dist_worker_co.py"), "--cases", cf, "--out", tmp]
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "2")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    assert p.returncode == 0, f"ranks failed (rc={p.returncode}):\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    return {c["name"]: [dict(np.load(os.path.join(tmp, f"{c['name']}_rank{r}.npz"))) for r in range(world)]
            for c in cases}


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    return 2, _launch(CASES, 2, str(tmp_path_factory.mktemp("dist_co_gmres")))


@pytest.fixture(scope="module")
def reference():
    """The restated two-rank solve (the same for both cases: the overlap changes no sum)."""
    from oracle import synthetic as S
    case = dict(CASES[0], db={k: v for k, v in _OUTER.items() if "pls_gmres" not in k})
    spec, A, o = T._oracle(case, 2)
    ksp = o.solver
    A_low = CO.low_matrix(ksp.A)
    ksp.solve = lambda b: CO.gmres(ksp, b, lambda v: A_low @ v)
    b = S.rhs(spec)
    xo = o.solve(b)
    its, reason, ho = o.its, o.reason, np.asarray(o.history)
    counters = (ksp.cb_forced, ksp.cb_confirm, ksp.cb_failed, ksp.co_low, ksp.co_double)
    assert counters == (0, 1, 0, its, 1)
    r = np.asarray(ksp.cb_ratios)
    assert not np.any((r >= CB.BAND[0]) & (r <= CB.BAND[1])), "bad input: a borderline rule (a) decision"
    CO.check_confirmations("dist 2d12_right", ksp.co_confirm)
    tol = max(1e-10, 10 * K._noise_floor(o, b, ho, its))
    return {"A": A, "A_low": A_low, "xo": xo, "its": its, "reason": reason, "ho": ho, "tol": tol, "counters": counters}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_dist_co_gmres(ranks, reference, case):
    G_, res = ranks
    parts = res[case["name"]]
    ref = reference
    its, ho, tol = ref["its"], ref["ho"], ref["tol"]
    for p in parts:
        assert int(p["its"]) == its, (int(p["its"]), its)
        assert int(p["reason"]) == ref["reason"]
        h = p["hist"]
        assert h.shape == ho.shape
        rel = float(np.max(np.abs(h - ho) / ho))
        print(f"{case['name']}: its {its} entries {ho.size} history rel diff {rel:.3e} (tol {tol:.2e}); "
              f"operator stats {p['op_stats']} layout {p['layout']} single {p['layout_single']}")
        assert rel <= tol
        assert p["layout"][0] == 1 and p["layout_single"][0] == 1
        low_bytes = int(p["layout"][1] - p["layout_single"][1])  # 4 B per stored entry of the rank's layout
        assert low_bytes > 0
        assert tuple(p["op_stats"]) == (1, low_bytes, ref["counters"][3], ref["counters"][4])
        assert tuple(p["basis_stats"][[0, 2, 3, 4]]) == (1,) + ref["counters"][:3]
        # the rank's low product is its rows of fl32(A) v, and not its rows of A v
        rows, v = p["rows"], p["v"]
        want = (ref["A_low"] @ v)[rows]
        scale = (abs(ref["A_low"]) @ np.abs(v))[rows]
        assert np.all(np.abs(p["Av_low"] - want) <= 1e-13 * scale)
        assert np.any(p["Av_low"] != p["Av"])
    x = T.assemble(parts)
    assert np.linalg.norm(x - ref["xo"]) <= max(1e-8, tol) * np.linalg.norm(ref["xo"])
