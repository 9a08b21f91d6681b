"""The Fischer guess (``global_ksp_guess_type fischer``) in the outer gmres on two
ranks (sharing the box's one GPU through the host-staged communicator) against
``OracleSolver(dist_size=2)`` with the numpy restatement
(tests/ksp_guess_restatement.py) installed as its ``solver.solve``: the stored
columns are each rank's rows and every projection goes through the global sum,
so nothing but the rank-ordered sums differs from one rank.  One 6-step
sequence, 2-D N=12, right, rtol 1e-6, size 2 (two resets); built as
tests/test_dist_gpu_cb_gmres.py is, on the block options of the first case of
tests/test_dist_gpu.py.  The bar is the one of tests/test_gpu_ksp_guess.py, per
step and on every rank: iteration count, reason and history length exact, every
history entry within max(1e-10, 10 x the restatement's own deviation up to that step under
1e-15 perturbations of the inner PC outputs and the stored columns, 4 seeds),
the assembled solution within max(1e-8, 10 x its own deviation), and the counters equal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ksp_guess_restatement as R
import test_dist_gpu as T
import test_gpu_ksp_guess as GG
from distutil import free_port
from oracle import petsc
from oracle import synthetic as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS, SIZE = 6, 2
_BLOCKS = {k: v for k, v in T.CASES[0]["db"].items() if not k.startswith("global_")}
CASE = {"name": "fischer_2d", "dim": 2, "N": 12,
        "db": dict(_BLOCKS, global_ksp_type="gmres", global_ksp_pc_side="right", **GG.fischer(SIZE)),
        "params": dict(T.BASE, **{"solver rtol": 1e-6, "solver atol": 0})}


def _restatement(seed=None, bs=None):
    case = dict(CASE, db={k: v for k, v in CASE["db"].items() if "ksp_guess" not in k})
    spec, A, o = T._oracle(case, 2)
    make = lambda k: GG.Perturbed(k, size=SIZE)  # noqa: E731
    return GG._sequence(o, A, S.rhs(spec), STEPS, make, petsc._gmres, bs=bs, seed=seed)


@pytest.fixture(scope="module")
def reference():
    base, g = _restatement()
    bs = [s["b"] for s in base]
    floor, xfloor = np.zeros(STEPS), np.zeros(STEPS)
    for seed in range(4):
        other, g2 = _restatement(seed, bs)
        assert g2.stats() == g.stats()
        for t, (a, c) in enumerate(zip(base, other)):
            assert a["its"] == c["its"], f"bad input: step {t} takes {c['its']} iterations with seed {seed}"
            floor[t] = max(floor[t], GG._rel(c["history"], a["history"]))
            xfloor[t] = max(xfloor[t], float(np.linalg.norm(c["x"] - a["x"]) / np.linalg.norm(a["x"])))
    for t, s in enumerate(base):
        assert R.margin(s["history"], s["ttol"]) >= R.BAND, f"bad input: step {t} is borderline"
    return base, g, np.maximum.accumulate(floor), np.maximum.accumulate(xfloor)


@pytest.fixture(scope="module")
def ranks(reference, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dist_ksp_guess"))
    rhs = os.path.join(tmp, "rhs.npy")
    np.save(rhs, np.array([s["b"] for s in reference[0]]))
    cf = os.path.join(tmp, "cases.json")
    with open(cf, "w") as f:
        json.dump([dict(CASE, rhs=rhs)], f)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}",
           os.path.join(HERE, "dist_seq_worker.py"), "--cases", cf, "--out", tmp]
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "2")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, f"ranks failed (rc={p.returncode}):\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    return [dict(np.load(os.path.join(tmp, f"{CASE['name']}_rank{r}.npz"))) for r in range(2)]


def test_dist_fischer_sequence(reference, ranks):
    base, g, floor, xfloor = reference
    assert g.resets >= 1
    n = sum(p["rows"].size for p in ranks)
    for t, s in enumerate(base):
        tol, xtol = max(1e-10, 10 * floor[t]), max(1e-8, 10 * xfloor[t])
        ho = np.asarray(s["history"])
        x = np.zeros(n)
        for p in ranks:
            assert int(p[f"its{t}"]) == s["its"], (t, int(p[f"its{t}"]), s["its"])
            assert int(p[f"reason{t}"]) == s["reason"]
            h = p[f"hist{t}"]
            assert h.shape == ho.shape
            rel = GG._rel(h, ho)
            assert rel <= tol, f"step {t}: history rel diff {rel:.3e} (tol {tol:.1e})"
            x[p["rows"]] = p[f"x{t}"]
        xerr = np.linalg.norm(x - s["x"]) / np.linalg.norm(s["x"])
        print(f"step {t}: its {s['its']} entries {ho.size} x {xerr:.2e} (tol {xtol:.1e})")
        assert xerr <= xtol
    for p in ranks:
        assert tuple(int(v) for v in p["stats"]) == g.stats()
        assert abs(float(p["reduction"]) - base[-1]["reduction"]) <= max(1e-10, 10 * floor[-1]) * base[-1]["reduction"]
