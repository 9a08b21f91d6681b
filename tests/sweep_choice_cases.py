"""The case table of the sweep-choice recordings (tests/golden/ilu_sweep_choice/), shared by the device
test that compares the device with them (tests/test_gpu_sweep_choice.py, which describes the cases)
and the CPU test that compares them with the oracle (tests/test_sweep_choice_recorded.py)."""
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ilu_sweep_choice")

PARAMS = {"solver type": "gmres", "solver atol": 1e-8, "solver rtol": 1e-6, "solver maxiter": 100,
          "pc type": "diagonal", "inner ksp type": "preonly", "inner pc type": "ilu", "inner accel order": 0,
          "AAR order": 10, "AAR p": 5, "AAR omega": 1, "AAR beta": 1}
GLOBAL = {"global_ksp_type": "gmres", "global_ksp_pc_side": "right", "pls.ilu_view": "1"}

# (b): options that force a kind on the grid system
FORCED = {
    "grid-default": {},
    "grid-levels": {"pls.ilu_lds": "0"},
    "grid-levels-csr": {"pls.ilu_lds": "0", "pls.ilu_gmem": "-2"},
    "grid-gmem-2": {"pls.ilu_gmem": "-2"},
    "grid-gmem": {"pls.ilu_gmem": "1", "pls.ilu_ring": "0"},
    "grid-ring": {"pls.ilu_gmem": "1"},
    "grid-chain": {"pls.sweep_chain": "1"},
    "grid-window": {"pls.sweep_window": "1"},
    "grid-window-ring": {"pls.sweep_window": "1", "pls.window_ring": "1"},
    "grid-gmem-window-ring": {"pls.ilu_gmem": "1", "pls.sweep_window": "1"},
    "grid-mixed": {"pls.ilu_gmem": "1", "pls.sweep_window": "1", "pls.window_mixed": "1"},
    "grid-swin": {"pls.ilu_gmem": "1", "pls.sweep_swin": "1"},
}
CASES = (["synth-bjacobi-1", "synth-bjacobi-8", "synth-bjacobi-64", "synth-bjacobi-264", "synth-ilu",
          "swelling-2way", "swelling-3way", "footing-inexact", "footing-inexact-sgs", "footing-inexact-sgs-ranks3",
          "lu-envelope"] + list(FORCED))
# the AMG's Gauss-Seidel chunks as PCILU blocks (not dense inverses); as under mpirun -np 3: explicit chunk bounds
FOOTING = {"footing-inexact": {}, "footing-inexact-sgs": {"pls.amg_gs_dense": "0"},
           "footing-inexact-sgs-ranks3": {"pls.amg_gs_dense": "0", "pls.hypre_ranks": "3",
                                          "pls.hypre_relax_chunks": "12", "pls.hypre_relax_min_rows": "0"}}
KINDS = ("levels", "levels-csr", "lds", "gmem", "ring", "chain", "window", "window-ring", "levels+window-ring", "swin")


def preonly(prefixes, pc_type, extra=None):
    db = dict(GLOBAL)
    for pre in prefixes:
        db[pre + "ksp_type"] = "preonly"
        db[pre + "pc_type"] = pc_type
    db.update(extra or {})
    return db


def _grid_block(nx, ny, rng):
    n = nx * ny
    i = np.arange(n)
    rows, cols = [i], [i]
    for d, ok in ((1, (i % nx) < nx - 1), (-1, (i % nx) > 0), (nx, i < n - nx), (-nx, i >= nx)):
        rows.append(i[ok])
        cols.append(i[ok] + d)
    r, c = np.concatenate(rows), np.concatenate(cols)
    v = -rng.uniform(0.2, 1.0, r.size)
    v[:n] = 0.0
    M = sp.csr_matrix((v, (r, c)), shape=(n, n))
    M = M + sp.diags(np.asarray(abs(M).sum(axis=1)).ravel() + rng.uniform(0.05, 0.5, n))
    return M.tocsr()


def grid_system():
    rng = np.random.default_rng(17)
    blocks = [_grid_block(40, 40, rng), _grid_block(40, 38, rng), _grid_block(24, 24, rng)]
    A = sp.block_diag(blocks, format="csr")
    A.sort_indices()
    off = np.cumsum([0] + [b.shape[0] for b in blocks])
    return (A,) + tuple(np.arange(off[k], off[k + 1], dtype=np.int32) for k in range(3))


def footing_options():
    """(params, db) of options/inexact as tests/golden/make_golden_footing.py reads them."""
    golden = os.path.join(HERE, "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    import make_golden_footing as G
    return G.options("inexact")
