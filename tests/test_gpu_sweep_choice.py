"""Which sweep kernel every ILU(0) / Gauss-Seidel PC picks, pinned.

PCILU (csrc/ilu.cpp) serves ``ilu``, ``bjacobi``, the envelope ``lu`` and the
classical AMG's hybrid Gauss-Seidel chunks with one of ten apply kernels
(levels, levels-csr, lds, gmem, ring, chain, window, window-ring,
levels+window-ring, swin).  A change of the choice is silent: the PC stays
correct, only no longer the kernel that was measured.  For a fixed case list
tests/golden/ilu_sweep_choice/ holds every ``[pls ilu]`` line that
pls.ilu_view printed (lines.json: type, n, blocks, max_len, levels L/U,
sweep, records) and the block PC applied to one seeded vector (<case>.npy:
the vectors do not compress, so one file per case), as recorded on the MI355X
before PCILU moved into its own file.  The lines must match character for
character and the vector bitwise (two recordings in separate processes agreed
bitwise on every case).

Cases: (a) every tuning option at its default -- synthetic 3-D N = 8 with
BJACOBI at 1, 8, 64 and 264 blocks and with whole-block ILU(0), the assembled
3-D swelling system at N = 4 (2-way, 3-way), the 2-D footing system at N = 16
under options/inexact, and the envelope LU on blocks of a few hundred rows.
At N = 16 the AMG's cost model sends every Gauss-Seidel chunk through its
dense inverse (no PCILU, no line), so the footing case runs twice more with
pls.amg_gs_dense 0 -- the chunks as sgs factors with every ILU option at its
default -- once under pls.hypre_ranks 3 for explicit chunk bounds; (b) each
kind the small default cases do not reach, forced with the options the sweep
tests use, on 5-point grid blocks of ~40 x 40 rows (25 windows, 79 levels;
the fp block as 3 BJACOBI blocks).
"""
import json
import os
import sys

import numpy as np
import pytest
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


def _preonly(prefixes, pc_type, extra=None):
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


def _grid_system():
    rng = np.random.default_rng(17)
    blocks = [_grid_block(40, 40, rng), _grid_block(40, 38, rng), _grid_block(24, 24, rng)]
    A = sp.block_diag(blocks, format="csr")
    A.sort_indices()
    off = np.cumsum([0] + [b.shape[0] for b in blocks])
    return (A,) + tuple(np.arange(off[k], off[k + 1], dtype=np.int32) for k in range(3))


def _handle(name):
    """The case's handle (not yet set up) and the size of its system."""
    from lib.handle import Handle, params_to_options
    from oracle import synthetic as S

    def synthetic(spec, params, db):
        opts = dict(db)
        opts.update(params_to_options(params))
        return Handle.synthetic(spec.dim, spec.N, spec.seed, spec.delta, opts), spec.n

    def assembled(s, params, db):
        opts = dict(db)
        opts.update(params_to_options(params))
        h = Handle.from_csr(s.A, s.P, s.P_diff, s.is_s, s.is_f, s.is_p, s.bcs_sub_pressure, opts)
        return h, s.A.shape[0]

    if name.startswith("synth-bjacobi-"):
        nb = name.rsplit("-", 1)[1]
        db = _preonly(("s_", "fp_"), "bjacobi", {"s_pc_bjacobi_blocks": nb, "fp_pc_bjacobi_blocks": nb})
        return synthetic(S.SynthSpec(3, 8), PARAMS, db)
    if name == "synth-ilu":
        return synthetic(S.SynthSpec(3, 8), PARAMS, _preonly(("s_", "fp_"), "ilu"))
    if name == "lu-envelope":
        params = dict(PARAMS, **{"inner pc type": "lu"})
        return synthetic(S.SynthSpec(2, 12), params, _preonly(("s_", "fp_"), "lu", {"pls.lu_path": "envelope"}))
    if name in ("swelling-2way", "swelling-3way"):
        from lib.fe_swelling import assemble_swelling
        two = name == "swelling-2way"
        pc = "diagonal" if two else "diagonal 3-way"
        db = _preonly(("s_", "fp_") if two else ("s_", "f_", "p_", "diff_"), "ilu")
        return assembled(assemble_swelling(3, 4, pc), dict(PARAMS, **{"pc type": pc}), db)
    if name in FOOTING:
        from lib.fe_footing import assemble_footing
        sys.path.insert(0, os.path.join(HERE, "golden"))
        import make_golden_footing as G
        params, db = G.options("inexact")
        return assembled(assemble_footing(16, "undrained"), params, dict(db, **{"pls.ilu_view": "1"}, **FOOTING[name]))
    A, is_s, is_f, is_p = _grid_system()
    db = _preonly(("s_",), "ilu", {"fp_ksp_type": "preonly", "fp_pc_type": "bjacobi", "fp_pc_bjacobi_blocks": "3"})
    opts = dict(db, **FORCED[name])
    opts.update(params_to_options(PARAMS))
    return Handle.from_csr(A, A, None, is_s, is_f, is_p, [], opts), A.shape[0]


def run_case(name):
    """Build the case's PCs (their [pls ilu] lines go to stderr) and apply the block PC once."""
    h, n = _handle(name)
    y = h.pc_apply(np.random.default_rng(8).standard_normal(n))
    h.destroy()
    return y


def ilu_lines(err):
    return [ln for ln in err.splitlines() if ln.startswith("[pls ilu]")]


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(FIXTURE, "lines.json")) as f:
        return json.load(f)


def test_case_list_is_the_recorded_one(recorded):
    assert list(recorded) == CASES


def test_recorded_cases_reach_every_kind(recorded):
    seen = {ln.split(" sweep ")[1].split(" ")[0] for c in CASES for ln in recorded[c]}
    assert seen == set(KINDS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_sweep_choice_and_apply_as_recorded(gpu, capfd, recorded, name):
    capfd.readouterr()
    y = run_case(name)
    lines = ilu_lines(capfd.readouterr().err)
    assert lines == recorded[name]
    assert np.array_equal(y, np.load(os.path.join(FIXTURE, name + ".npy"), allow_pickle=False))
