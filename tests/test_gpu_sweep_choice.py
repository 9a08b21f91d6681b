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

import numpy as np
import pytest

from sweep_choice_cases import CASES, FIXTURE, FOOTING, FORCED, KINDS, PARAMS, footing_options, grid_system, preonly


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
        db = preonly(("s_", "fp_"), "bjacobi", {"s_pc_bjacobi_blocks": nb, "fp_pc_bjacobi_blocks": nb})
        return synthetic(S.SynthSpec(3, 8), PARAMS, db)
    if name == "synth-ilu":
        return synthetic(S.SynthSpec(3, 8), PARAMS, preonly(("s_", "fp_"), "ilu"))
    if name == "lu-envelope":
        params = dict(PARAMS, **{"inner pc type": "lu"})
        return synthetic(S.SynthSpec(2, 12), params, preonly(("s_", "fp_"), "lu", {"pls.lu_path": "envelope"}))
    if name in ("swelling-2way", "swelling-3way"):
        from lib.fe_swelling import assemble_swelling
        two = name == "swelling-2way"
        pc = "diagonal" if two else "diagonal 3-way"
        db = preonly(("s_", "fp_") if two else ("s_", "f_", "p_", "diff_"), "ilu")
        return assembled(assemble_swelling(3, 4, pc), dict(PARAMS, **{"pc type": pc}), db)
    if name in FOOTING:
        from lib.fe_footing import assemble_footing
        params, db = footing_options()
        return assembled(assemble_footing(16, "undrained"), params, dict(db, **{"pls.ilu_view": "1"}, **FOOTING[name]))
    A, is_s, is_f, is_p = grid_system()
    db = preonly(("s_",), "ilu", {"fp_ksp_type": "preonly", "fp_pc_type": "bjacobi", "fp_pc_bjacobi_blocks": "3"})
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
