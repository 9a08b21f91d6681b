"""The recorded sweep-choice vectors against the CPU oracle.

tests/golden/ilu_sweep_choice/<case>.npy are device recordings (tests/test_gpu_sweep_choice.py
compares the device with them bitwise), so far never compared with anything but the device.  Here
every vector is held against the oracle's block PC applied to the same seeded vector, within 1e-12
max |y| -- the window kinds' bar, since some cases run explicit window inverses.  The footing cases'
oracle is the BoomerAMG restatement (about a second each at N = 16); pls.amg_gs_dense only chooses
between two forms of the same smoother.  footing-inexact-sgs-ranks3 is left out: the restatement of
hypre's three processes with twelve relaxation chunks takes minutes on the CPU (measured 215 s).
"""
import os

import numpy as np
import pytest

import sweep_choice_cases as G
from oracle.solver import OracleSolver

LEFT_OUT = ("footing-inexact-sgs-ranks3",)
CASES = [c for c in G.CASES if c not in LEFT_OUT]
_grid_oracle = []


def _petsc_db(db):
    return {k: v for k, v in db.items() if not k.startswith("pls.")}


def _oracle(name):
    """The oracle solver of the case's system, with the options the device test gives the device, and its size."""
    from oracle import synthetic as S

    def synthetic(spec, params, db):
        is_s, is_f, is_p = S.field_major_index_sets(spec)
        return OracleSolver(S.matrix(spec, 0), S.matrix(spec, 1), None, is_s, is_f, is_p, params, _petsc_db(db),
                            S.bcs_sub_pressure(spec)), spec.n

    if name.startswith("synth-bjacobi-"):
        nb = name.rsplit("-", 1)[1]
        db = G.preonly(("s_", "fp_"), "bjacobi", {"s_pc_bjacobi_blocks": nb, "fp_pc_bjacobi_blocks": nb})
        return synthetic(S.SynthSpec(3, 8), G.PARAMS, db)
    if name == "synth-ilu":
        return synthetic(S.SynthSpec(3, 8), G.PARAMS, G.preonly(("s_", "fp_"), "ilu"))
    if name == "lu-envelope":
        return synthetic(S.SynthSpec(2, 12), dict(G.PARAMS, **{"inner pc type": "lu"}), G.preonly(("s_", "fp_"), "lu"))
    if name in ("swelling-2way", "swelling-3way"):
        from lib.fe_swelling import assemble_swelling
        two = name == "swelling-2way"
        pc = "diagonal" if two else "diagonal 3-way"
        db = G.preonly(("s_", "fp_") if two else ("s_", "f_", "p_", "diff_"), "ilu")
        s = assemble_swelling(3, 4, pc)
        return OracleSolver(s.A, s.P, s.P_diff, s.is_s, s.is_f, s.is_p, dict(G.PARAMS, **{"pc type": pc}),
                            _petsc_db(db), s.bcs_sub_pressure), s.A.shape[0]
    if name in G.FOOTING:
        from lib.fe_footing import assemble_footing
        params, db = G.footing_options()
        db = dict(db, **{k: v for k, v in G.FOOTING[name].items() if k.startswith("pls.hypre")})
        s = assemble_footing(16, "undrained")
        return OracleSolver(s.A, s.P, s.P_diff, s.is_s, s.is_f, s.is_p, params,
                            {k: v for k, v in db.items() if not k.startswith("pls.") or k.startswith("pls.hypre")},
                            s.bcs_sub_pressure), s.A.shape[0]
    # the forced kinds: one system, one PC (the pls.* options only choose the kernel)
    if not _grid_oracle:
        A, is_s, is_f, is_p = G.grid_system()
        db = G.preonly(("s_",), "ilu", {"fp_ksp_type": "preonly", "fp_pc_type": "bjacobi", "fp_pc_bjacobi_blocks": "3"})
        _grid_oracle.append((OracleSolver(A, A, None, is_s, is_f, is_p, G.PARAMS, _petsc_db(db), []), A.shape[0]))
    return _grid_oracle[0]


def test_one_case_is_left_out():
    assert len(CASES) == len(G.CASES) - 1 and set(G.FORCED) <= set(CASES)


@pytest.mark.parametrize("name", CASES)
def test_recorded_vector_matches_the_oracle(name):
    o, n = _oracle(name)
    y = np.load(os.path.join(G.FIXTURE, name + ".npy"), allow_pickle=False)
    assert y.shape == (n,)
    yo = o.block_pc.apply(np.random.default_rng(8).standard_normal(n))
    scale = float(np.max(np.abs(yo)))
    ratio = float(np.max(np.abs(y - yo))) / scale
    print(f"{name}: max |y_recorded - y_oracle| / max |y_oracle| = {ratio:.2e}")
    assert ratio <= 1e-12
