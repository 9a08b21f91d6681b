"""The block PC's stateful and two-stream paths, AAR and the inner mixer, pinned bitwise.

tests/golden/blockpc_recorded/<case>.npz holds what libpls.so computed on the
MI355X before the block preconditioner, the Anderson machinery and the
sharding moved out of csrc/capi.cpp (recorder and case definitions:
tests/golden/make_golden_blockpc_recorded.py; two recordings in separate
processes agreed bitwise on every case).  On the synthetic 2-D system at
N = 8 (1,237 rows), ILU(0) inner PCs, input
``np.random.default_rng(8).standard_normal(n)``:

  * threeway-concurrent / threeway-serial: one 3-way pc_apply and a GMRES
    solve with the DIFF sweep on the second stream (pls.concurrent_sweeps 1)
    and on the main one (0); threeway-cg: CG inner solves (the serial branch);
  * twoway-mixer2 / threeway-mixer2: four successive pc_apply calls of one
    input with the inner Anderson mixer at order 2 (its history persists);
  * aar-m5p3 / aar-3way-mixer1: AAR (order 5, p 3), 2-way, and 3-way with the
    inner mixer at order 1;
  * twoway-fieldsplit: the fp fieldsplit with linear inner solves, and the
    pls_get_ksp_stats of both of its splits (the KSP enumeration);
  * twoway-update: a solve, pls_update_matrices with 1.25 P, a second solve.

Every array must be equal bitwise, every integer equal.
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_blockpc_recorded as G  # noqa: E402

CASES = G.CASES


def test_case_list_is_the_recorded_one():
    with open(os.path.join(G.FIXTURE, "cases.json")) as f:
        assert json.load(f) == CASES
    for name in CASES:
        assert os.path.exists(os.path.join(G.FIXTURE, name + ".npz"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_blockpc_as_recorded(gpu, name):
    want = G.load(name)
    got = G.run_case(name)
    assert sorted(got) == sorted(want)
    for key, w in want.items():
        g = np.asarray(got[key])
        assert g.dtype == w.dtype and g.shape == w.shape, key
        assert np.array_equal(g, w), key
