"""tests/bc_columns_restatement.py pinned on the CPU: on the blocks
lib/fe_footing.py and lib/fe_swelling.py assemble, the counts of the split, K' + C == K, the
lifted solve against the solve of the block as assembled (scipy splu), `drop` as a different
solve, and the oracle's CG + BoomerAMG on K' with a lifted right-hand side.
tests/test_gpu_bc_columns.py holds the device against this restatement.

Measured with splu and b = default_rng(1).standard_normal(n):

    block              rows  identity rows  moved  rows of C  |lift - keep|/|keep|  |drop - keep|/|keep|
    footing N=10, s    3690       42         408       84          1.9e-11               0.56
    footing N=10, f    3690       74         674      160          3.5e-16               0.19
    swelling N=8, s     578       34         448      152          2.0e-12               0.67
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import bc_columns_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "tools"),):
    if p not in sys.path:
        sys.path.insert(0, p)

# block -> (rows, identity rows, entries moved to C, rows of C, |lift - keep| / |keep| as measured)
TABLE = {
    "footing10_s": (3690, 42, 408, 84, 1.9e-11),
    "footing10_f": (3690, 74, 674, 160, 3.5e-16),
    "swelling8_s": (578, 34, 448, 152, 2.0e-12),
}


def _system(name):
    if name.startswith("footing"):
        from lib.fe_footing import assemble_footing
        return assemble_footing(10, "undrained")
    from lib.fe_swelling import assemble_swelling
    return assemble_swelling(2, 8, "diagonal")


@pytest.fixture(scope="module")
def blocks():
    out = {}
    for name in TABLE:
        s = _system(name)
        K = R.block_of(s.P, s.is_f if name.endswith("_f") else s.is_s)
        out[name] = (K,) + R.split(K)
    return out


@pytest.mark.parametrize("name", list(TABLE))
def test_counts(blocks, name):
    K, bc, Kp, c_rp, c_ci, c_val = blocks[name]
    n, nbc, moved, nrc, _ = TABLE[name]
    assert K.shape == (n, n)
    assert (bc.size, c_ci.size, int(np.count_nonzero(np.diff(c_rp)))) == (nbc, moved, nrc)
    assert np.all(np.diff(bc) > 0)
    assert np.all(c_val != 0.0)
    # the rule is tools/s_cg_attribution.py's
    import s_cg_attribution as T
    assert np.array_equal(bc, T.identity_rows(K))
    # a constrained row's own row of C is empty, and C's columns are the constrained rows
    assert np.all(np.diff(c_rp)[bc] == 0)
    assert np.all(np.isin(c_ci, bc))
    for i in np.flatnonzero(np.diff(c_rp)):
        assert np.all(np.diff(c_ci[c_rp[i]:c_rp[i + 1]]) > 0)


@pytest.mark.parametrize("name", list(TABLE))
def test_split_adds_up(blocks, name):
    K, bc, Kp, c_rp, c_ci, c_val = blocks[name]
    n = K.shape[0]
    assert np.array_equal(Kp.indptr, K.indptr) and np.array_equal(Kp.indices, K.indices)  # the pattern is kept
    C = R.c_matrix(n, c_rp, c_ci, c_val)
    assert np.array_equal((Kp + C).toarray(), K.toarray())
    # K' is what tools/s_cg_attribution.py calls the symmetric block, and symmetric to rounding
    import s_cg_attribution as T
    assert np.array_equal(T.symmetrized(K, bc).toarray(), Kp.toarray())
    assert abs(Kp - Kp.T).sum() <= 1e-15 * abs(Kp).sum()
    assert abs(K - K.T).sum() > 1e-3 * abs(K).sum()


@pytest.mark.parametrize("name", list(TABLE))
def test_lift_solves_the_block_as_assembled(blocks, name):
    K, bc, Kp, c_rp, c_ci, c_val = blocks[name]
    n = K.shape[0]
    b = np.random.default_rng(1).standard_normal(n)
    keep = spla.splu(sp.csc_matrix(K)).solve(b)
    lu = spla.splu(sp.csc_matrix(Kp))
    bl = R.lift(b, c_rp, c_ci, c_val)
    assert np.array_equal(bl[bc], b[bc])
    assert np.allclose(bl, b - R.c_matrix(n, c_rp, c_ci, c_val) @ b, rtol=0, atol=1e-12 * np.abs(b).max())
    lifted, dropped = lu.solve(bl), lu.solve(b)
    nk = np.linalg.norm(keep)
    err = np.linalg.norm(lifted - keep) / nk
    print(f"{name}: |lift - keep|/|keep| = {err:.2e}, |drop - keep|/|keep| = {np.linalg.norm(dropped - keep) / nk:.2e}")
    assert err <= max(10 * TABLE[name][4], 1e-12)
    assert np.linalg.norm(dropped - keep) / nk > 1e-3  # (the lift check's teeth)


@pytest.mark.parametrize("nranks", [8, 1])
@pytest.mark.parametrize("name", ["footing10_s", "swelling8_s"])
def test_oracle_cg_boomeramg_converges_on_the_lifted_system(blocks, name, nranks):
    """The inexact set's s solve (CG, rtol 1e-1, BoomerAMG) on K' with a lifted random right-hand
    side; on the block as assembled the same solve ends with a negative reason
    (tests/test_s_cg_attribution.py)."""
    import s_cg_attribution as T
    from robustness import load_set
    K, bc, Kp, c_rp, c_ci, c_val = blocks[name]
    db = dict(load_set("inexact"), **({"pls.hypre_ranks": "8", "pls.hypre_relax_chunks": "8"} if nranks > 1
                                      else {"pls.hypre_relax_chunks": "1"}))
    b = R.lift(np.random.default_rng(1).standard_normal(K.shape[0]), c_rp, c_ci, c_val)
    res = T.run(Kp, b, db, 200)
    assert res["reason"] > 0 and res["its"] <= 15, res


def test_rule_on_a_hand_matrix():
    """Row 1: identity row with a stored zero.  Row 3: diagonal 1 but a nonzero neighbour -- not
    constrained.  Row 4: no stored diagonal.  Column 1 holds 2.0 (row 0), a stored 0.0 (row 2) and
    -3.0 (row 3): two entries move, the stored zero stays in the pattern and in K' only."""
    rows = [[0, 1], [0, 1], [1, 2], [1, 3, 4], [3]]
    vals = [[4.0, 2.0], [0.0, 1.0], [0.0, 5.0], [-3.0, 1.0, 0.5], [1.0]]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    K = sp.csr_matrix((np.concatenate(vals), np.concatenate(rows), rp), shape=(5, 5))
    bc, Kp, c_rp, c_ci, c_val = R.split(K)
    assert bc.tolist() == [1]
    assert c_rp.tolist() == [0, 1, 1, 1, 2, 2] and c_ci.tolist() == [1, 1] and c_val.tolist() == [2.0, -3.0]
    assert Kp.nnz == K.nnz and Kp.data.tolist() == [4.0, 0.0, 0.0, 1.0, 0.0, 5.0, 0.0, 1.0, 0.5, 1.0]
    b = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    assert R.lift(b, c_rp, c_ci, c_val).tolist() == [1.0 - 4.0, 2.0, 3.0, 4.0 + 6.0, 5.0]
