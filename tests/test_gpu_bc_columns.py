"""<prefix>pls_bc_columns keep | lift | drop on the device (csrc/bccols.hip,
csrc/bccols.cpp) against tests/bc_columns_restatement.py and the CPU oracle, on the blocks
lib/fe_footing.py and lib/fe_swelling.py assemble.

1. the split, bitwise: constrained rows and C (c_rp, c_ci, c_val) equal to the restatement's, the
   stats with them; a block without constrained rows (p_) is not touched by lift;
2. drop against the oracle handed P with the constrained columns zeroed inside each block: one
   block-PC application at the bound the existing parity tests use for the inner PC (ilu and
   hypre: 1e-12 of the largest entry, tests/test_gpu_fe.py and tests/test_gpu_amg.py; lu: the
   block residuals of tests/test_gpu_sparse_lu.py, 1e-9 on s and 1e-12 on fp), one solve through
   tests/test_gpu_fe.py's _compare;
3. lift is the same preconditioner as keep (PREONLY + LU): within 10 x what the same comparison
   gives with scipy's splu on the CPU (at least 1e-12), while drop is not (> 1e-3);
4. lift under the inexact set: the s part of a 2-way application is the oracle's CG + BoomerAMG
   on K' with the lifted x_s -- the same iteration count, a positive reason, the solution within
   1e-8 (the bound of tests/test_gpu_footing.py's inner-CG application);
5. footing N = 20, 2-way, options/inexact-lift, np = 8 semantics against
   tests/golden/bc_columns/footing_N20_inexact_lift.json: converged, no s_ solve with a negative
   reason, the longest s_ solve within twice the oracle's, the outer count in the oracle's
   perturbed range (tests/test_gpu_harness.py's window).  On the parent commit this case took
   271,570 s_ iterations with 27 solves at max_it;
6. the refusals, and pls_update_matrices: a P with one more constrained row is detected and
   split again; a second identical solve is bitwise the first.
   The refusal of differing operator and preconditioner matrices cannot be reached through any
   entry point today (every make_ksp call passes one matrix for both, or no operator) and the
   sharded one needs a worker process: both are checked by reading make_ksp.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

import bc_columns_restatement as B
from lib import fe_footing as FF
from lib import fe_swelling as F
from oracle.solver import OracleSolver
from test_gpu_fe import BASE, _db

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

BOOMER = {"pc_hypre_boomeramg_P_max": "4", "pc_hypre_boomeramg_agg_nl": "1", "pc_hypre_boomeramg_agg_num_paths": "2",
          "pc_hypre_boomeramg_coarsen_type": "HMIS", "pc_hypre_boomeramg_interp_type": "ext+i",
          "pc_hypre_boomeramg_no_CF": "true"}


@functools.lru_cache(maxsize=None)
def _system(problem, N, pc, ordering="field-major"):
    if problem == "footing":
        return FF.assemble_footing(N, pc, ordering=ordering)
    return F.assemble_swelling(2, N, pc, ordering=ordering)


def _handle(s, params, db, P=None):
    from lib.handle import Handle, params_to_options
    opts = dict(db)
    opts.update(params_to_options(dict(BASE, **params)))
    return Handle.from_csr(s.A, s.P if P is None else P, s.P_diff, s.is_s, s.is_f, s.is_p, s.bcs_sub_pressure, opts)


def _rows_of(s, prefix):
    """The rows (P's numbering) of the block a prefix solves, in the block's own order."""
    return {"s_": np.asarray(s.is_s), "f_": np.asarray(s.is_f), "p_": np.asarray(s.is_p),
            "fp_": np.sort(np.concatenate([s.is_f, s.is_p]))}[prefix]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _rel_fields(a, b, s):
    """The largest relative difference over the three fields (the fp part of a 2-way application is 1e6 times
    the s part on the swelling system: one norm over the whole vector would not see the s block)."""
    return max(_rel(a[i], b[i]) for i in (np.asarray(s.is_s), np.asarray(s.is_f), np.asarray(s.is_p)))


def _check_split(h, K, prefix, mode):
    bc, _, c_rp, c_ci, c_val = B.split(K)
    st = h.bc_columns_stats(prefix)
    rows, rp, ci, v = h.bc_columns_matrix(prefix)
    print(f"{prefix} stats {st}")
    assert st[:4] == (mode, bc.size, c_ci.size, int(np.count_nonzero(np.diff(c_rp))))
    # DESIGN.md section 25, "Memory": K', C with its lists, and under lift the row map and b'
    n, nrc = K.shape[0], int(np.count_nonzero(np.diff(c_rp)))
    want = 12 * K.nnz + 8 * (n + 1) + 12 * c_ci.size + 4 * (bc.size + nrc) + 8 * (nrc + 1)
    if mode == 1:
        want += 8 * ((n + 31) // 32) + 8 * n
    assert st[4] == (want if c_ci.size else 4 * bc.size), (st[4], want)
    assert np.array_equal(rows, bc)
    assert np.array_equal(rp, c_rp) and np.array_equal(ci, c_ci)
    assert np.array_equal(v, c_val)  # bitwise
    return st


# ------------------------------------------------------------- 1. the split --
@pytest.mark.parametrize("problem,N,pc,ordering,inner,prefixes", [
    ("footing", 10, "undrained 3-way", "field-major", "lu", ("s_", "f_")),
    ("swelling", 8, "diagonal", "interleaved", "ilu", ("s_",)),
    ("swelling", 8, "diagonal", "field-major", "ilu", ("s_",)),
])
def test_split_bitwise(gpu, problem, N, pc, ordering, inner, prefixes):
    s = _system(problem, N, pc, ordering)
    db = _db(inner, {p + "pls_bc_columns": "lift" for p in prefixes})
    h = _handle(s, {"pc type": pc}, db)
    for p in prefixes:
        st = _check_split(h, B.block_of(s.P, _rows_of(s, p)), p, 1)
        assert st[1] > 0 and st[2] > 0
    # the same lists under drop, and nothing under keep
    h2 = _handle(s, {"pc type": pc}, _db(inner, {prefixes[0] + "pls_bc_columns": "drop"}))
    _check_split(h2, B.block_of(s.P, _rows_of(s, prefixes[0])), prefixes[0], 2)
    for p in prefixes[1:]:
        assert h2.bc_columns_stats(p) == (0, 0, 0, 0, 0)
        rows, rp, ci, v = h2.bc_columns_matrix(p)
        assert rows.size == 0 and ci.size == 0 and not rp.any()
    # a second handle gives the same bits (no atomics decide an order)
    h3 = _handle(s, {"pc type": pc}, db)
    for a, b in zip(h.bc_columns_matrix(prefixes[0]), h3.bc_columns_matrix(prefixes[0])):
        assert np.array_equal(a, b)
    for x in (h, h2, h3):
        x.destroy()


def test_block_without_constrained_rows(gpu):
    """The p block holds no identity rows: lift reports 0 rows, copies nothing and solves bitwise as keep."""
    s = _system("footing", 10, "undrained 3-way")
    assert B.identity_rows(B.block_of(s.P, s.is_p)).size == 0
    hk = _handle(s, {"pc type": "undrained 3-way"}, _db("lu"))
    hl = _handle(s, {"pc type": "undrained 3-way"}, _db("lu", {"p_pls_bc_columns": "lift"}))
    assert hl.bc_columns_stats("p_") == (1, 0, 0, 0, 0)
    assert hk.bc_columns_stats("p_") == (0, 0, 0, 0, 0)
    x = np.random.default_rng(11).standard_normal(s.A.shape[0])
    assert np.array_equal(hl.pc_apply(x), hk.pc_apply(x))
    hk.destroy()
    hl.destroy()


def test_constrained_rows_whose_columns_are_zero(gpu):
    """P with the s block's constrained columns already zero: the rows are reported, nothing moves, the block is
    not copied (the bytes are the row list's) and lift solves bitwise as keep."""
    s = _system("swelling", 8, "diagonal")
    P0 = B.zero_bc_columns(s.P, [s.is_s])
    nbc = B.identity_rows(B.block_of(s.P, s.is_s)).size
    hk = _handle(s, {"pc type": "diagonal"}, _db("ilu"), P=P0)
    hl = _handle(s, {"pc type": "diagonal"}, _db("ilu", {"s_pls_bc_columns": "lift"}), P=P0)
    assert hl.bc_columns_stats("s_") == (1, nbc, 0, 0, 4 * nbc)
    _check_split(hl, B.block_of(P0, s.is_s), "s_", 1)
    x = np.random.default_rng(12).standard_normal(s.A.shape[0])
    assert np.array_equal(hl.pc_apply(x), hk.pc_apply(x))
    hk.destroy()
    hl.destroy()


# ------------------------------------------------- 2. drop against the oracle --
def _drop_case(pc, inner):
    three = "3-way" in pc
    prefixes = ("s_", "f_") if three else ("s_",)
    extra = {p + "pls_bc_columns": "drop" for p in prefixes}
    db = _db("lu" if inner == "lu" else "ilu", extra)
    if inner == "hypre":  # PREONLY + the classical AMG with the inexact set's BoomerAMG settings (a linear PC)
        for p in ("s_", "f_", "p_", "diff_"):
            db[p + "pc_type"] = "hypre"
            db.update({p + k: v for k, v in BOOMER.items()})
    return prefixes, db


@pytest.mark.parametrize("problem,N,pc,inner", [
    ("swelling", 8, "diagonal", "lu"),
    ("footing", 10, "undrained", "lu"),
    ("swelling", 8, "diagonal", "ilu"),
    ("swelling", 8, "diagonal 3-way", "ilu"),
    ("swelling", 8, "diagonal", "hypre"),
    ("swelling", 8, "diagonal 3-way", "hypre"),
])
def test_drop_pc_apply_matches_oracle(gpu, problem, N, pc, inner):
    s = _system(problem, N, pc)
    prefixes, db = _drop_case(pc, inner)
    params = dict(BASE, **{"pc type": pc})
    P0 = B.zero_bc_columns(s.P, [_rows_of(s, p) for p in prefixes])
    assert abs(P0 - s.P).sum() > 0
    o = OracleSolver(s.A, P0, s.P_diff, s.is_s, s.is_f, s.is_p, params, db, s.bcs_sub_pressure)
    okeep = OracleSolver(s.A, s.P, s.P_diff, s.is_s, s.is_f, s.is_p, params, db, s.bcs_sub_pressure)
    h = _handle(s, {"pc type": pc}, db)
    x = np.random.default_rng(3).standard_normal(s.A.shape[0])
    y, yo = h.pc_apply(x), o.block_pc.apply(x)
    diff = float(np.max(np.abs(y - yo)) / np.max(np.abs(yo)))
    print(f"{problem} N={N} {pc} {inner}: drop against the oracle {diff:.3e}; "
          f"drop against keep {_rel_fields(yo, okeep.block_pc.apply(x), s):.3e}")
    assert _rel_fields(yo, okeep.block_pc.apply(x), s) > 1e-3  # (the zeroed columns matter on this vector)
    if inner == "lu":
        # two exact solves of an ill-conditioned block: the block residuals of tests/test_gpu_sparse_lu.py,
        # against the column-zeroed P
        from test_gpu_sparse_lu import _block_residuals
        rs, rfp = _block_residuals(s, y, x, P=P0)
        print(f"block residuals s {rs:.3e} fp {rfp:.3e}")
        assert rs <= 1e-9 and rfp <= 1e-12
    else:
        assert diff <= 1e-12
    h.destroy()


def test_drop_solve_matches_oracle(gpu, monkeypatch):
    """One full solve through tests/test_gpu_fe.py's _compare and its bounds, the oracle (and the
    perturbed oracles that set the bound) handed the column-zeroed P."""
    import test_gpu_fe as T
    s = _system("swelling", 8, "diagonal 3-way")
    prefixes, db = _drop_case("diagonal 3-way", "lu")
    sets = [_rows_of(s, p) for p in prefixes]

    def zeroed(A, P, *a, **k):
        return OracleSolver(A, B.zero_bc_columns(P, sets), *a, **k)
    monkeypatch.setattr(T, "OracleSolver", zeroed)
    r = T._compare(s, {"pc type": "diagonal 3-way"}, db)
    assert r.reason > 0


# --------------------------------------- 3. lift is the same preconditioner --
def _lifting(ksp, K):
    """The oracle KSP's solve with b' = b - C b in front (the restatement's lift)."""
    _, _, c_rp, c_ci, c_val = B.split(K)
    solve = ksp.solve
    ksp.solve = lambda b: solve(B.lift(b, c_rp, c_ci, c_val))


def _cpu_lift_against_keep(s, P, prefixes, params, x):
    """|lift - keep| / |keep| of one block-PC application with scipy's splu on every block: the blocks of P as
    assembled against K' behind the lift."""
    names = {"s_": "ksp_s", "f_": "ksp_f", "fp_": "ksp_fp"}
    okeep = OracleSolver(s.A, P, s.P_diff, s.is_s, s.is_f, s.is_p, params, _db("lu"), s.bcs_sub_pressure)
    olift = OracleSolver(s.A, B.zero_bc_columns(P, [_rows_of(s, p) for p in prefixes]), s.P_diff, s.is_s, s.is_f,
                         s.is_p, params, _db("lu"), s.bcs_sub_pressure)
    for p in prefixes:
        _lifting(getattr(olift.block_pc, names[p]), B.block_of(P, _rows_of(s, p)))
    return _rel_fields(olift.block_pc.apply(x), okeep.block_pc.apply(x), s)


@pytest.mark.parametrize("problem,N,pc", [
    ("swelling", 8, "diagonal"), ("swelling", 8, "diagonal 3-way"),
    ("footing", 10, "undrained"), ("footing", 10, "undrained 3-way"),
])
def test_lift_is_the_same_preconditioner(gpu, problem, N, pc):
    s = _system(problem, N, pc)
    three = "3-way" in pc
    prefixes = ("s_", "f_") if three else ("s_", "fp_")
    params = dict(BASE, **{"pc type": pc})
    x = np.random.default_rng(7).standard_normal(s.A.shape[0])
    cpu = _cpu_lift_against_keep(s, s.P, prefixes, params, x)  # the same comparison on the CPU
    tol = max(10 * cpu, 1e-12)
    ys = {}
    for mode in ("keep", "lift", "drop"):
        h = _handle(s, {"pc type": pc}, _db("lu", {p + "pls_bc_columns": mode for p in prefixes}))
        ys[mode] = h.pc_apply(x)
        if mode == "lift":
            assert all(h.bc_columns_stats(p)[2] > 0 for p in prefixes)
            assert np.array_equal(h.pc_apply(x), ys[mode])  # (b' is formed again: repeatable)
        h.destroy()
    dl, dd = _rel_fields(ys["lift"], ys["keep"], s), _rel_fields(ys["drop"], ys["keep"], s)
    print(f"{problem} N={N} {pc}: lift against keep {dl:.3e} (CPU {cpu:.3e}, tol {tol:.1e}); drop against keep {dd:.3e}")
    assert dl <= tol
    assert dd > 1e-3


# ------------------------------------------ 4. lift under the inexact set ---
@pytest.mark.parametrize("problem,N,pc", [("swelling", 8, "diagonal"), ("footing", 10, "undrained")])
def test_lift_inexact_s_solve_matches_oracle(gpu, problem, N, pc):
    import robustness as R
    from oracle import boomeramg as BA
    from oracle import petsc as OP
    s = _system(problem, N, pc)
    db = R.load_set("inexact")
    db.update(R.np_options(8))
    db["s_pls_bc_columns"] = "lift"
    params = dict(R.DRIVER[problem], **{"pc type": pc})
    h = _handle(s, params, db)
    x = np.random.default_rng(5).standard_normal(s.A.shape[0])
    y = h.pc_apply(x)
    st = h.ksp_stats("s_")
    h.destroy()
    K = B.block_of(s.P, s.is_s)
    _, Kp, c_rp, c_ci, c_val = B.split(K)
    ksp = OP.KSP(Kp, BA.PCBoomerAMG(Kp, db, "s_"), ksp_type="cg", rtol=1e-1, atol=0.0, maxit=10000,
                 norm_type="unpreconditioned")
    ys = ksp.solve(B.lift(x[s.is_s], c_rp, c_ci, c_val))
    print(f"{problem} N={N}: s_ stats {st}, oracle its {ksp.its} reason {ksp.reason}")
    assert st[0] == 1 and st[1] == ksp.its and st[3] == 0 and ksp.reason > 0
    assert ksp.its <= 15
    assert np.max(np.abs(y[s.is_s] - ys)) <= 1e-8 * np.max(np.abs(ys))


# ------------------------------------------------- 5. the stall is gone -----
def test_footing_n20_inexact_lift_converges(gpu):
    import robustness as R
    ref = json.load(open(os.path.join(HERE, "golden", "bc_columns", "footing_N20_inexact_lift.json")))
    r = R.run_case(ref["problem"], ref["N"], ref["pc_type"], "inexact-lift", ref["np"], history=True)
    inner = r["inner"]["s_"]
    print(f"outer its {r['its']} reason {r['reason']} (oracle {ref['its']}, perturbed {ref['perturbed_its']}); "
          f"s_ {inner} (oracle {ref['s_its']} its over {ref['s_solves']} solves, max {ref['s_max']}); "
          f"setup {r['setup_s']} s, solve {r['solve_s']} s")
    assert r["reason"] > 0
    assert inner["negative_reason"] == 0
    # 2 x: slack for the count sensitivity of an inner CG at rtol 1e-1, not a performance bar
    assert inner["max"] <= 2 * ref["s_max"]
    pert = ref["perturbed_its"] + [ref["its"]]
    assert 0.95 * min(pert) <= r["its"] <= 1.05 * max(pert), (r["its"], pert)


# --------------------------------------- 6. refusals and the update path ----
def _inexact_db(extra):
    import robustness as R
    db = R.load_set("inexact")
    db.update(R.np_options(1))
    db.update(extra)
    return db


@pytest.mark.parametrize("key,value,pc,words", [
    ("s_pls_bc_columns", "zap", "diagonal", "keep, lift, drop"),
    ("fp_pls_bc_columns", "lift", "diagonal", "fp_fieldsplit_"),       # the fp_ solver over a fieldsplit
    ("fp_pls_bc_columns", "drop", "diagonal", "fp_fieldsplit_"),
    ("fp_fieldsplit_1_pls_bc_columns", "lift", "diagonal", "not a stored matrix"),  # the Schur split
    ("global_pls_bc_columns", "lift", "diagonal", "handed its preconditioner"),
])
def test_refusals(gpu, key, value, pc, words):
    import robustness as R
    s = _system("swelling", 4, pc)
    h = _handle(s, dict(R.DRIVER["swelling"], **{"pc type": pc}), _inexact_db({key: value}))
    with pytest.raises(RuntimeError) as e:
        h.setup()
        h.create_solver()
    assert key in str(e.value) and words in str(e.value), str(e.value)
    h.destroy()


def test_unknown_prefix(gpu):
    s = _system("swelling", 4, "diagonal")
    h = _handle(s, {"pc type": "diagonal"}, _db("ilu"))
    with pytest.raises(RuntimeError, match="nope_"):
        h.bc_columns_stats("nope_")
    with pytest.raises(ValueError, match="nope_"):
        h.bc_columns_matrix("nope_")
    assert h.bc_columns_stats("s_") == (0, 0, 0, 0, 0)
    h.destroy()


def test_update_matrices_splits_again(gpu):
    """P with one more identity row in the s block: the stats, C and a solve follow the new matrix."""
    import scipy.sparse as sp
    s = _system("swelling", 8, "diagonal")
    is_s = np.asarray(s.is_s)
    K = B.block_of(s.P, is_s)
    bc = B.identity_rows(K)
    free = np.setdiff1d(np.arange(K.shape[0]), bc)
    r = int(is_s[free[free.size // 2]])
    P2 = sp.csr_matrix(s.P, copy=True)
    P2.sort_indices()
    seg = slice(P2.indptr[r], P2.indptr[r + 1])
    P2.data[seg] = np.where(P2.indices[seg] == r, 1.0, 0.0)
    K2 = B.block_of(P2, is_s)
    assert B.identity_rows(K2).size == bc.size + 1
    db = _db("lu", {"s_pls_bc_columns": "lift"})
    h = _handle(s, {"pc type": "diagonal"}, db)
    st1 = _check_split(h, K, "s_", 1)
    x1, r1 = h.solve(s.b)
    x1b, r1b = h.solve(s.b)
    assert r1.reason > 0 and r1b.its == r1.its and np.array_equal(x1, x1b)  # a second identical solve: bitwise
    h.update_matrices(None, P2, None)
    st2 = _check_split(h, K2, "s_", 1)
    assert st2[1] == st1[1] + 1 and st2[2] > st1[2]
    v = np.random.default_rng(2).standard_normal(s.A.shape[0])
    hk = _handle(s, {"pc type": "diagonal"}, _db("lu"), P=P2)
    y, yk = h.pc_apply(v), hk.pc_apply(v)
    hold = _handle(s, {"pc type": "diagonal"}, _db("lu"))
    cpu = _cpu_lift_against_keep(s, P2, ("s_",), dict(BASE, **{"pc type": "diagonal"}), v)
    print(f"after the update: lift against keep on the new P {_rel_fields(y, yk, s):.3e} (CPU {cpu:.3e}), "
          f"on the old P {_rel_fields(y, hold.pc_apply(v), s):.3e}")
    assert _rel_fields(y, yk, s) <= max(10 * cpu, 1e-12)  # (the bound of test_lift_is_the_same_preconditioner)
    assert _rel_fields(y, hold.pc_apply(v), s) > 1e-6
    x2, r2 = h.solve(s.b)
    assert r2.reason > 0
    for q in (h, hk, hold):
        q.destroy()
