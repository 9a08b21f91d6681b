"""Overlapping additive Schwarz on the device (<prefix>pc_type asm; csrc/asm.hip, csrc/asm.cpp)
against the numpy restatement tests/asm_restatement.py (pinned by tests/test_asm_restatement.py).

Subdomains: Handle.asm_rows / asm_stats equal the restatement's exactly.  PC apply: <= 1e-13
relative (max norm), the project's bar for a PC application.  Solves: iteration count and reason
exact, every history entry within max(1e-10, 10 x the restatement's own worst deviation over 4
seeds when every inner PC output is perturbed by 1e-15 relative) -- tests/test_gpu_iluk.py's
rule, whose _noise_floor is copied here.  Identities (overlap 0 = bjacobi, one block = ilu, the
fused kernel = the generic path) are np.array_equal.

Sizes: synthetic 2-D N = 6 (s block 338 rows, fp block 387) and 3-D N = 4 (2,187 and 2,312), B = 3 and
B = 7 (uneven sizes).  The oracle is built from the options with bjacobi and gets the restated
PCs installed in its inner KSPs.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from asm_restatement import PCASM, TYPES
from ksp_restatements import fgmres
from oracle import synthetic as S
from oracle.solver import OracleSolver

pytestmark = pytest.mark.gpu

BASE = {"solver type": "gmres", "solver atol": 1e-8, "solver rtol": 1e-6, "solver maxiter": 300,
        "pc type": "diagonal", "inner ksp type": "preonly", "inner pc type": "ilu", "inner rtol": 1e-6,
        "inner atol": 0, "inner maxiter": 1000, "inner monitor": False, "solver monitor": False,
        "inner accel order": 0, "AAR order": 10, "AAR p": 5, "AAR omega": 1, "AAR beta": 1}
TWO, THREE = ("s_", "fp_"), ("s_", "f_", "p_", "diff_")
KSP_OF = {"s_": "ksp_s", "fp_": "ksp_fp", "f_": "ksp_f", "p_": "ksp_p", "diff_": "ksp_p_diff"}
INNER = ("ksp_s", "ksp_fp", "ksp_f", "ksp_p")
SPECS = {"2d6": S.SynthSpec(2, 6), "3d4": S.SynthSpec(3, 4)}
VIEW = {"pls.ilu_view": "1"}
# the inner sweep of these small blocks may be the chain or window kernel; with both off it is the
# plain LDS sweep, the one the fused kernel serves
LDS = {"pls.sweep_chain": "0", "pls.sweep_window": "0"}


def _db(prefixes, pc, B=3, overlap=1, atype=None, levels=None, extra=None):
    """preonly + asm / bjacobi / ilu on every prefix."""
    db = {"global_ksp_type": "gmres", "global_ksp_pc_side": "right"}
    for pre in prefixes:
        db[pre + "ksp_type"] = "preonly"
        db[pre + "pc_type"] = pc
        if pc == "bjacobi":
            db[pre + "pc_bjacobi_blocks"] = str(B)
        if pc == "asm":
            db[pre + "pc_asm_blocks"] = str(B)
            db[pre + "pc_asm_overlap"] = str(overlap)
            if atype is not None:
                db[pre + "pc_asm_type"] = atype
        if levels is not None:
            db[pre + ("pc_factor_levels" if pc == "ilu" else "sub_pc_factor_levels")] = str(levels)
    db.update(extra or {})
    return db


def _handle(spec, params, db):
    from lib.handle import Handle, params_to_options
    opts = dict(db)
    opts.update(params_to_options(params))
    return Handle.synthetic(spec.dim, spec.N, spec.seed, spec.delta, opts)


_restated = {}


def _restate(key, M, B, overlap, atype, k):
    """The restated PC of a block, computed once per key and left unchanged."""
    key = key + (B, overlap, atype, k)
    if key not in _restated:
        # 3-D blocks: PCILUk's fast path (pinned equal to the plain one by tests/test_iluk_restatement.py)
        _restated[key] = PCASM(M, min(B, M.shape[0]), overlap, atype, k, fast=key[0] == "3d4")
    return _restated[key]


def _oracle(name, params, prefixes, B=3, overlap=1, atype="restrict", k=0, system=None, extra=None, tag=None):
    """The oracle on the db with bjacobi, the restated asm PCs installed."""
    spec = SPECS[name]
    A, P, Pd = system if system is not None else (S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2))
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    o = OracleSolver(A, P, Pd, is_s, is_f, is_p, params, _db(prefixes, "bjacobi", extra=extra), S.bcs_sub_pressure(spec))
    for pre in prefixes:
        ksp = getattr(o.block_pc, KSP_OF[pre])
        ksp.pc = _restate((name, tag, pre), ksp.A, B, overlap, atype, k)
    return o


def _noise_floor(o, b, ho, its, eps=1e-15, seeds=4):
    """Worst relative deviation of the restatement's own history over the seeds
    (every inner PC output perturbed by eps relative); its count must not move."""
    worst = 0.0
    for seed in range(seeds):
        rng = np.random.default_rng(seed)
        saved = []
        for name in INNER:
            ksp = getattr(o.block_pc, name, None)
            if ksp is None:
                continue
            orig = ksp.pc.apply
            saved.append((ksp.pc, orig))
            ksp.pc.apply = (lambda f: lambda x: (lambda y: y * (1 + eps * rng.standard_normal(y.size)))(f(x)))(orig)
        o.solve(b)
        for pc, orig in saved:
            pc.apply = orig
        assert o.its == its, f"bad input: the restatement takes {o.its} iterations with seed {seed}, {its} without"
        h2 = np.asarray(o.history)
        worst = max(worst, float(np.max(np.abs(h2 - ho) / np.abs(ho))))
    return worst


def _rel(y, yo):
    return float(np.max(np.abs(y - yo)) / np.max(np.abs(yo)))


def _check_rows(h, o, prefixes, fused=None):
    """asm_rows and asm_stats of every prefix equal the restatement's."""
    for pre in prefixes:
        pc = getattr(o.block_pc, KSP_OF[pre]).pc
        ptr, rows = h.asm_rows(pre)
        stats = h.asm_stats(pre)
        print(pre, "asm_stats", stats, "restatement", pc.stats(stats[5]))
        assert np.array_equal(ptr, pc.ptr) and ptr.dtype == np.int64
        assert np.array_equal(rows, np.concatenate(pc.rows)) and rows.dtype == np.int32
        assert stats == pc.stats(stats[5] if fused is None else fused)


# ------------------------------------------------------------ subdomains ----
@pytest.mark.parametrize("B", [3, 7])
@pytest.mark.parametrize("overlap", [0, 1, 2])
@pytest.mark.parametrize("name", list(SPECS))
def test_subdomains(gpu, name, overlap, B):
    o = _oracle(name, BASE, TWO, B, overlap)
    h = _handle(SPECS[name], BASE, _db(TWO, "asm", B, overlap, extra=LDS))
    h.setup()
    _check_rows(h, o, TWO, fused=1)  # a few hundred / thousand rows: LDS-resident, the fused kernel
    h.destroy()


def _one_sided_system(spec, count=40, seed=9):
    """tests/test_gpu_iluk.py's: `count` entries added to P's s block on one side of the diagonal only."""
    A, P, Pd = S.matrix(spec, 0), sp.lil_matrix(S.matrix(spec, 1)), S.matrix(spec, 2)
    is_s = np.asarray(S.field_major_index_sets(spec)[0])
    pat = sp.csr_matrix(S.matrix(spec, 1))
    rng = np.random.default_rng(seed)
    added = 0
    while added < count:
        i, j = (int(v) for v in rng.choice(is_s, 2, replace=False))
        if abs(i - j) > 40 or pat[i, j] != 0 or pat[j, i] != 0 or P[i, j] != 0 or P[j, i] != 0:
            continue
        P[i, j] = 1e-2 * rng.standard_normal()
        added += 1
    P = sp.csr_matrix(P)
    P.sort_indices()
    return A, P, Pd


@pytest.mark.parametrize("B,overlap", [(48, 1), (7, 2)])
def test_subdomains_of_a_nonsymmetric_pattern(gpu, B, overlap):
    from lib.handle import Handle, params_to_options
    spec = SPECS["2d6"]
    system = _one_sided_system(spec)
    A, P, Pd = system
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    o = _oracle("2d6", BASE, TWO, B, overlap, system=system, tag="one-sided")
    sym = _oracle("2d6", BASE, TWO, B, overlap)
    opts = _db(TWO, "asm", B, overlap)
    opts.update(params_to_options(BASE))
    h = Handle.from_csr(A, P, Pd, is_s, is_f, is_p, S.bcs_sub_pressure(spec), opts)
    h.setup()
    _check_rows(h, o, TWO)
    if B == 48:
        # 48 blocks of 7 rows, one round: the 40 one-sided entries reach rows the symmetric pattern does not
        # (4,094 rows in all against 4,083), and a search over the transposed pattern reaches others (4,092).
        # With 7 blocks and two rounds the sets happen to agree: every one-sided target is already inside.
        pc = o.block_pc.ksp_s.pc
        assert not np.array_equal(np.concatenate(pc.rows), np.concatenate(sym.block_pc.ksp_s.pc.rows))
        tr = PCASM(sp.csr_matrix(o.block_pc.ksp_s.A).T.tocsr(), B, overlap)
        assert not np.array_equal(np.concatenate(pc.rows), np.concatenate(tr.rows))
        assert (int(pc.ptr[-1]), int(sym.block_pc.ksp_s.pc.ptr[-1]), int(tr.ptr[-1])) == (4094, 4083, 4092)
    x = np.random.default_rng(7).standard_normal(spec.n)
    assert _rel(h.pc_apply(x), o.block_pc.apply(x)) <= 1e-13
    h.destroy()


def test_overlap_that_covers_the_whole_block(gpu):
    spec = SPECS["2d6"]
    o = _oracle("2d6", BASE, TWO, 3, 400)
    for pre in TWO:
        pc = getattr(o.block_pc, KSP_OF[pre]).pc
        assert all(r.size == pc.n for r in pc.rows)
    h = _handle(spec, BASE, _db(TWO, "asm", 3, 400))
    h.setup()
    _check_rows(h, o, TWO)
    x = np.random.default_rng(12).standard_normal(spec.n)
    assert _rel(h.pc_apply(x), o.block_pc.apply(x)) <= 1e-13
    h.destroy()


def test_one_block_per_row(gpu):
    """pc_asm_blocks = n (338 and 387 blocks: more than the growth kernel's 256 workgroups), overlap 1."""
    spec = SPECS["2d6"]
    db = _db(TWO, "asm", 1, 1, extra={"s_pc_asm_blocks": "338", "fp_pc_asm_blocks": "387"})
    o = _oracle("2d6", BASE, TWO, 10 ** 6, 1)  # (_restate: min(B, n))
    assert o.block_pc.ksp_s.pc.nblocks == 338 and o.block_pc.ksp_fp.pc.nblocks == 387
    h = _handle(spec, BASE, db)
    h.setup()
    _check_rows(h, o, TWO)
    x = np.random.default_rng(13).standard_normal(spec.n)
    assert _rel(h.pc_apply(x), o.block_pc.apply(x)) <= 1e-13
    h.destroy()


# -------------------------------------------------------------- PC apply ----
@pytest.mark.parametrize("atype", TYPES)
@pytest.mark.parametrize("overlap", [1, 2])
@pytest.mark.parametrize("name,B", [("2d6", 3), ("2d6", 7), ("3d4", 3)])
def test_pc_apply(gpu, name, B, overlap, atype):
    o = _oracle(name, BASE, TWO, B, overlap, atype)
    h = _handle(SPECS[name], BASE, _db(TWO, "asm", B, overlap, atype))
    x = np.random.default_rng(5).standard_normal(SPECS[name].n)
    y, yo = h.pc_apply(x), o.block_pc.apply(x)
    print(f"PC apply rel diff {_rel(y, yo):.3e}")
    assert _rel(y, yo) <= 1e-13
    assert h.asm_stats("s_")[2] == TYPES.index(atype)
    h.destroy()


def test_pc_apply_differs_from_bjacobi_and_between_types(gpu):
    spec = SPECS["2d6"]
    x = np.random.default_rng(5).standard_normal(spec.n)
    ys = []
    for db in [_db(TWO, "bjacobi")] + [_db(TWO, "asm", 3, 1, t) for t in TYPES]:
        h = _handle(spec, BASE, db)
        ys.append(h.pc_apply(x))
        h.destroy()
    for i in range(5):
        for j in range(i):
            assert _rel(ys[i], ys[j]) > 1e-6


def test_pc_apply_levels_1(gpu):
    o = _oracle("2d6", BASE, TWO, 3, 1, "restrict", 1)
    h = _handle(SPECS["2d6"], BASE, _db(TWO, "asm", 3, 1, levels=1))
    x = np.random.default_rng(6).standard_normal(SPECS["2d6"].n)
    y, yo = h.pc_apply(x), o.block_pc.apply(x)
    assert _rel(y, yo) <= 1e-13
    for pre in TWO:  # pls_get_ilu_fill reports the factors of the extended matrix
        pc = getattr(o.block_pc, KSP_OF[pre]).pc
        M = sp.csr_matrix(getattr(o.block_pc, KSP_OF[pre]).A)
        nnz0 = sum(M[r][:, r].nnz for r in pc.rows)
        assert h.ilu_fill(pre) == (1, nnz0, pc.nnz, pc.max_row)
    h.destroy()


@pytest.mark.parametrize("atype", ["restrict", "basic"])
def test_pc_apply_three_way(gpu, atype):
    params = dict(BASE, **{"pc type": "diagonal 3-way"})
    o = _oracle("2d6", params, THREE, 3, 1, atype)
    h = _handle(SPECS["2d6"], params, _db(THREE, "asm", 3, 1, atype))
    x = np.random.default_rng(8).standard_normal(SPECS["2d6"].n)
    y, yo = h.pc_apply(x), o.block_pc.apply(x)
    assert _rel(y, yo) <= 1e-13
    _check_rows(h, o, THREE)
    h.destroy()


# ------------------------------------------------------------ identities ----
def _apply_and_solve(spec, db):
    h = _handle(spec, BASE, db)
    x = np.random.default_rng(9).standard_normal(spec.n)
    y = h.pc_apply(x)
    sol, r = h.solve(S.rhs(spec))
    out = (y, sol, h.history(), r.its, r.reason)
    return h, out


@pytest.mark.parametrize("B", [3, 7])
@pytest.mark.parametrize("name", list(SPECS))
def test_overlap_0_is_bjacobi(gpu, name, B):
    spec = SPECS[name]
    ha, a = _apply_and_solve(spec, _db(TWO, "asm", B, 0))
    hb, b = _apply_and_solve(spec, _db(TWO, "bjacobi", B))
    assert ha.asm_stats("s_")[3] == ha.ns
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3:] == b[3:]
    ha.destroy(), hb.destroy()


@pytest.mark.parametrize("name", list(SPECS))
def test_one_block_is_ilu(gpu, name):
    spec = SPECS[name]
    ha, a = _apply_and_solve(spec, _db(TWO, "asm", 1, 1))
    hb, b = _apply_and_solve(spec, _db(TWO, "ilu"))
    assert ha.asm_stats("s_")[:2] == (1, 1) and ha.asm_stats("s_")[3] == ha.ns
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3:] == b[3:]
    ha.destroy(), hb.destroy()


@pytest.mark.parametrize("atype", TYPES)
@pytest.mark.parametrize("name,B,overlap", [("2d6", 7, 1), ("2d6", 3, 2), ("3d4", 3, 1)])
def test_fused_equals_generic(gpu, name, B, overlap, atype):
    spec = SPECS[name]
    hf, f = _apply_and_solve(spec, _db(TWO, "asm", B, overlap, atype, extra=LDS))
    hg, g = _apply_and_solve(spec, _db(TWO, "asm", B, overlap, atype, extra=dict(LDS, **{"pls.asm_fused": "0"})))
    for pre in TWO:
        assert hf.asm_stats(pre)[5] == 1 and hg.asm_stats(pre)[5] == 0
        assert hf.asm_stats(pre)[:5] == hg.asm_stats(pre)[:5]
    assert np.array_equal(f[0], g[0]) and np.array_equal(f[1], g[1]) and np.array_equal(f[2], g[2])
    assert f[3:] == g[3:]
    hf.destroy(), hg.destroy()


@pytest.mark.parametrize("forced,kinds", [({"pls.ilu_lds": "0"}, {"levels", "levels-csr"}),
                                          ({"pls.ilu_gmem": "-2"}, None)], ids=["ilu_lds0", "ilu_gmem-2"])
@pytest.mark.parametrize("atype", ["restrict", "basic"])
def test_other_inner_sweeps_take_the_generic_path(gpu, capfd, atype, forced, kinds):
    o = _oracle("2d6", BASE, TWO, 3, 1, atype)
    capfd.readouterr()
    h = _handle(SPECS["2d6"], BASE, _db(TWO, "asm", 3, 1, atype, extra=dict(forced, **VIEW)))
    x = np.random.default_rng(10).standard_normal(SPECS["2d6"].n)
    y, yo = h.pc_apply(x), o.block_pc.apply(x)
    err = capfd.readouterr().err.splitlines()
    ilu = [ln for ln in err if ln.startswith("[pls ilu]")]
    asm = [ln for ln in err if ln.startswith("[pls asm]")]
    print("\n".join(ilu + asm))
    assert len(ilu) == 2 and len(asm) == 2
    got = {ln.split(" sweep ")[1].split(" ")[0] for ln in ilu}
    if kinds is not None:
        assert got <= kinds, got
        assert all(h.asm_stats(pre)[5] == 0 for pre in TWO) and all(ln.endswith("fused no") for ln in asm)
    else:  # pls.ilu_gmem -2 keeps LDS-resident blocks in the LDS sweep: whichever path, the stats say which
        assert all((h.asm_stats(pre)[5] == 1) == ln.endswith("fused yes") for pre, ln in zip(TWO, asm))
    assert _rel(y, yo) <= 1e-13
    h.destroy()


def test_the_view_line(gpu, capfd):
    capfd.readouterr()
    h = _handle(SPECS["2d6"], BASE, _db(TWO, "asm", 3, 1, "basic", extra=dict(LDS, **VIEW)))
    h.setup()
    asm = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[pls asm]")]
    st = h.asm_stats("s_")
    assert asm[0] == (f"[pls asm] prefix s_ blocks 3 overlap 1 type basic rows {st[3]} ({st[3] / h.ns:.3f} n) "
                      f"largest {st[4]} fused yes")
    h.destroy()


def test_basic_is_reproducible(gpu):
    spec = SPECS["3d4"]
    h = _handle(spec, BASE, _db(TWO, "asm", 7, 2, "basic"))
    x = np.random.default_rng(11).standard_normal(spec.n)
    y1, y2 = h.pc_apply(x), h.pc_apply(x)
    h.destroy()
    h2 = _handle(spec, BASE, _db(TWO, "asm", 7, 2, "basic"))
    y3 = h2.pc_apply(x)
    h2.destroy()
    assert np.array_equal(y1, y2) and np.array_equal(y1, y3)


# ---------------------------------------------------------------- solves ----
def _solve_case(name, params, prefixes, db_extra, oracle_extra, install=None, B=3, overlap=1, atype="restrict"):
    spec = SPECS[name]
    b = S.rhs(spec)
    o = _oracle(name, params, prefixes, B, overlap, atype, extra=oracle_extra)
    if install:
        install(o)
    xo = o.solve(b)
    its, reason, ho = o.its, o.reason, np.asarray(o.history)
    tol = max(1e-10, 10 * _noise_floor(o, b, ho, its))
    h = _handle(spec, params, _db(prefixes, "asm", B, overlap, atype, extra=db_extra))
    x, r = h.solve(b)
    hist = h.history()
    print(f"its {r.its} (restatement {its}) reason {r.reason} ({reason}) history tol {tol:.2e}")
    assert r.its == its, f"its {r.its} vs restatement {its}"
    assert r.reason == reason, f"reason {r.reason} vs restatement {reason}"
    assert hist.shape == ho.shape
    rel = np.max(np.abs(hist - ho) / np.abs(ho))
    print(f"history rel diff {rel:.3e}; |x - x_o| / |x_o| {np.linalg.norm(x - xo) / np.linalg.norm(xo):.3e}")
    assert rel <= tol, f"residual history rel diff {rel:.3e} (tol {tol:.1e})"
    assert np.linalg.norm(x - xo) <= max(1e-8, tol) * np.linalg.norm(xo)
    h.destroy()
    return its


@pytest.mark.parametrize("name,side,B,overlap", [("2d6", "right", 3, 1), ("2d6", "right", 7, 2), ("2d6", "left", 3, 1),
                                                 ("3d4", "right", 3, 1)])
def test_solve_gmres(gpu, name, side, B, overlap):
    extra = {"global_ksp_pc_side": side}
    its = _solve_case(name, BASE, TWO, extra, extra, B=B, overlap=overlap)
    if (side, B) == ("right", 3):  # tests/test_asm_restatement.py's table
        assert its == {"2d6": 12, "3d4": 11}[name]


def test_solve_gmres_three_way_basic(gpu):
    _solve_case("2d6", dict(BASE, **{"pc type": "diagonal 3-way"}), THREE, None, None, atype="basic")


def test_solve_fgmres(gpu):
    extra = {"global_ksp_type": "fgmres"}

    def install(o):
        o.solver.solve = lambda b: fgmres(o.solver, b)

    _solve_case("2d6", BASE, TWO, extra, extra, install)


def test_solve_inner_gmres_under_fgmres(gpu):
    extra = {"global_ksp_type": "fgmres", "s_ksp_type": "gmres", "s_ksp_rtol": "1e-2", "s_ksp_max_it": "20"}

    def install(o):
        o.solver.solve = lambda b: fgmres(o.solver, b)

    _solve_case("2d6", BASE, TWO, extra, extra, install)


def test_update_matrices_rebuilds_the_subdomains(gpu):
    """New values and a new pattern (the one-sided entries): apply and subdomains follow."""
    from lib.handle import Handle, params_to_options
    spec = SPECS["2d6"]
    A, P, Pd = S.matrix(spec, 0), S.matrix(spec, 1), S.matrix(spec, 2)
    is_s, is_f, is_p = S.field_major_index_sets(spec)
    opts = _db(TWO, "asm", 7, 1)
    opts.update(params_to_options(BASE))
    h = Handle.from_csr(A, P, Pd, is_s, is_f, is_p, S.bcs_sub_pressure(spec), opts)
    x = np.random.default_rng(14).standard_normal(spec.n)
    o1 = _oracle("2d6", BASE, TWO, 7, 1)
    assert _rel(h.pc_apply(x), o1.block_pc.apply(x)) <= 1e-13
    A2, P2, Pd2 = _one_sided_system(spec)
    P2 = (1.25 * P2).tocsr()
    h.update_matrices(None, P2, None)
    o2 = _oracle("2d6", BASE, TWO, 7, 1, system=(A2, P2, Pd2), tag="updated")
    y, yo = h.pc_apply(x), o2.block_pc.apply(x)
    assert _rel(y, yo) <= 1e-13 and _rel(y, o1.block_pc.apply(x)) > 1e-3
    _check_rows(h, o2, TWO)
    h.destroy()


# -------------------------------------------------------------- refusals ----
@pytest.mark.parametrize("key,value,match", [
    ("s_pc_asm_local_type", "multiplicative", r"s_pc_asm_local_type multiplicative"),
    ("fp_sub_pc_type", "lu", r"fp_sub_pc_type lu"),
    ("s_pc_asm_overlap", "-1", r"s_pc_asm_overlap.*non-negative"),
    ("s_pc_asm_overlap", "1.5", r"s_pc_asm_overlap.*integer"),
    ("fp_pc_asm_type", "restricted", r"fp_pc_asm_type restricted"),
    ("s_pc_asm_blocks", "0", r"s_pc_asm_blocks 0"),
    ("s_pc_asm_blocks", "339", r"s_pc_asm_blocks 339.*338"),
])
def test_refusals_name_the_key(gpu, key, value, match):
    h = _handle(SPECS["2d6"], BASE, dict(_db(TWO, "asm", 3, 1), **{key: value}))
    with pytest.raises(RuntimeError, match=match):
        h.setup()
    h.destroy()


def test_asm_without_a_block_count_is_refused(gpu):
    """The block count has no default here (PETSc's one block per rank would be plain ilu)."""
    db = _db(TWO, "asm", 3, 1)
    del db["s_pc_asm_blocks"]
    h = _handle(SPECS["2d6"], BASE, db)
    with pytest.raises(RuntimeError, match=r"'asm'.*s_pc_asm_blocks"):
        h.setup()
    h.destroy()


def test_asm_entries_refuse_other_pcs(gpu):
    h = _handle(SPECS["2d6"], BASE, dict(_db(TWO, "asm", 3, 1), fp_pc_type="bjacobi", fp_pc_bjacobi_blocks="3"))
    h.setup()
    with pytest.raises(RuntimeError, match="pls_get_asm_stats.*fp_.*bjacobi.*not asm"):
        h.asm_stats("fp_")
    with pytest.raises(RuntimeError, match="pls_get_asm_stats.*no inner solver.*nope_"):
        h.asm_rows("nope_")
    assert h.asm_stats("s_")[0] == 3
    h.destroy()
