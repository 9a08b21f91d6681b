"""The preconditions of tests/sweep_cases.py, on the CPU.

For every case: the properties of the pattern that the case's table row names (row lengths per
triangle, off-window entries and records per triangle, reach, widest level, block lengths), a numpy
restatement of PCILU::choose_sweep (csrc/ilu.cpp) from those numbers that must give the kind each
run lists, and the reference conditions -- the "int" and "unit" data's factors are ILU(0) of K bitwise
with every magnitude far below 2^53, the float64 restatement of the windowed solve returns y* on the
"unit" data (it does not on the "int" data: that is why the inverse kinds run "unit"), and on the
"normal" data the float64 oracle and a float64 restatement of the windowed solve stay within 1e-14
and 1e-13 of the np.longdouble reference.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import sweep_cases as C
from oracle import native


def _ceil(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def stats(case_id):
    """What choose_sweep reads off the block-truncated pattern."""
    case = C.BY_ID[case_id]
    T = C.truncated(case, C.pattern(*case.pattern))
    n, bst = case.n, C.block_starts(case)
    r, c = C.coords(T)
    # max_len as PCILU::factor leaves it: n / blocks + 1, or the longest block where that is longer
    s = SimpleNamespace(n=n, nb=case.blocks, bst=bst, blen=max(n // case.blocks + 1, int(np.diff(bst).max())))
    s.lenL = np.bincount(r[c < r], minlength=n)
    s.lenU = np.bincount(r[c > r], minlength=n)
    s.nlev_L, s.lvL = native.levels(T, lower=True)  # (no entry crosses a block: global levels are the blocks')
    _, s.lvU = native.levels(T, lower=False)
    blk = np.searchsorted(bst, np.arange(n), side="right") - 1
    s.blk = blk
    # levels per block, width of every (block, level)
    s.widthL = [np.bincount(s.lvL[bst[b]:bst[b + 1]]) for b in range(case.blocks)]
    s.widthU = [np.bincount(s.lvU[bst[b]:bst[b + 1]]) for b in range(case.blocks)]
    s.levL, s.levU = sum(len(w) for w in s.widthL), sum(len(w) for w in s.widthU)
    s.widest = max(max(w.max() for w in s.widthL), max(w.max() for w in s.widthU))
    s.nw = int(sum(_ceil(bst[b + 1] - bst[b], 64) for b in range(case.blocks)))
    # off-window entries: windows of 64 rows from the block's first row
    w0 = bst[blk[r]] + (r - bst[blk[r]]) // 64 * 64
    w1 = np.minimum(w0 + 64, bst[blk[r] + 1])
    s.offL = np.bincount(r[c < w0], minlength=n)
    s.offU = np.bincount(r[c >= w1], minlength=n)
    s.eL, s.eU = int(s.offL.max()), int(s.offU.max())
    s.reach = int(np.abs(r - c).max())
    return s


def records(e):
    return 4 if e <= 16 else 6 if e <= 24 else 8


def chain_steps(s, lens, widths):
    """build_chain_tri's dry run: the steps of one triangle, or -1 where a row does not fit 16 lanes x 7."""
    total = 0
    for b in range(s.nb):
        mx = int(lens[s.bst[b]:s.bst[b + 1]].max())
        lpr = 1
        while lpr < 16 and _ceil(mx, lpr) > C.LANE_ENTRIES:
            lpr *= 2
        if _ceil(mx, lpr) > C.LANE_ENTRIES:
            return -1
        total += int(sum(_ceil(int(w), 16 // lpr) for w in widths[b]))
    return total


def restated_kind(s, o):
    """PCILU::choose_sweep for the options o (pls.* keys, strings).  Left out: the y-resident sweeps' row
    limit (ilu_gmem_max_rows() is INT_MAX) and the envelope LU (`exact`), which no case here runs."""
    g = lambda k, d: int(o.get("pls." + k, d))  # noqa: E731
    allow_lds, gmem_mode, ring_mode = g("ilu_lds", 1) != 0, g("ilu_gmem", 0), g("ilu_ring", 1)
    sweep_chain, sweep_window, window_ring = g("sweep_chain", -1), g("sweep_window", -1), g("window_ring", -1)
    window_mixed, sweep_swin, force_lpr = g("window_mixed", -1), g("sweep_swin", 0), g("sweep_lpr", 0)
    fits_lds = s.blen <= C.LDS_ROWS and gmem_mode != 1
    narrow = s.nlev_L > 0 and s.n // s.nlev_L <= 2048
    gmem = allow_lds and not fits_lds and gmem_mode >= 0 and (narrow or s.nb >= 64 or gmem_mode == 1)
    if not (s.nb >= 64 or (fits_lds and allow_lds) or gmem):
        return "levels-csr" if gmem_mode == -2 else "levels"
    if not ((allow_lds and fits_lds) or gmem):
        return "levels"
    lev = s.levL + s.levU
    ring_fits = window_ring != 0 and s.blen <= C.WINDOW_RING_ROWS and s.reach <= C.WINDOW_RING_REACH
    entries_fit = max(s.eL, s.eU) <= C.WINDOW_ENTRIES
    if gmem:
        if sweep_swin != 0 and (sweep_swin == 1 or ring_mode != 0):
            return "swin"
        if sweep_window != 0 and ring_fits:
            cost_win, cost_mix = 2 * s.nw, s.levL + s.nw
            mix = window_mixed == 1 or (window_mixed == -1 and cost_mix < cost_win)
            cost = cost_mix if mix else cost_win
            if (sweep_window == 1 or (gmem_mode != 1 and 5 * cost <= 4 * lev)) and entries_fit:
                return "levels+window-ring" if mix else "window-ring"
        return "ring" if ring_mode != 0 and s.widest <= C.RING_CHUNK else "gmem"
    if (sweep_chain != 0 or sweep_window == 1) and force_lpr == 0:
        sL = chain_steps(s, s.lenL, s.widthL)
        sU = -1 if sL < 0 else chain_steps(s, s.lenU, s.widthU)
        deep = sL >= 0 and sU >= 0 and 2 * (sL + sU) <= 7 * lev
        chain = sweep_chain != 0 and sL >= 0 and sU >= 0 and (sweep_chain == 1 or deep)
        many_levels = lev >= 2 * (2 * s.nw)
        if ((sweep_window == 1 or (sweep_window == -1 and sweep_chain != 1 and (deep or many_levels)))
                and s.blen <= C.WINDOW_ROWS and entries_fit):
            return "window-ring" if window_ring == 1 and ring_fits else "window"
        if chain:
            return "chain"
    return "lds"


def ring_rows(s, upper):
    """ring_tables (csrc/ilu.cpp) of a one-block case: level-order positions (rows of a level longest
    first, stable), level-aligned chunks of at most 4,096 positions, row_lo = the end of the row's
    chunk - 16,384.  Returns (posof, row_lo)."""
    lvl, lens = (s.lvU, s.lenU) if upper else (s.lvL, s.lenL)
    rows = np.arange(s.n)  # (block_level_groups keeps a level's rows ascending in both triangles)
    order = rows[np.lexsort((rows, -lens, lvl))]
    posof = np.empty(s.n, dtype=np.int64)
    posof[order] = np.arange(s.n)
    grp = np.concatenate([[0], np.cumsum(np.bincount(lvl))])
    row_lo = np.empty(s.n, dtype=np.int64)
    g = 0
    while g < len(grp) - 1:
        e = g + 1
        while e < len(grp) - 1 and grp[e + 1] - grp[g] <= C.RING_CHUNK:
            e += 1
        row_lo[order[grp[g]:grp[e]]] = grp[e] - C.RING_SLOTS
        g = e
    return posof, row_lo


CASES = pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)


def test_every_kind_is_expected_in_three_cases():
    for kind in C.KINDS:
        cases = [c.id for c in C.CASES if kind in c.runs.values()]
        assert len(cases) >= 3, (kind, cases)
    assert all(set(c.runs) <= set(C.RUNS) for c in C.CASES)
    assert all(C.BY_ID[c].runs.get("window") == "window" and C.BY_ID[c].runs.get("window-ring") == "window-ring"
               for c in C.EQUALITY_CASES)
    assert all(C.BY_ID[c].runs.get("lds") == "lds" for c in C.FACTOR_CASES)


@CASES
def test_pattern_is_symmetric_with_full_diagonal(case):
    P = C.pattern(*case.pattern)
    assert P.shape == (case.n, case.n) and case.n != C.NFP
    assert (abs(P - P.T)).nnz == 0
    assert np.all(P.diagonal() == 1.0)


@CASES
def test_expected_kinds_follow_from_choose_sweep(case):
    s = stats(case.id)
    for run, kind in case.runs.items():
        assert restated_kind(s, C.options(case, C.RUNS[run])) == kind, run
    if any(k in ("window", "window-ring", "levels+window-ring") for k in case.runs.values()):
        assert case.records == (records(s.eL), records(s.eU))
    else:
        assert case.records is None


def test_block_lengths_against_the_limits():
    blen = {c.id: stats(c.id).blen for c in C.CASES}
    for cid in ("far", "reach-16320", "reach-16321"):  # longer than LDS and the LDS window, within the ring variant
        assert C.LDS_ROWS < blen[cid] <= C.WINDOW_RING_ROWS and blen[cid] > C.WINDOW_ROWS
    for cid in set(blen) - {"far", "reach-16320", "reach-16321"}:
        assert blen[cid] <= C.WINDOW_ROWS
    assert [stats(c).reach for c in ("reach-16320", "reach-16321")] == [16320, 16321]
    assert C.WINDOW_RING_REACH == 16320 and stats("far").reach == 20900


def test_diag_one_level_wider_than_waves_and_ring_chunk():
    for cid, n in (("diag-4100", 4100), ("diag-4096", 4096)):
        s = stats(cid)
        assert s.lenL.max() == 0 and s.lenU.max() == 0 and s.levL == 1 and s.levU == 1 and s.widest == n
    assert stats("diag-4100").widest > C.RING_CHUNK >= stats("diag-4096").widest
    assert stats("diag-4096").widest // 64 > 16  # more slices than the workgroup has waves


def test_chain_one_row_per_level_and_a_partial_last_window():
    s = stats("chain")
    assert s.n == 15 * 64 + 40 and s.levL == s.n and s.levU == s.n and s.widest == 1
    assert np.array_equal(np.nonzero(s.offL)[0], np.arange(64, s.n, 64)) and s.eL == 1
    assert np.array_equal(np.nonzero(s.offU)[0], np.arange(63, s.n - 1, 64)) and s.eU == 1


def test_twolevel_two_levels_wider_than_1024():
    s = stats("twolevel")
    assert [list(w) for w in s.widthL] == [[1300, 1300]]
    (wu,) = s.widthU  # (first-half rows that no row of the second half reaches stay in U's first level)
    assert len(wu) == 2 and wu.min() > 1024
    assert set(s.lenL[1300:]) == set(range(1, 13)) and s.lenL[:1300].max() == 0


def test_lanes_row_lengths():
    s = stats("lanes")
    inL, inU = C.lanes_rows()
    assert [s.lenL[inL[c]] for c in C.LANE_COUNTS] == list(C.LANE_COUNTS)
    assert [s.lenU[inU[c]] for c in C.LANE_COUNTS] == list(C.LANE_COUNTS)
    assert not set(inL.values()) & set(inU.values())
    assert s.lenL.max() == 225 and s.lenU.max() == 225 and s.widest == 1
    # 1 / 2 / 4 lanes x 7 (lds), 16 x 7 (gmem, chain: 113 refuses), 32 x 7 (ring: 225 is over)
    for lanes in (1, 2, 4, 16, 32):
        assert lanes * C.LANE_ENTRIES in C.LANE_COUNTS and lanes * C.LANE_ENTRIES + 1 in C.LANE_COUNTS
    assert chain_steps(s, s.lenL, s.widthL) == -1


@pytest.mark.parametrize("cid,max_l,max_u", [("win_records-4/8", 16, 32), ("win_records-6/4", 24, 16),
                                             ("win_records-8/6", 32, 24), ("win33", 16, 33)])
def test_window_records_off_window_counts(cid, max_l, max_u):
    s = stats(cid)
    inL, inU = C.win_rows()
    assert (s.eL, s.eU) == (max_l, max_u)
    for c in C.WINDOW_COUNTS:
        assert s.offL[inL[c]] == (c if c <= max_l else 0)
        assert s.offU[inU[c]] == (c if c <= min(max_u, 32) else 0)
    others = np.setdiff1d(np.arange(s.n), list(inL.values()) + list(inU.values()) + [C.WIN33_ROW])
    assert s.offL[others].max() <= 6 and s.offU[others].max() <= 6
    if cid == "win33":
        assert s.offU[C.WIN33_ROW] == 33 and (s.offU > 32).sum() == 1
    else:
        assert C.BY_ID[cid].records == (records(max_l), records(max_u))
        assert s.n % 64 != 0


def test_arrow_one_long_row_and_one_gathered_column():
    s = stats("arrow")
    assert s.lenL[-1] == 400 and s.lenL[:-1].max() == 1
    P = C.pattern(*C.BY_ID["arrow"].pattern)
    assert (P[:-1, -1].toarray().ravel() != 0).sum() == 400 and s.lenU.max() == 2
    assert s.eL > C.WINDOW_ENTRIES


def test_blocks_truncation_and_tiny_blocks():
    sizes = {c: np.diff(C.block_starts(C.BY_ID[c])) for c in ("blocks-3", "blocks-70", "blocks-100")}
    assert sorted(set(sizes["blocks-70"])) == [64, 65] and sizes["blocks-70"][0] == 65  # windows of 1 row
    assert sorted(set(sizes["blocks-100"])) == [1, 2]
    assert list(sizes["blocks-3"]) == [334, 333, 333]
    for cid in sizes:
        case = C.BY_ID[cid]
        P = C.pattern(*case.pattern)
        assert C.truncated(case, P).nnz < P.nnz  # cross-block entries exist
        assert stats(cid).reach < sizes[cid].max()


def test_far_rows_have_near_and_far_ring_entries():
    """The ring sweep on `far`: rows with the entries i - 17,000 and i - 20,900 (L) hold them as far
    dependencies (position below row_lo) beside the near i - 1 and i - 70; the rows they point to see
    the same in U."""
    case = C.BY_ID["far"]
    s = stats("far")
    T = C.pattern(*case.pattern)
    r, c = C.coords(T)
    assert s.widest <= C.RING_CHUNK and s.n > C.LDS_ROWS
    for upper in (False, True):
        posof, row_lo = ring_rows(s, upper)
        side = (c > r) if upper else (c < r)
        is_far = side & (posof[c] < row_lo[r])
        is_near = side & ~is_far
        nfar, nnear = np.bincount(r[is_far], minlength=s.n), np.bincount(r[is_near], minlength=s.n)
        both = np.nonzero((nfar > 0) & (nnear > 0))[0]
        print(f"far {'U' if upper else 'L'}: {is_far.sum()} far entries in {(nfar > 0).sum()} rows, "
              f"{both.size} rows with near entries too, most far entries in a row {nfar.max()}")
        assert both.size >= 40 and nfar.max() >= (1 if upper else 2)
        assert np.all(np.abs(r - c)[is_far] >= 17000)
    # swin: far terms are those before the super-window (at most 8 windows of 64 rows)
    assert s.reach > 8 * 64


@CASES
@pytest.mark.parametrize("kind", ["int", "unit"])
def test_exact_data_is_exact(case, kind):
    d = C.data(case, kind)
    aL, aU = C.int_factors(case, kind)
    prod = (aL @ aU)
    grow = prod @ np.abs(d.y)
    print(f"{case.id} {kind}: max |L||U| {prod.data.max():.0f}, max |L||U||y*| {grow.max():.0f}, max |K| "
          f"{np.abs(d.K.data).max():.1f}, explicit zeros in K {(d.K.data == 0).sum()}, max |x| {np.abs(d.x).max():.1f}")
    assert prod.data.max() < 2.0 ** 40 and grow.max() < 2.0 ** 40
    assert d.K.nnz == C.pattern(*case.pattern).nnz  # explicit zeros stay stored
    T = C.truncated(case, d.K)
    ilu = native.ILU0(T)
    assert np.array_equal(ilu.lu, d.factors)
    assert np.array_equal(ilu.solve(d.x[:case.n]), d.y)


@CASES
def test_unit_data_survives_the_window_inverses(case):
    """The inverse kinds' exact data: the windowed solve in float64 (explicit inverses of the 64-row window
    triangles) is finite and within 1e-12 max |y*| -- the bar the device is held to -- on "unit"."""
    d = C.data(case, "unit")
    T = C.truncated(case, d.K)
    y = C.windowed_solve(T, native.ILU0(T).lu, C.block_starts(case), d.x[:case.n])
    ratio = float(np.abs(y - d.y).max()) / float(np.abs(d.y).max())
    print(f"{case.id}: windowed restatement on unit data {ratio:.2e} of max |y*|, rows wrong {(y != d.y).sum()}")
    assert np.all(np.isfinite(y)) and ratio <= 1e-12


def test_int_data_does_not_survive_deep_window_inverses():
    """Why the inverse kinds do not run "int": a chain's window inverse grows like 6^k."""
    case = C.BY_ID["chain"]
    d = C.data(case, "int")
    T = C.truncated(case, d.K)
    with np.errstate(all="ignore"):
        y = C.windowed_solve(T, native.ILU0(T).lu, C.block_starts(case), d.x[:case.n])
    assert not np.array_equal(y, d.y)


@CASES
def test_normal_data_reference_conditions(case):
    d = C.data(case, "normal")
    T = C.truncated(case, d.K)
    ilu = native.ILU0(T)
    scale = float(np.abs(d.y).max())
    x = d.x[:case.n]
    e_oracle = float(np.abs(ilu.solve(x) - d.y).max()) / scale
    e_window = float(np.abs(C.windowed_solve(T, ilu.lu, C.block_starts(case), x) - d.y).max()) / scale
    print(f"{case.id}: oracle {e_oracle:.2e}, windowed restatement {e_window:.2e} of max |y|")
    assert e_oracle <= 1e-14
    assert e_window <= 1e-13


def test_lds_layout_cases_reach_every_lane_count_and_tails():
    """The cases whose LDS stream layout the device test compares (sweep_cases.LAYOUT_RUNS): 1, 2 and 4
    lanes per row chosen by the rows, slices with tails under every lane count, levels wider than the
    16 waves, and none of them prints what the 64-row identity fp block prints."""
    fp_block = (1, 1, 1, 0, 0, C.LANE_ENTRIES, 0)
    chosen = set()
    for name, run in C.LAYOUT_RUNS:
        case = C.BY_ID[name]
        assert case.runs[run] == "lds"
        force = int(C.RUNS[run].get("pls.sweep_lpr", 0))
        for upper in (False, True):
            nums, lprs = C.lds_layout(case, upper, force)
            assert nums != fp_block
            if name == "lanes":
                assert nums[6] > 0 and set(lprs) == {force or 4}
            if not force:
                chosen |= set(lprs)
    assert chosen == {1, 2, 4}
    assert C.lds_layout(C.BY_ID["twolevel"], True)[0][3] > 0 and C.lds_layout(C.BY_ID["diag-4100"], False)[0][2] == 65
