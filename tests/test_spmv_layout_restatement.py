"""The numpy restatement of the outer SpMV layouts (tests/spmv_layout_restatement.py) on the
patterns of tests/spmv_layout_cases.py: no device needed.

Per case: the restated plan reaches the branch the case is named for, and the streams decode to the
exact product on integer data (``decode_matvec(encode(A), x) == A @ x`` in int64 arithmetic).  The
device tests (tests/test_gpu_spmv_layouts.py) then pin libpls to the same plan through the bytes
of the layout.

The last tests replace one step of the restatement with a wrong version and require the product
to change: they show that the cases can tell these mistakes (the device kernels are not mutated).
"""
import numpy as np
import pytest

import spmv_layout_cases as C
import spmv_layout_restatement as R

_layouts = {}


def _layout(case):
    """(restated layout, A, x, perm) of a case on integer data, computed once and left unchanged."""
    if case.id not in _layouts:
        if len(_layouts) >= 2:
            _layouts.pop(next(iter(_layouts)))
        A, x = C.matrix(case, "int")
        perm = C.index_sets(case, A.shape[0])[3]
        _layouts[case.id] = (R.layout(C.internal(A, perm), case.options), A, x, perm)
    return _layouts[case.id]


def _product(L, x, perm):
    """The caller-order product from the restated streams (internal order inside)."""
    y = np.empty_like(x)
    y[perm] = R.decode_matvec(L.encode(), x[perm])
    return y


def _check_expectation(L, key, want):
    plan = L.plan
    if key == "d16":
        assert L.d16 == want
    elif key == "fallback":
        assert L.fallback == want
    elif key == "sorted":
        assert (plan.rowmap is not None) == want
    elif key == "multi":
        if want == "all":
            assert len(plan.slpr) > 0 and (plan.slpr > 1).all()
        else:
            assert L.multi_lane_slices == want
    elif key == "mixed_lanes":
        assert ((plan.slpr > 1).any() and (plan.slpr == 1).any()) == want
    elif key == "b3":
        assert (L.b3 is not None) == want
    elif key == "rcm":
        assert (L.rcm is not None) == want
        if want:
            assert sorted(L.rcm.tolist()) == list(range(L.n))
            assert L.bytes() - R.replace(L, rcm=None).bytes() == 20 * L.n  # the nperm term
    elif key == "max_bases":
        assert L.max_bases == want
    elif key == "nsegs":
        assert L.nsegs == want
    elif key == "wide_groups":
        assert plan.wide_groups == want
    elif key == "groups_of_8":
        assert tuple(np.diff(L.sptr) // 64 // 8) == want
    elif key == "singles":
        assert len(L.b3.singles) == want
    elif key == "d16_slices":
        assert L.nslices == want
    else:
        raise KeyError(key)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_case_reaches_its_branch(case):
    L = _layout(case)[0]
    for key, want in case.expect:
        _check_expectation(L, key, want)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_streams_decode_to_the_exact_product(case):
    L, A, x, perm = _layout(case)
    y = _product(L, x, perm)
    assert np.array_equal(y, C.exact_product(A, x).astype(np.float64))


def test_wide_pattern_has_the_checked_group_count():
    """8 of the 17 full groups of the n = 1100 pattern are wide, for every lane count."""
    assert C.wide_groups_expected(1100) == 8 and 1100 // 64 == 17
    assert 1111 % 64 != 0 and C.wide_groups_expected(1111) > 0


def test_wide_rows_lose_to_the_sorted_plan_unless_the_lane_share_fills_its_groups():
    """24-entry wide rows: ceil(24 / lanes) rounds up to 8, so every lane count above 1 pads by more
    than 15 % and the sorted plan replaces the wide slices; 512-entry rows keep them."""
    n = 1100
    r = np.arange(n)
    short = C._pattern(n, *C._runs(n, np.full(n, 24), (5 * r) % (n - 24)))
    for l in (2, 4, 8, 16, 32, 64):
        plan = R.layout(short, {"pls.d16_wide_lpr": str(l)}).plan
        assert plan.rowmap is not None and plan.wide_groups == 0
    assert R.layout(short, {"pls.d16_wide_lpr": "1"}).plan.rowmap is None


def test_alternating_long_and_short_rows_get_no_multi_lane_group():
    """Rows of 40 and 3 entries in turn: the sorted plan is taken, but with 2 lanes per row a group of
    40-entry rows stores 2 x 64 x roundup8(20) = 3072 entries against 64 x 40 = 2560 with one: the
    5 % rule rejects it."""
    n = 1024
    r = np.arange(n)
    lens = np.where(r % 2 == 0, 40, 3)
    L = R.layout(C._pattern(n, *C._runs(n, lens, np.minimum(r, n - lens))))
    assert L.plan.rowmap is not None and L.multi_lane_slices == 0


@pytest.mark.parametrize("name", C.XCD_CASES)
def test_xcd_cases_leave_surplus_blocks(name):
    """pls.d16_xcd 1 rounds the grid up to 8 blocks of 4 slices: these slice counts are no multiple of 32."""
    assert _layout(C.BY_ID[name])[0].nslices % 32 != 0


def test_sell_bytes_formula_on_a_hand_case():
    """n = 3, one entry: int32 SELL stores 64 entries (12 B) and 2 slice pointers, plus the empty B3 pointer."""
    L = R.layout(C.pattern("edges", 3), {"pls.sell_d16": "0"})
    assert (L.d16, L.bytes()) == (False, 64 * 12 + 2 * 8 + 8)
    L = R.layout(C.pattern("edges", 3))
    assert (L.d16, L.bytes()) == (True, 64 * 8 * 10 + (64 * 4 * 4 + 20) + 8 + 8)


# ------------------------------------------------------------------ mutations --
def _differs(case_id):
    """True when the (mutated) restatement no longer gives the exact product of the case."""
    case = C.BY_ID[case_id]
    A, x = C.matrix(case, "int")
    perm = C.index_sets(case, A.shape[0])[3]
    try:
        y = _product(R.layout(C.internal(A, perm), case.options), x, perm)
    except IndexError:  # a base or a column outside its array
        return True
    return not np.array_equal(y, C.exact_product(A, x).astype(np.float64))


def test_mutation_delta_threshold(monkeypatch):
    assert not _differs("delta-edge")
    monkeypatch.setattr(R, "DELTA_MAX", 65536)  # a gap of 65536 then wraps to a zero delta
    assert _differs("delta-edge")


def test_mutation_no_base_clamp(monkeypatch):
    assert not _differs("edges-65")
    monkeypatch.setattr(R, "_base_index", lambda si, nsegs: si)  # padding walks past the lane's bases
    assert _differs("edges-65")
    assert _differs("segments-4")


def test_mutation_swapped_combine_lanes(monkeypatch):
    def partner(lanes, o):
        p = lanes ^ o
        p[[0, 2]] = p[[2, 0]]  # lane 0 adds the sum lane 2 should add, and the other way round
        return p

    assert not _differs("sigma-lpr2")
    monkeypatch.setattr(R, "_combine_partner", partner)
    assert _differs("sigma-lpr2")
    assert _differs("wide-1100-lpr8")
    assert _differs("b3-all")


def test_mutation_row_map_inverse(monkeypatch):
    assert not _differs("sigma-lpr1")
    monkeypatch.setattr(R, "_output_rows", lambda rowmap, pos: pos if rowmap is None else np.argsort(rowmap)[pos])
    assert _differs("sigma-lpr1")
    assert _differs("dense-row")
