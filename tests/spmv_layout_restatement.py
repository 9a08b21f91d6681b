"""The SpMV layouts of the outer operator (csrc/runtime.cpp: build_sell, d16_plan, build_b3,
build_sell_rcm, d16_from_plan; csrc/kernels.hip: k_d16_*, k_b3_*, k_sell_*), restated in numpy.

``layout(A, options)`` follows build_sell for a square CSR matrix with sorted columns on one rank
and returns a ``Layout``: the slice plan (sfirst, slpr, rowmap), the most segment bases a lane
needs, the B3 split, the RCM order, and the value DevSELL::bytes() has for the chosen layout.
``Layout.encode()`` fills the streams the device arrays would hold, with the indexing k_d16_fill /
k_b3_fill / k_sell_fill document, and ``decode_matvec(streams, x)`` walks them as the product
kernels do: a zero delta takes the lane's next base, the base index clamps to the last base, a
row's lane sums combine in the kernels' xor order, results go to rowmap[position].

The planner's rules, as pinned here:

* plain plan: one slice of 64 rows per 64-row group, lane = row.  A full group is "wide" when the
  first columns of its rows r and r + 63 are more than 4 * 63 apart, neither row is empty and the
  group holds 16+ entries per row on average (integer division); it then becomes d16_wide_lpr
  slices of 64 / d16_wide_lpr rows with d16_wide_lpr lanes per row.
* a slice stores 64 * roundup8(max over its rows of ceil(len / lanes)) entries.
* SELL-C-sigma: when the plain plan stores more than (1 + d16_sigma_pad) * nnz (and d16_sigma > 0,
  n >= 64), rows are stably sorted by decreasing length inside windows of d16_sigma rows; a group
  of 64 positions takes d16_sorted_lpr lanes per row when its rows hold 32+ entries on average and
  that stores at most 1.05 x what one lane per row stores; the sorted plan is taken when it stores
  at most 0.85 x the plain plan's entries.  It replaces the plain plan as a whole, wide slices
  included: wide rows survive only where ceil(len / lanes) rounds to a multiple of 8 with little
  padding.
* segment bases: a lane starts a new base at its first entry, at a column gap above 65535 and at
  a non-increasing column; up to 4 bases give nsegs 4 (8 with d16_segs 8), up to 8 give nsegs 8,
  more give the int32 SELL-64 layout for the whole matrix.
* B3 (spmv_b3, n >= 192): greedy heads of row triples with one column list; used when the triples
  hold at least half the entries; heads stably sorted by decreasing length in windows of 512;
  the other rows go to a D16 part that always takes the sorted plan (no 5 % rule there).
* RCM (spmv_rcm, n >= 16384, no B3): -1 relabels where the plain matrix takes the sorted plan, 1
  always; the relabelled matrix is planned with spmv_rcm 0 and the product gathers x first.

The loops over entries are numpy calls; Python loops run over 64-row groups, triples, distinct
slice lengths and the vertices of the RCM sweep.
"""
from dataclasses import dataclass, replace

import numpy as np
import scipy.sparse as sp

D16_SEG, D16_SEG_MAX = 4, 8
DELTA_MAX = 65535        # largest column delta a 16-bit entry holds
B3_LPT, B3_WINDOW, B3_MIN_ROWS = 4, 512, 192
RCM_MIN_ROWS = 16384
LANES = np.arange(64)


@dataclass(frozen=True)
class Options:
    sell_d16: bool = True
    d16_wide_lpr: int = 8
    d16_sigma: int = 1024
    d16_sigma_pad: float = 0.15
    d16_sorted_lpr: int = 2
    d16_segs: int = D16_SEG
    spmv_b3: bool = False
    spmv_rcm: int = -1

    @classmethod
    def from_pls(cls, opts):
        """From a dict of ``pls.*`` option strings (other keys -- unroll, xcd -- do not change the layout)."""
        kw = {}
        for f, conv in (("sell_d16", lambda v: bool(int(v))), ("d16_wide_lpr", int), ("d16_sigma", int),
                        ("d16_sigma_pad", float), ("d16_sorted_lpr", int), ("d16_segs", int),
                        ("spmv_b3", lambda v: bool(int(v))), ("spmv_rcm", int)):
            if "pls." + f in opts:
                kw[f] = conv(opts["pls." + f])
        return cls(**kw)


@dataclass
class Plan:
    sfirst: np.ndarray            # first position of every slice, and the end (nslices + 1)
    slpr: np.ndarray              # lanes per row of every slice
    rowmap: np.ndarray = None     # position -> row (None: rows keep their order)
    wide_groups: int = 0          # 64-row groups the plain plan split into wide slices


@dataclass
class B3:
    heads: np.ndarray             # first row of every triple, in slice order (the device's b3map)
    singles: np.ndarray           # the rows left to the D16 part
    bptr: np.ndarray              # slice pointers into the column stream (64 * L entries per slice)


@dataclass
class Layout:
    n: int
    rp: np.ndarray                # the matrix the streams are filled from (RCM: the relabelled one)
    ci: np.ndarray
    val: np.ndarray
    d16: bool = False
    fallback: bool = False        # D16 asked for, but a lane needs more than 8 bases
    plan: Plan = None
    max_bases: int = 0
    nsegs: int = D16_SEG
    sptr: np.ndarray = None
    b3: B3 = None
    rcm: np.ndarray = None        # order[new] = old (the device's xperm); None: not relabelled
    rowmap_out: np.ndarray = None  # the row map the product writes through

    @property
    def nslices(self):
        return len(self.sptr) - 1

    @property
    def stored(self):
        return int(self.sptr[-1])

    @property
    def multi_lane_slices(self):
        return int((self.plan.slpr > 1).sum()) if self.d16 and self.plan is not None else 0

    def bytes(self):
        """DevSELL::bytes()."""
        b3_stored = int(self.b3.bptr[-1]) if self.b3 else 0
        b3_ntrip = len(self.b3.heads) if self.b3 else 0
        b3_nslices = len(self.b3.bptr) - 1 if self.b3 else 0
        nrows_mapped = 0 if self.rowmap_out is None else len(self.rowmap_out)
        nperm = 0 if self.rcm is None else self.n
        if self.d16:
            own = self.stored * 10 + self.nslices * (64 * 4 * self.nsegs + 20) + 8 + nrows_mapped * 4
        else:
            own = self.stored * 12 + (self.nslices + 1) * 8
        return own + b3_stored * 28 + b3_ntrip * 4 + (b3_nslices + 1) * 8 + nperm * 20

    def encode(self):
        return encode(self)


def _csr(A):
    A = sp.csr_matrix(A)
    if A.shape[0] != A.shape[1]:
        raise ValueError("square matrices only")
    if not A.has_sorted_indices:
        A = A.sorted_indices()
    return A.shape[0], A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float64)


def _up8(v):
    return (v + 7) & ~7


def _ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the plan --
def plan_stored(lens, plan):
    """Entries the D16 slices of a plan store (d16_plan_stored)."""
    if len(plan.slpr) == 0:
        return 0
    ls = lens if plan.rowmap is None else lens[plan.rowmap]
    if len(ls) == 0:
        return 0
    longest = np.maximum.reduceat(ls, plan.sfirst[:-1])
    return int((64 * _up8(_ceil_div(longest, plan.slpr))).sum())


def _sorted_windows(rows, lens, window):
    rm = np.array(rows, dtype=np.int64)
    for w in range(0, len(rm), window):
        part = rm[w:w + window]
        rm[w:w + window] = part[np.argsort(-lens[part], kind="stable")]
    return rm


def _group_stored(ls, p, e, l):
    st = 0
    for q in range(p, e, 64 // l):
        L = _ceil_div(int(ls[q:min(e, q + 64 // l)].max()), l)
        st += 64 * _up8(L)
    return st


def d16_plan(n, rp, ci, o, subset=None):
    """d16_plan: the slice plan of the rows (subset: of the rows the B3 layout leaves over)."""
    lens = np.diff(rp)
    if subset is not None:
        rm = _sorted_windows(subset, lens, max(o.d16_sigma, 64))
        m = len(rm)
        sf, sl = [], []
        for p in range(0, m, 64):
            e = min(m, p + 64)
            tot = int(lens[rm[p:e]].sum())
            l = o.d16_sorted_lpr if (o.d16_sorted_lpr > 1 and tot >= 32 * (e - p)) else 1
            for q in range(p, e, 64 // l):
                sf.append(q)
                sl.append(l)
        sf.append(m)
        return Plan(np.array(sf, dtype=np.int64), np.array(sl, dtype=np.int64), rm)
    c0 = np.full(n, -1, dtype=np.int64)  # first column of every row, -1: empty (k_first_col)
    c0[lens > 0] = ci[rp[:-1][lens > 0]]
    sf, sl, wide_groups = [], [], 0
    for r in range(0, n, 64):
        wide = False
        if r + 64 <= n and c0[r] >= 0 and c0[r + 63] >= 0:
            spread = int(c0[r + 63]) - int(c0[r])
            avg = int(rp[r + 64] - rp[r]) // 64
            wide = spread > 4 * 63 and avg >= 16
        if wide:
            l = o.d16_wide_lpr
            wide_groups += 1
            for q in range(l):
                sf.append(r + (64 // l) * q)
                sl.append(l)
        else:
            sf.append(r)
            sl.append(1)
    sf.append(n)
    plain = Plan(np.array(sf, dtype=np.int64), np.array(sl, dtype=np.int64), None, wide_groups)
    if o.d16_sigma <= 0 or n < 64:
        return plain
    nnz = int(rp[n])
    stored = plan_stored(lens, plain)
    if float(stored) <= (1.0 + o.d16_sigma_pad) * float(nnz):
        return plain
    rm = _sorted_windows(np.arange(n), lens, o.d16_sigma)
    ls = lens[rm]
    sf, sl = [], []
    for p in range(0, n, 64):
        e = min(n, p + 64)
        tot = int(ls[p:e].sum())
        l = 1
        if (o.d16_sorted_lpr > 1 and tot >= 32 * (e - p) and
                float(_group_stored(ls, p, e, o.d16_sorted_lpr)) <= 1.05 * float(_group_stored(ls, p, e, 1))):
            l = o.d16_sorted_lpr
        for q in range(p, e, 64 // l):
            sf.append(q)
            sl.append(l)
    sf.append(n)
    srt = Plan(np.array(sf, dtype=np.int64), np.array(sl, dtype=np.int64), rm)
    if float(plan_stored(lens, srt)) > 0.85 * float(stored):
        return plain
    return srt


# ------------------------------------------------------------- lane streams --
@dataclass
class _Streams:
    """Every entry of the planned rows, ordered by (row, lane of the row, place in the lane)."""
    idx: np.ndarray      # the entry's place in ci / val
    pos: np.ndarray      # the row's position in the plan
    sl: np.ndarray       # the slice of that position
    lane: np.ndarray     # the lane of the slice holding the entry
    k: np.ndarray        # the entry's place in the lane's stream
    col: np.ndarray
    newbase: np.ndarray  # the entry starts a segment (k_d16_count's rule)
    gap: np.ndarray      # column minus the previous column of the lane
    segi: np.ndarray     # bases the lane used before this entry's segment


def _lane_streams(n, rp, ci, plan):
    npos = int(plan.sfirst[-1])
    rows_of_pos = np.arange(npos) if plan.rowmap is None else plan.rowmap
    lens = np.diff(rp)[rows_of_pos]
    sl_of_pos = np.searchsorted(plan.sfirst, np.arange(npos), side="right") - 1
    pos = np.repeat(np.arange(npos), lens)
    j = np.arange(len(pos)) - np.repeat(np.cumsum(lens) - lens, lens)
    idx = rp[rows_of_pos][pos] + j
    sl = sl_of_pos[pos]
    l = plan.slpr[sl]
    sub, k = j % l, j // l
    order = np.lexsort((k, sub, pos))
    idx, pos, sl, sub, k, l = idx[order], pos[order], sl[order], sub[order], k[order], l[order]
    col = ci[idx]
    first = k == 0
    gap = np.zeros(len(col), dtype=np.int64)
    gap[1:] = col[1:] - col[:-1]
    newbase = first | (gap > DELTA_MAX) | (gap <= 0)
    cs = np.cumsum(newbase)
    start = np.maximum.accumulate(np.where(first, cs - 1, 0)) if len(cs) else cs
    lane = (pos - plan.sfirst[sl]) * l + sub
    return _Streams(idx, pos, sl, lane, k, col, newbase, gap, cs - 1 - start)


def max_bases(n, rp, ci, plan):
    """The most segment bases a lane of the plan needs (k_d16_count)."""
    s = _lane_streams(n, rp, ci, plan)
    return int(s.segi.max()) + 1 if len(s.segi) else 0


def _slice_ptr(lens, plan):
    if len(plan.slpr) == 0:
        return np.zeros(1, dtype=np.int64)
    ls = lens if plan.rowmap is None else lens[plan.rowmap]
    longest = np.maximum.reduceat(ls, plan.sfirst[:-1])
    return np.concatenate(([0], np.cumsum(64 * _up8(_ceil_div(longest, plan.slpr))))).astype(np.int64)


# ------------------------------------------------------------------- B3 ------
def triple_flags(n, rp, ci):
    """flag[r]: rows r, r + 1, r + 2 are not empty and have one column list (k_triple_flags)."""
    lens = np.diff(rp)
    f = np.zeros(n, dtype=bool)
    if n < 3:
        return f
    cand = np.zeros(n, dtype=bool)
    cand[:n - 2] = (lens[:n - 2] > 0) & (lens[1:n - 1] == lens[:n - 2]) & (lens[2:] == lens[:n - 2])
    rows = np.nonzero(cand)[0]
    cl = lens[rows]
    re = np.repeat(rows, cl)
    j = np.arange(len(re)) - np.repeat(np.cumsum(cl) - cl, cl)
    same = (ci[rp[re] + j] == ci[rp[re + 1] + j]) & (ci[rp[re] + j] == ci[rp[re + 2] + j])
    bad = np.zeros(n, dtype=bool)
    bad[re[~same]] = True
    return cand & ~bad


def b3_split(n, rp, ci, o):
    """build_b3: None when the B3 layout is not used."""
    if not o.spmv_b3 or n < B3_MIN_ROWS:
        return None
    lens = np.diff(rp)
    flagged = np.nonzero(triple_flags(n, rp, ci))[0]
    heads, r = [], 0
    while True:  # greedy: the first flagged row at or after r heads a triple, the sweep goes on 3 rows later
        t = np.searchsorted(flagged, r)
        if t == len(flagged):
            break
        heads.append(int(flagged[t]))
        r = heads[-1] + 3
    heads = np.array(heads, dtype=np.int64)
    in_triple = np.zeros(n, dtype=bool)
    for d in range(3):
        in_triple[heads + d] = True
    singles = np.nonzero(~in_triple)[0]
    if 2 * 3 * int(lens[heads].sum()) < int(rp[n]):
        return None
    heads = _sorted_windows(heads, lens, B3_WINDOW)
    per = 64 // B3_LPT
    nt = len(heads)
    ns = _ceil_div(nt, per)
    bptr = np.zeros(ns + 1, dtype=np.int64)
    for s in range(ns):
        L = _ceil_div(int(lens[heads[s * per:s * per + per]].max()), B3_LPT)
        bptr[s + 1] = bptr[s] + 64 * L
    return B3(heads, singles, bptr)


# ------------------------------------------------------------------ RCM ------
def rcm_order(n, rp, ci):
    """rcm_order: order[new] = old."""
    lev = np.full(n, -1, dtype=np.int64)
    done = np.zeros(n, dtype=bool)
    deg = np.diff(rp)
    order = []

    def bfs_last(s):
        q = [s]
        lev[s] = 0
        h = 0
        while h < len(q):
            u = q[h]
            nb = ci[rp[u]:rp[u + 1]]
            nb = nb[(lev[nb] < 0) & ~done[nb]]
            lev[nb] = lev[u] + 1
            q.extend(nb.tolist())
            h += 1
        lev[q] = -1
        return q[-1]

    s0 = 0
    while s0 < n:
        if done[s0]:
            s0 += 1
            continue
        s = bfs_last(bfs_last(s0))
        h = len(order)
        order.append(s)
        done[s] = True
        while h < len(order):
            u = order[h]
            nb = ci[rp[u]:rp[u + 1]]
            nb = nb[~done[nb]]
            done[nb] = True
            order.extend(nb[np.argsort(deg[nb], kind="stable")].tolist())
            h += 1
    return np.array(order[::-1], dtype=np.int64)


# --------------------------------------------------------------- build_sell --
def _sell_layout(n, rp, ci, val, fallback):
    lens = np.diff(rp)
    ns = (n + 63) // 64
    longest = np.maximum.reduceat(np.concatenate((lens, np.zeros(ns * 64 - n, dtype=np.int64))), np.arange(ns) * 64)
    sptr = np.concatenate(([0], np.cumsum(64 * longest))).astype(np.int64)
    return Layout(n, rp, ci, val, d16=False, fallback=fallback, sptr=sptr)


def _build(n, rp, ci, val, o):
    nnz = int(rp[n])
    if o.spmv_rcm != 0 and o.sell_d16 and not o.spmv_b3 and n >= RCM_MIN_ROWS:
        pads = o.spmv_rcm == 1
        if not pads:
            pads = d16_plan(n, rp, ci, o).rowmap is not None
        if pads:
            order = rcm_order(n, rp, ci)
            P = sp.csr_matrix((val, ci, rp), shape=(n, n))[order][:, order].tocsr()
            P.sort_indices()
            inner = _build(*_csr(P), replace(o, spmv_rcm=0))
            if inner.d16 and inner.b3 is None:
                inner.rcm = order
                inner.rowmap_out = order if inner.plan.rowmap is None else order[inner.plan.rowmap]
                return inner
    if o.sell_d16 and nnz > 0:
        b3 = b3_split(n, rp, ci, o)
        plan = d16_plan(n, rp, ci, o, subset=b3.singles if b3 else None)
        if len(plan.slpr) == 0:  # every row in a triple
            return Layout(n, rp, ci, val, d16=True, plan=plan, sptr=np.zeros(1, dtype=np.int64), b3=b3)
        h = max_bases(n, rp, ci, plan)
        if h <= D16_SEG_MAX:
            nsegs = D16_SEG if (h <= D16_SEG and o.d16_segs <= D16_SEG) else D16_SEG_MAX
            return Layout(n, rp, ci, val, d16=True, plan=plan, max_bases=h, nsegs=nsegs,
                          sptr=_slice_ptr(np.diff(rp), plan), b3=b3, rowmap_out=plan.rowmap)
        if b3:
            return _build(n, rp, ci, val, replace(o, spmv_b3=False))
        L = _sell_layout(n, rp, ci, val, fallback=True)
        L.max_bases = h
        return L
    return _sell_layout(n, rp, ci, val, fallback=False)


def layout(A, options=None):
    """The layout build_sell gives the square CSR matrix A; options: an Options or a dict of pls.* strings."""
    o = options if isinstance(options, Options) else Options.from_pls(options or {})
    return _build(*_csr(A), o)


# ------------------------------------------------------------------ streams --
@dataclass
class Streams:
    n: int
    kind: str                     # "d16" or "sell"
    sptr: np.ndarray
    val: np.ndarray
    col: np.ndarray = None        # sell
    dl: np.ndarray = None         # d16: uint16 deltas
    seg: np.ndarray = None        # d16: (slices * 64, nsegs) bases
    nsegs: int = D16_SEG
    sfirst: np.ndarray = None
    slpr: np.ndarray = None
    rowmap: np.ndarray = None
    xperm: np.ndarray = None
    b3ptr: np.ndarray = None
    b3map: np.ndarray = None
    b3col: np.ndarray = None
    b3val: np.ndarray = None


def _encode_d16(L):
    plan = L.plan
    ns = len(plan.slpr)
    stored = L.stored
    dl = np.zeros(max(stored, 8), dtype=np.uint16)
    dv = np.zeros(max(stored, 2), dtype=np.float64)
    seg = np.zeros((ns * 64, L.nsegs), dtype=np.int64)
    s = _lane_streams(L.n, L.rp, L.ci, plan)
    base = L.sptr[s.sl]
    # deltas dl[base + (k / 8) * 512 + lane * 8 + k % 8], values dv[base + (k / 2) * 128 + lane * 2 + k % 2]
    dl[base + (s.k >> 3) * 512 + s.lane * 8 + (s.k & 7)] = np.where(s.newbase, 0, s.gap).astype(np.uint16)
    dv[base + (s.k >> 1) * 128 + s.lane * 2 + (s.k & 1)] = L.val[s.idx]
    slot = s.sl * 64 + s.lane
    nb = s.newbase
    seg[slot[nb], s.segi[nb]] = s.col[nb]
    used = np.zeros(ns * 64, dtype=np.int64)
    np.maximum.at(used, slot[nb], s.segi[nb] + 1)
    for jj in range(1, L.nsegs):  # unused bases repeat the last one (a lane without entries: 0)
        seg[:, jj] = np.where(jj < used, seg[:, jj], seg[:, jj - 1])
    return dl, dv, seg


def _encode_b3(L):
    b3 = L.b3
    stored = int(b3.bptr[-1])
    bcol = np.zeros(max(stored, 1), dtype=np.int64)
    bval = np.zeros(max(3 * stored, 1), dtype=np.float64)
    per = 64 // B3_LPT
    for pos, h in enumerate(b3.heads):
        s, first_lane = pos // per, (pos % per) * B3_LPT
        base, Ls = int(b3.bptr[s]), int(b3.bptr[s + 1] - b3.bptr[s]) // 64
        s0, ln = int(L.rp[h]), int(L.rp[h + 1] - L.rp[h])
        # col[base + kk * 64 + lane], val[3 * base + (3 kk + row of the triple) * 64 + lane]; padding: the first column
        kk, sub = np.meshgrid(np.arange(Ls), np.arange(B3_LPT), indexing="ij")
        k = kk * B3_LPT + sub
        inside = k < ln
        lane = first_lane + sub
        bcol[base + kk * 64 + lane] = np.where(inside, L.ci[s0 + np.minimum(k, ln - 1)], L.ci[s0])
        for d in range(3):
            sd = int(L.rp[h + d])
            bval[3 * base + (3 * kk + d) * 64 + lane] = np.where(inside, L.val[sd + np.minimum(k, ln - 1)], 0.0)
    return bcol, bval


def _encode_sell(L):
    n, ns = L.n, L.nslices
    col = np.zeros(max(L.stored, 1), dtype=np.int64)
    val = np.zeros(max(L.stored, 2), dtype=np.float64)
    lens = np.diff(L.rp)
    # padding repeats the row's last column with value 0
    Ls = np.diff(L.sptr) // 64
    rows = np.arange(n)
    padc = np.where(lens > 0, L.ci[np.maximum(L.rp[1:] - 1, 0)] if len(L.ci) else 0, 0)
    rl = Ls[rows // 64]
    re = np.repeat(rows, rl)
    k = np.arange(len(re)) - np.repeat(np.cumsum(rl) - rl, rl)
    where = L.sptr[re // 64] + k * 64 + re % 64
    inside = k < lens[re]
    src = np.where(inside, L.rp[re] + k, 0)
    if len(L.ci):
        col[where] = np.where(inside, L.ci[src], padc[re])
        val[where] = np.where(inside, L.val[src], 0.0)
    return col, val


def encode(L):
    """The streams the device arrays of the layout hold."""
    if not L.d16:
        col, val = _encode_sell(L)
        return Streams(L.n, "sell", L.sptr, val, col=col)
    dl, dv, seg = _encode_d16(L)
    E = Streams(L.n, "d16", L.sptr, dv, dl=dl, seg=seg, nsegs=L.nsegs, sfirst=L.plan.sfirst, slpr=L.plan.slpr,
                rowmap=L.rowmap_out, xperm=L.rcm)
    if L.b3:
        E.b3ptr, E.b3map = L.b3.bptr, L.b3.heads
        E.b3col, E.b3val = _encode_b3(L)
    return E


# ----------------------------------------------------------------- products --
# The three steps below are functions of their own so that a test can replace one with a wrong
# version and see the product change (tests/test_spmv_layout_restatement.py).
def _base_index(si, nsegs):
    """The base a zero delta takes: the lane's next one, clamped to the last."""
    return np.minimum(si, nsegs - 1)


def _combine_partner(lanes, o):
    """The lane whose sum a lane adds in the combine step with offset o (__shfl_xor)."""
    return lanes ^ o


def _output_rows(rowmap, pos):
    """The row a position's result is written to."""
    return pos if rowmap is None else rowmap[pos]


def _columns_checked(col, n):
    if col.size and (col.min() < 0 or col.max() >= n):
        raise IndexError("the product would read x outside [0, n)")
    return col


def _decode_d16(E, x, y):
    L = np.diff(E.sptr) // 64
    for Lv in np.unique(L):
        S = np.nonzero(L == Lv)[0]
        base = E.sptr[S][:, None]
        slot = S[:, None] * 64 + LANES
        col = np.zeros((len(S), 64), dtype=np.int64)
        si = np.zeros((len(S), 64), dtype=np.int64)
        acc = np.zeros((len(S), 64), dtype=x.dtype)
        for k in range(int(Lv)):
            d = E.dl[base + (k >> 3) * 512 + LANES * 8 + (k & 7)].astype(np.int64)
            a = E.val[base + (k >> 1) * 128 + LANES * 2 + (k & 1)]
            zero = d == 0
            b = E.seg[slot, _base_index(si, E.nsegs)]
            col = np.where(zero, b, col + d)
            si = si + zero
            acc = acc + a * x[_columns_checked(col, E.n)]
        lpr = E.slpr[S][:, None]
        o = 1
        while o < 64:  # for (o = 1; o < lpr; o <<= 1) acc += __shfl_xor(acc, o)
            acc = np.where(o < lpr, acc + acc[:, _combine_partner(LANES, o)], acc)
            o <<= 1
        pos = E.sfirst[S][:, None] + LANES // lpr
        writes = (LANES % lpr == 0) & (pos < E.sfirst[S + 1][:, None])
        y[_output_rows(E.rowmap, pos[writes])] = acc[writes]


def _decode_b3(E, x, y):
    per = 64 // B3_LPT
    nt = len(E.b3map)
    for s in range(len(E.b3ptr) - 1):
        base, Ls = int(E.b3ptr[s]), int(E.b3ptr[s + 1] - E.b3ptr[s]) // 64
        acc = np.zeros((3, 64), dtype=x.dtype)
        for k in range(Ls):
            xv = x[_columns_checked(E.b3col[base + k * 64 + LANES], E.n)]
            for d in range(3):
                acc[d] = acc[d] + E.b3val[3 * base + (3 * k + d) * 64 + LANES] * xv
        for o in (1, 2):  # DPP quad_perm xor 1, xor 2
            acc = acc + acc[:, _combine_partner(LANES, o)]
        pos = s * per + LANES // B3_LPT
        for d in range(3):
            w = (pos < nt) & (LANES % B3_LPT == d)
            y[E.b3map[pos[w]] + d] = acc[d][w]


def _decode_sell(E, x, y):
    n = E.n
    L = np.diff(E.sptr) // 64
    for Lv in np.unique(L):
        S = np.nonzero(L == Lv)[0]
        acc = np.zeros((len(S), 64), dtype=x.dtype)
        for k in range(int(Lv)):
            where = E.sptr[S][:, None] + k * 64 + LANES
            acc = acc + E.val[where] * x[_columns_checked(E.col[where], n)]
        rows = S[:, None] * 64 + LANES
        y[rows[rows < n]] = acc[rows < n]


def decode_matvec(E, x):
    """y = A x from the streams alone, the way the product kernels walk them.  Rows no slice
    writes stay NaN.  The sums run in x's floating-point type."""
    x = np.asarray(x)
    y = np.full(E.n, np.nan, dtype=x.dtype)
    if E.kind == "sell":
        _decode_sell(E, x, y)
        return y
    if E.xperm is not None:
        x = x[E.xperm]
    if E.b3map is not None:
        _decode_b3(E, x, y)
    _decode_d16(E, x, y)
    return y
