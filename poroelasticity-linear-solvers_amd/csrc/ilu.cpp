// ilu.cpp -- PCILU: ILU(0) of a matrix's block-Jacobi truncation (ilu, bjacobi; ILU(k) where levels of
// fill are asked for: fill_levels swaps the pattern before the factorization), the exact LU on its
// envelope pattern (lu) and the classical AMG's hybrid Gauss-Seidel chunks (sgs).  The constructor
// factors (factor), picks one of ten sweep kernels (choose_sweep) and builds that kernel's device
// tables from the factors (build_tables); apply() launches it.
#include "runtime.hpp"
#include "amg_host.hpp"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace pls {

// One triangle's rows in level order: level (group) g is rows [grp[g], grp[g + 1])
// of `order`; per block (off[b] = first group of block b) or global (off empty).
struct TriLevels {
    bool upper = false;
    std::vector<int32_t> order;
    std::vector<int64_t> grp, off;
    int64_t count() const { return (int64_t)grp.size() - 1; }
    int64_t widest() const {
        int64_t w = 0;
        for (int64_t g = 0; g < count(); ++g) w = std::max(w, grp[g + 1] - grp[g]);
        return w;
    }
};
// Ring sweep: per row its block-local level-order position, the first position still in the ring, its near entries
struct RingRows {
    std::vector<int32_t> posof, row_lo, near_len;
};
struct PCILU::Setup {
    int64_t n = 0;
    std::vector<int64_t> rp, dg, bst;  // F's row pointers and diagonal positions; block starts
    std::vector<int32_t> ci;
    TriLevels levL;  // global levels of L (the factorization's draw order)
    // what choose_sweep yields on the way: levels per block, where a block kernel can sweep (else global
    // levels); for the window kinds the rows' most off-window entries per triangle
    TriLevels L, U;
    int eL = 32, eU = 32;
};

// host vector -> device buffer (at least one entry), enqueued on c.st
template <class T>
static void upload_vec(DBuf<T> &d, const std::vector<T> &v, Ctx &c) {
    d.alloc(std::max<size_t>(v.size(), 1));
    if (!v.empty()) HIPCHK(hipMemcpyAsync(d.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, c.st));
}

// every row's level in the strict lower (upper) dependency graph
static std::vector<int32_t> row_levels(const PCILU::Setup &s, bool upper) {
    const int64_t n = s.n;
    const auto &rp = s.rp;
    const auto &ci = s.ci;
    std::vector<int32_t> lvl(n, 0);
    if (!upper) {
        for (int64_t i = 0; i < n; ++i) {
            int32_t L = 0;
            for (int64_t k = rp[i]; k < rp[i + 1] && ci[k] < i; ++k) L = std::max(L, lvl[ci[k]] + 1);
            lvl[i] = L;
        }
    } else {
        for (int64_t i = n - 1; i >= 0; --i) {
            int32_t L = 0;
            for (int64_t k = rp[i + 1] - 1; k >= rp[i] && ci[k] > i; --k) L = std::max(L, lvl[ci[k]] + 1);
            lvl[i] = L;
        }
    }
    return lvl;
}

// Block-major level groups: rows sorted by (block, level); grp[g] = first row
// of group g, off[b] = first group of block b (counting sort).
static TriLevels block_level_groups(const PCILU::Setup &s, const std::vector<int64_t> &bst, bool upper) {
    const int64_t n = s.n, nb = (int64_t)bst.size() - 1;
    const std::vector<int32_t> lvl = row_levels(s, upper);
    TriLevels t{upper};
    auto &order = t.order;
    auto &grp = t.grp, &off = t.off;
    order.reserve(n);
    off.assign(nb + 1, 0);
    int64_t b0 = 0;
    std::vector<int64_t> cnt;
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t len = bst[b + 1] - bst[b];
        int32_t nl = 0;
        for (int64_t i = b0; i < b0 + len; ++i) nl = std::max(nl, lvl[i] + 1);
        cnt.assign(nl + 1, 0);
        for (int64_t i = b0; i < b0 + len; ++i) cnt[lvl[i] + 1]++;
        for (int32_t l = 0; l < nl; ++l) cnt[l + 1] += cnt[l];
        off[b] = (int64_t)grp.size();
        const int64_t base = (int64_t)order.size();
        for (int32_t l = 0; l < nl; ++l) grp.push_back(base + cnt[l]);
        order.resize(base + len);
        std::vector<int64_t> pos(cnt.begin(), cnt.end() - 1);
        for (int64_t i = b0; i < b0 + len; ++i) order[base + pos[lvl[i]]++] = (int32_t)i;
        b0 += len;
    }
    off[nb] = (int64_t)grp.size();
    grp.push_back(n);
    return t;
}

// global levels: one block, no block table
static TriLevels level_order(const PCILU::Setup &s, bool upper) {
    TriLevels t = block_level_groups(s, {0, s.n}, upper);
    t.off.clear();
    return t;
}

// Build a level-aligned SELL-64 factor from the factored F: rows in `order`,
// groups = t's levels (blockwise where t has them per block) -- padded to
// whole slices per group.
static void build_tri_sell(const PCILU &P, const PCILU::Setup &s, const TriLevels &t, TriSELL &T, Ctx &c) {
    const auto &rp = s.rp, &dg = s.dg, &grp = t.grp;
    const auto &order = t.order;
    const bool upper = t.upper;
    const int64_t ng = t.count();
    std::vector<int32_t> srow, slen;
    std::vector<int64_t> sl_len;  // 64 * L per slice
    T.gslice_h.assign(ng + 1, 0);
    for (int64_t g = 0; g < ng; ++g) {
        T.gslice_h[g] = (int64_t)sl_len.size();
        for (int64_t r = grp[g]; r < grp[g + 1]; r += 64) {
            int32_t L = 0;
            for (int l = 0; l < 64; ++l) {
                const int64_t rr = r + l;
                if (rr < grp[g + 1]) {
                    const int64_t i = order[rr];
                    const int32_t len = (int32_t)(upper ? rp[i + 1] - dg[i] - 1 : dg[i] - rp[i]);
                    srow.push_back((int32_t)i);
                    slen.push_back(len);
                    L = std::max(L, len);
                } else {
                    srow.push_back(-1);
                    slen.push_back(0);
                }
            }
            sl_len.push_back(64 * (int64_t)L);
        }
    }
    T.gslice_h[ng] = (int64_t)sl_len.size();
    T.ngroups = ng;
    T.nslices = (int64_t)sl_len.size();
    std::vector<int64_t> sptr(T.nslices + 1, 0);
    for (int64_t s = 0; s < T.nslices; ++s) sptr[s + 1] = sptr[s] + sl_len[s];
    upload_vec(T.sptr, sptr, c);
    upload_vec(T.gslice, T.gslice_h, c);
    upload_vec(T.slot_row, srow, c);
    upload_vec(T.slot_len, slen, c);
    T.blockwise = !t.off.empty();
    if (T.blockwise) {
        upload_vec(T.goff, t.off, c);
        T.nblocks = (int64_t)t.off.size() - 1;
    }
    T.col.alloc(std::max<int64_t>(sptr.back(), 1));
    T.val.alloc(std::max<int64_t>(sptr.back(), 1));
    if (upper) T.sdinv.alloc(std::max<int64_t>(T.nslices * 64, 1));
    launch_tri_fill(T.nslices, T.slot_row.p, T.slot_len.p, P.F.rp.p, P.F.ci.p, P.F.val.p, P.diag.p, P.dinv.p,
                    upper ? 1 : 0, T.sptr.p, T.col.p, T.val.p, upper ? T.sdinv.p : nullptr, c.st);
    HIPCHK(hipGetLastError());
    c.sync();
}

// LDS-kernel stream layout (sweep_lds.hip, "LDS sweep stream layout"): per block
// the lanes per row (1, 2 or 4) that fit every lane's share of the block's
// longest row into the kernel's register window; slices of 64 / LPR rows of
// one level; one header entry per lane.  Returns the most lanes per row of any block.
static int build_lds_tri(const PCILU &P, const PCILU::Setup &s, const TriLevels &t, int force_lpr, int max_lpr,
                         LdsTri &D, Ctx &c, std::vector<int64_t> *blk_maxsl, const RingRows *ring = nullptr) {
    const auto &rp = s.rp, &dg = s.dg, &grp = t.grp, &goff = t.off;
    const auto &order = t.order;
    const bool upper = t.upper;
    const int64_t n = s.n, nb = P.nblocks, ng = t.count(), nblk = nb;
    const int W = ilu_lds_lane_entries();
    auto rlen = [&](int64_t i) -> int64_t {
        if (ring) return ring->near_len[i];  // ring sweep: the near entries only
        return upper ? rp[i + 1] - dg[i] - 1 : dg[i] - rp[i];
    };
    std::vector<int32_t> lpr(nblk, 1), s_start, s_n, s_lpr;
    std::vector<int64_t> gsl(ng + 1, 0), sptr(1, 0);
    for (int64_t b = 0; b < nblk; ++b) {
        // lanes per row: the fewest that fit the longest row's per-lane share
        // into the kernel's register window (measured at N=59: 2 or 4 lanes
        // on short rows cost more in extra slices and headers than they gain)
        int64_t mx = 0;
        for (int64_t r = grp[goff[b]]; r < grp[goff[b + 1]]; ++r) mx = std::max(mx, rlen(order[r]));
        // (the y-resident sweep, max_lpr 16: its y gathers miss LDS, so an
        // in-level reload of a long row's tail costs an HBM round trip per
        // level; up to 16 lanes keep every entry in the prefetched window)
        // (capping the lanes so the widest level fits one slice per wave was
        // measured slower: FE 3-D N=12 53 -> 44 it/s, N=20 unchanged)
        int l = 1;
        while (l < max_lpr && (mx + l - 1) / l > W) l *= 2;
        if (force_lpr) {
            // pls.sweep_lpr: the sweep kernels are instantiated for 1/2/4 lanes per
            // row (LDS) and 1/2/4/8/16 (y-resident); anything else would run slices
            // under the wrong template and silently corrupt the apply
            if (force_lpr < 1 || force_lpr > max_lpr || (force_lpr & (force_lpr - 1)))
                throw Error("pls.sweep_lpr " + std::to_string(force_lpr) + " not supported by this sweep (allowed: 1.." +
                            std::to_string(max_lpr) + ", powers of two)");
            l = force_lpr;
        }
        lpr[b] = l;
        const int64_t per = 64 / l;
        if (ring) {
            // ring sweep: lanes per row chosen per slice (rows sorted longest first
            // inside each level): the fewest that keep every lane's share within the
            // register window, so short-row slices hold more rows and a level needs
            // fewer slices than the workgroup has waves (no in-level reloads)
            for (int64_t g = goff[b]; g < goff[b + 1]; ++g) {
                gsl[g] = (int64_t)s_start.size();
                for (int64_t r0 = grp[g]; r0 < grp[g + 1];) {
                    const int WR = ilu_ring_lane_entries();
                    int ls = force_lpr ? force_lpr : 1;  // pls.sweep_lpr pins it
                    int64_t r1 = 0, mxs = 0;
                    for (;;) {
                        r1 = std::min(grp[g + 1], r0 + 64 / ls);
                        mxs = 0;
                        for (int64_t r = r0; r < r1; ++r) mxs = std::max(mxs, rlen(order[r]));
                        if ((mxs + ls - 1) / ls <= WR || ls >= 32 || force_lpr) break;
                        ls *= 2;
                    }
                    s_start.push_back((int32_t)r0);
                    s_n.push_back((int32_t)(r1 - r0));
                    s_lpr.push_back(ls);
                    // lane-major entries, a multiple of the slot (WR + 1) per lane (header included)
                    sptr.push_back(sptr.back() + 64 * ((((mxs + ls - 1) / ls + 1) + WR) / (WR + 1) * (WR + 1)));
                    lpr[b] = std::max(lpr[b], ls);
                    r0 = r1;
                }
            }
            continue;
        }
        for (int64_t g = goff[b]; g < goff[b + 1]; ++g) {
            gsl[g] = (int64_t)s_start.size();
            for (int64_t r0 = grp[g]; r0 < grp[g + 1]; r0 += per) {
                const int64_t r1 = std::min(grp[g + 1], r0 + per);
                int64_t L = 0;
                for (int64_t r = r0; r < r1; ++r) L = std::max(L, (rlen(order[r]) + l - 1) / l);
                s_start.push_back((int32_t)r0);
                s_n.push_back((int32_t)(r1 - r0));
                s_lpr.push_back(l);
                sptr.push_back(sptr.back() + 64 * (L + 1));
            }
        }
    }
    gsl[ng] = (int64_t)s_start.size();
    const int64_t ns = (int64_t)s_start.size();
    if (blk_maxsl) {  // per block: the most slices any level has (max over both triangles)
        blk_maxsl->resize(nblk, 0);
        for (int64_t b = 0; b < nblk; ++b)
            for (int64_t g = goff[b]; g < goff[b + 1]; ++g) (*blk_maxsl)[b] = std::max((*blk_maxsl)[b], gsl[g + 1] - gsl[g]);
    }
    if (c.ilu_view >= 2 && !ring) {
        // per block: levels, slices beyond the 16 waves (run inline with dependent
        // loads), slices whose lanes hold more than the W prefetched entries
        int64_t worst_inline = 0, worst_lev = 0, worst_long = 0, wmax = 0, b_inl = 0;
        for (int64_t b = 0; b < nblk; ++b) {
            int64_t inl = 0, lng = 0;
            for (int64_t g = goff[b]; g < goff[b + 1]; ++g) {
                const int64_t s = gsl[g + 1] - gsl[g];
                wmax = std::max(wmax, s);
                inl += std::max<int64_t>(0, s - 16);
                for (int64_t k = gsl[g]; k < gsl[g + 1]; ++k) lng += (sptr[k + 1] - sptr[k]) / 64 - 1 > W;
            }
            if (inl > worst_inline) { worst_inline = inl; b_inl = b; }
            worst_lev = std::max(worst_lev, goff[b + 1] - goff[b]);
            worst_long = std::max(worst_long, lng);
        }
        fprintf(stderr, "[pls ilu lds %s] blocks %lld: max levels %lld, max slices per level %lld, inline slices "
                "(beyond 16 waves) max %lld (block %lld), slices with > %d entries per lane max %lld\n",
                upper ? "U" : "L", (long long)nblk, (long long)worst_lev, (long long)wmax, (long long)worst_inline,
                (long long)b_inl, W, (long long)worst_long);
    }
    auto up = [&](auto &d, const auto &v) { upload_vec(d, v, c); };
    DBuf<int32_t> d_start, d_n, d_lpr, d_order;
    up(D.sptr, sptr);
    up(D.gslice, gsl);
    up(D.lpr, lpr);
    up(d_start, s_start);
    up(d_n, s_n);
    up(d_lpr, s_lpr);
    up(d_order, order);
    D.col.alloc(std::max<int64_t>(sptr.back(), 1));
    D.val.alloc(std::max<int64_t>(sptr.back(), 1));
    DBuf<int32_t> d_posof, d_lo;
    if (ring) up(d_posof, ring->posof);
    if (ring) up(d_lo, ring->row_lo);
    launch_lds_fill(ns, d_start.p, d_n.p, d_lpr.p, d_order.p, P.F.rp.p, P.F.ci.p, P.F.val.p, P.diag.p, P.dinv.p,
                    upper ? 1 : 0, n, nb, D.sptr.p, D.col.p, D.val.p, c.st, /*wide headers: y-resident sweep*/ max_lpr > 4,
                    ring ? d_posof.p : nullptr, ring ? d_lo.p : nullptr, P.bstart_h.empty() ? nullptr : P.bstart.p);
    HIPCHK(hipGetLastError());
    c.sync();
    if (ring) {  // ring sweep: slice starts carry log2(lanes per row) in bits 0-2
        for (int64_t k = 0; k < ns; ++k) {
            int l2 = 0;
            while ((1 << l2) < s_lpr[k]) ++l2;
            sptr[k] |= l2;
        }
        HIPCHK(hipMemcpyAsync(D.sptr.p, sptr.data(), sizeof(int64_t) * sptr.size(), hipMemcpyHostToDevice, c.st));
        c.sync();
    }
    return *std::max_element(lpr.begin(), lpr.end());
}

void TriSELL::apply(const double *b, double *y, Ctx &c) const {
    const double *dv = sdinv.p;
    if (blockwise) {
        launch_tri_blocks(nblocks, goff.p, gslice.p, sptr.p, slot_row.p, slot_len.p, col.p, val.p, dv, b, y, c.st);
        return;
    }
    for (int64_t g = 0; g < ngroups; ++g)
        launch_tri_group(gslice_h[g], gslice_h[g + 1], sptr.p, slot_row.p, slot_len.p, col.p, val.p, dv, b, y, c.st);
}

// Profile (envelope) pattern of M with M's values and explicit zeros.
static void envelope_csr(const DevCSR &M, DevCSR &E, Ctx &c) {
    const int64_t n = M.nrows;
    const HostCSR H = download(M, c);
    const auto &rp = H.rp;
    const auto &ci = H.ci;
    const auto &v = H.v;
    std::vector<int64_t> erp(n + 1, 0), lo(n), hi(n);
    int64_t hmax = -1;
    for (int64_t i = 0; i < n; ++i) {
        int64_t a = i, b = i;
        if (rp[i + 1] > rp[i]) {
            a = std::min<int64_t>(a, ci[rp[i]]);
            b = std::max<int64_t>(b, ci[rp[i + 1] - 1]);
        }
        hmax = std::max(hmax, b);
        lo[i] = a;
        hi[i] = std::max<int64_t>(hmax, i);
        erp[i + 1] = erp[i] + (hi[i] - lo[i] + 1);
        if (hi[i] - lo[i] + 1 > ilu0_max_row())
            throw Error("lu: profile row longer than " + std::to_string(ilu0_max_row()) +
                        " entries; use ilu/bjacobi");
    }
    if (erp[n] > 400000000LL) throw Error("lu: profile fill exceeds 4e8 entries; use ilu/bjacobi on the device");
    std::vector<int32_t> eci(erp[n]);
    std::vector<double> ev(erp[n], 0.0);
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t j = lo[i]; j <= hi[i]; ++j) eci[erp[i] + (j - lo[i])] = (int32_t)j;
        for (int64_t k = rp[i]; k < rp[i + 1]; ++k) ev[erp[i] + (ci[k] - lo[i])] = v[k];
    }
    upload_csr(E, n, n, erp.data(), eci.data(), ev.data(), c);
}

// Ring sweep tables of one triangle: block-local level-order positions of the
// rows (posof), and level-aligned chunks of at most ilu_ring_chunk() positions.
// A row's dependency at position q is "near" when q >= row_lo[row] = (end of
// the row's chunk) - ilu_ring_slots(): still in the ring while the row runs.
// Far ones go to a CSR over positions, applied when the row's chunk loads.
static RingRows ring_tables(const PCILU::Setup &s, const TriLevels &t, const std::vector<double> &fv, RingTri &T,
                            Ctx &c) {
    RingRows rows;
    auto &posof = rows.posof, &row_lo = rows.row_lo, &near_len = rows.near_len;
    const auto &rp = s.rp, &dg = s.dg, &bst = s.bst, &grp = t.grp, &goff = t.off;
    const auto &ci = s.ci, &order = t.order;
    const bool upper = t.upper;
    const int64_t n = s.n, nb = (int64_t)bst.size() - 1;
    const int64_t C = ilu_ring_chunk(), R = ilu_ring_slots();
    posof.assign(n, 0);
    row_lo.assign(n, 0);
    near_len.assign(n, 0);
    std::vector<int64_t> coff(nb + 1, 0), cg, cp;
    int64_t b0 = 0;
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t len = bst[b + 1] - bst[b];
        for (int64_t k = b0; k < b0 + len; ++k) posof[order[k]] = (int32_t)(k - b0);
        coff[b] = (int64_t)cg.size();
        for (int64_t g = goff[b]; g < goff[b + 1];) {
            const int64_t c0 = grp[g] - b0;
            int64_t e = g + 1;
            while (e < goff[b + 1] && grp[e + 1] - b0 - c0 <= C) ++e;
            cg.push_back(g);
            cp.push_back(c0);
            cp.push_back(grp[e] - b0);
            for (int64_t k = grp[g]; k < grp[e]; ++k) row_lo[order[k]] = (int32_t)(grp[e] - b0 - R);
            g = e;
        }
        b0 += len;
    }
    coff[nb] = (int64_t)cg.size();
    // far dependencies, by position (b0 + p), in the row's entry order
    std::vector<int64_t> frp(n + 1, 0);
    std::vector<int32_t> fcol;
    std::vector<double> fval;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t i = order[k];
        const int64_t s0 = upper ? dg[i] + 1 : rp[i], s1 = upper ? rp[i + 1] : dg[i];
        int64_t near = 0;
        for (int64_t e = s0; e < s1; ++e) {
            const int32_t pc = posof[ci[e]];
            if (pc >= row_lo[i]) {
                ++near;
            } else {
                fcol.push_back(pc);
                fval.push_back(fv[e]);
            }
        }
        near_len[i] = (int32_t)near;
        frp[k + 1] = (int64_t)fcol.size();
    }
    T.nfar = (int64_t)fcol.size();
    auto up = [&](auto &d, const auto &v) { upload_vec(d, v, c); };
    up(T.coff, coff);
    up(T.cg, cg);
    up(T.cp, cp);
    up(T.ord, order);
    up(T.frp, frp);
    up(T.fcol, fcol);
    up(T.fval, fval);
    c.sync();
    return rows;
}

// Largest number of off-window entries of a row (the kernel's limit: ilu_window_max_entries())
static void window_max_entries(const PCILU::Setup &s, int &eL, int &eU) {
    const auto &rp = s.rp, &bst = s.bst;
    const auto &ci = s.ci;
    int64_t kml = 0, kmu = 0;
    for (size_t b = 0; b + 1 < bst.size(); ++b)
        for (int64_t i = bst[b]; i < bst[b + 1]; ++i) {
            const int64_t w0 = bst[b] + (i - bst[b]) / 64 * 64, w1 = std::min<int64_t>(w0 + 64, bst[b + 1]);
            int64_t kl = 0, ku = 0;
            for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
                kl += ci[k] < w0;
                ku += ci[k] >= w1;
            }
            kml = std::max(kml, kl);
            kmu = std::max(kmu, ku);
        }
    eL = (int)kml;
    eU = (int)kmu;
}
// Farthest dependency of a row in rows (|i - c| over the off-diagonal entries;
// the ring variant's limit: ilu_window_ring_rows() - 64)
static int64_t window_max_reach(const PCILU::Setup &s) {
    int64_t r = 0;
    for (int64_t i = 0; i < s.n; ++i)
        for (int64_t k = s.rp[i]; k < s.rp[i + 1]; ++k) r = std::max<int64_t>(r, std::abs(i - (int64_t)s.ci[k]));
    return r;
}

// Windows of 64 consecutive rows from every block's first row: per block its
// first window, per window its first and end row (global) and its block.
struct Windows {
    std::vector<int64_t> first, row, end, blk;
    int64_t n = 0;
    explicit Windows(const std::vector<int64_t> &bst) : first(bst.size(), 0) {
        const int64_t nblk = (int64_t)bst.size() - 1;
        for (int64_t b = 0; b < nblk; ++b) first[b + 1] = first[b] + (bst[b + 1] - bst[b] + 63) / 64;
        n = first[nblk];
        row.resize(n);
        end.resize(n);
        blk.resize(n);
        for (int64_t b = 0; b < nblk; ++b)
            for (int64_t w = first[b]; w < first[b + 1]; ++w) {
                row[w] = bst[b] + (w - first[b]) * 64;
                end[w] = std::min<int64_t>(row[w] + 64, bst[b + 1]);
                blk[w] = b;
            }
    }
};

// X = T^-1 of the leading m x m of a window's triangle (64 x 64, row-major) --
// unit lower (I + L_ww) or upper with the diagonal (U_ww) -- by row-wise
// substitution in double precision
static void invert_window_triangle(const std::vector<double> &T, std::vector<double> &X, int64_t m, bool upper) {
    std::fill(X.begin(), X.end(), 0.0);
    if (!upper) {  // T unit lower: row i of X from rows j < i
        for (int64_t i = 0; i < m; ++i) {
            X[i * 64 + i] = 1.0;
            for (int64_t j = 0; j < i; ++j) {
                double s = 0.0;
                for (int64_t k = j; k < i; ++k) s += T[i * 64 + k] * X[k * 64 + j];
                X[i * 64 + j] = -s;
            }
        }
    } else {  // T upper with its diagonal: rows from the last
        for (int64_t i = m - 1; i >= 0; --i) {
            const double d = T[i * 64 + i];
            X[i * 64 + i] = 1.0 / d;
            for (int64_t j = i + 1; j < m; ++j) {
                double s = 0.0;
                for (int64_t k = i + 1; k <= j; ++k) s += T[i * 64 + k] * X[k * 64 + j];
                X[i * 64 + j] = -s / d;
            }
        }
    }
}

// Window-sweep tables of one triangle of the (block-truncated) factors F
// (values fv): per block, windows of 64 consecutive rows;
// per window the rows' entries outside the window on the solved side (SELL,
// [k][lane], block-local columns) and the inverse of the window's triangle,
// stored [k][lane].
static void build_window_tri(const PCILU::Setup &s, const std::vector<double> &fv, bool upper, WinTri &W, Ctx &c) {
    const auto &rp = s.rp, &dg = s.dg, &bst = s.bst;
    const auto &ci = s.ci;
    const Windows win(bst);
    const std::vector<int64_t> &wrow = win.row, &wend = win.end;
    const int64_t nw = win.n;
    auto off_range = [&](int64_t i, int64_t w, int64_t &k0, int64_t &k1) {  // entries of row i outside window w
        if (!upper) {
            k0 = rp[i];
            k1 = k0;
            while (k1 < dg[i] && ci[k1] < wrow[w]) ++k1;
        } else {
            k1 = rp[i + 1];
            k0 = k1;
            while (k0 > dg[i] + 1 && ci[k0 - 1] >= wend[w]) --k0;
        }
    };
    std::vector<int64_t> woff(nw + 1, 0);
    for (int64_t w = 0; w < nw; ++w) {
        int64_t K = 0;
        for (int64_t i = wrow[w]; i < wend[w]; ++i) {
            int64_t k0, k1;
            off_range(i, w, k0, k1);
            K = std::max(K, k1 - k0);
        }
        woff[w + 1] = woff[w] + K * 64;
    }
    // (the staging copies read a fixed number of entries past a window's start: padding at the end)
    std::vector<int32_t> rec(3 * (woff[nw] + ilu_window_stream_pad()), 0);
    std::vector<double> tinv((size_t)std::max<int64_t>(nw, 1) * 4096, 0.0);
    auto put = [&](int64_t e, int32_t col, double v) {
        std::memcpy(&rec[3 * e], &v, 8);
        rec[3 * e + 2] = col;
    };
    amgh::parallel_rows(nw, amgh::setup_threads(), [&](int, int64_t w0, int64_t w1) {
        std::vector<double> T(64 * 64), X(64 * 64);
        for (int64_t w = w0; w < w1; ++w) {
            const int64_t r0 = wrow[w], m = wend[w] - r0, base = bst[win.blk[w]];
            std::fill(T.begin(), T.end(), 0.0);
            for (int64_t i = r0; i < wend[w]; ++i) {
                const int lane = (int)(i - r0);
                int64_t k0, k1;
                off_range(i, w, k0, k1);
                for (int64_t k = k0; k < k1; ++k) put(woff[w] + (k - k0) * 64 + lane, (int32_t)(ci[k] - base), fv[k]);
                // the window's triangle, row-major T[i][j]
                if (!upper) {
                    T[lane * 64 + lane] = 1.0;
                    for (int64_t k = k1; k < dg[i]; ++k) T[lane * 64 + (ci[k] - r0)] = fv[k];
                } else {
                    for (int64_t k = dg[i]; k < k0; ++k) T[lane * 64 + (ci[k] - r0)] = fv[k];
                }
            }
            invert_window_triangle(T, X, m, upper);
            for (int64_t i = 0; i < 64; ++i)  // column pairs: lane i loads X[i][k], X[i][k + 1] at once
                for (int64_t k = 0; k < 64; ++k) tinv[(size_t)w * 4096 + (k >> 1) * 128 + i * 2 + (k & 1)] = X[i * 64 + k];
        }
    });
    W.nwin = nw;
    W.woff.alloc(nw + 1);
    W.rec.alloc(rec.size());
    W.tinv.alloc(tinv.size());
    HIPCHK(hipMemcpyAsync(W.woff.p, woff.data(), sizeof(int64_t) * (nw + 1), hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemcpyAsync(W.rec.p, rec.data(), sizeof(int32_t) * rec.size(), hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemcpyAsync(W.tinv.p, tinv.data(), sizeof(double) * tinv.size(), hipMemcpyHostToDevice, c.st));
    c.sync();
}

// Super-window sweep tables of one triangle (kernels.hip, k_ilu_blocks_swin)
// for blocks too long for LDS.  Rows are cut into windows of 64 (from the
// block's first row, as build_window_tri), consecutive windows into
// super-windows in processing order (ascending for L, descending for U) as
// long as their staged data -- the packed window inverses (2,080 doubles) and
// the near streams -- fit ilu_swin_lds_budget() (at most 8 windows).  A row's
// entries on the solved side split three ways: in its own window (into the
// window's triangle, inverted as build_window_tri does), near (in its super-
// window, another window: SELL [k][lane], column = row - the super-window's
// first row, read from LDS) and far (before the super-window: SELL, block-
// local row, read from the block solution in global memory).  Padding entries
// carry column 0 and value 0.
static void build_swin_tri(const PCILU::Setup &s, const std::vector<double> &fv, bool upper, SwinTri &W, Ctx &c) {
    const auto &rp = s.rp, &dg = s.dg, &bst = s.bst;
    const auto &ci = s.ci;
    const int64_t nblk = (int64_t)bst.size() - 1;
    const Windows win(bst);
    const std::vector<int64_t> &wfirst = win.first, &wrow = win.row, &wend = win.end, &wblk = win.blk;
    const int64_t nw = win.n;
    // solved-side entries of row i: [s0, s1) in column order
    auto side = [&](int64_t i, int64_t &s0, int64_t &s1) {
        if (!upper) {
            s0 = rp[i];
            s1 = dg[i];
        } else {
            s0 = dg[i] + 1;
            s1 = rp[i + 1];
        }
    };
    // counts of row i's near / far entries for a super-window spanning rows [lo, hi) (global)
    auto counts = [&](int64_t i, int64_t w, int64_t lo, int64_t hi, int64_t &nn, int64_t &nf) {
        int64_t s0, s1;
        side(i, s0, s1);
        nn = nf = 0;
        for (int64_t k = s0; k < s1; ++k) {
            const int64_t cc = ci[k];
            if (cc >= wrow[w] && cc < wend[w]) continue;  // own window: the triangle
            if (cc >= lo && cc < hi) ++nn;
            else ++nf;
        }
    };
    auto win_near = [&](int64_t w, int64_t lo, int64_t hi) {  // the window's near entries per lane (max over rows)
        int64_t K = 0;
        for (int64_t i = wrow[w]; i < wend[w]; ++i) {
            int64_t nn, nf;
            counts(i, w, lo, hi, nn, nf);
            K = std::max(K, nn);
        }
        return K;
    };
    const int64_t budget = ilu_swin_lds_budget(), TRI = 2080;
    // super-windows, per block in processing order (greedy)
    std::vector<int64_t> bsw(nblk + 1, 0), sw;  // sw: 4 per super-window
    std::vector<int64_t> swof(nw, 0);           // window -> super-window
    int64_t max_stage = 0;
    for (int64_t b = 0; b < nblk; ++b) {
        const int64_t W0 = wfirst[b], W1 = wfirst[b + 1];
        int64_t k = 0;
        const int64_t nwb = W1 - W0;
        while (k < nwb) {
            const int64_t first = upper ? W1 - 1 - k : W0 + k;
            int64_t cnt = 0, bytes = 0;
            for (;;) {
                if (k + cnt >= nwb || cnt == 8) break;
                const int64_t w = upper ? W1 - 1 - (k + cnt) : W0 + k + cnt;
                // the super-window's rows if w joins: [lo, hi)
                const int64_t lo = upper ? wrow[w] : wrow[first], hi = upper ? wend[first] : wend[w];
                const int64_t add = TRI * 8 + win_near(w, lo, hi) * 64 * 12;
                if (cnt > 0 && bytes + add > budget) break;
                bytes += add;
                ++cnt;
            }
            const int64_t last = upper ? W1 - 1 - (k + cnt - 1) : W0 + k + cnt - 1;
            const int64_t wlo = std::min(first, last);
            sw.push_back(wlo);  // first window (ascending storage)
            sw.push_back(cnt);
            sw.push_back(wrow[wlo] - bst[b]);
            sw.push_back(wend[std::max(first, last)] - bst[b]);
            for (int64_t w = wlo; w < wlo + cnt; ++w) swof[w] = (int64_t)sw.size() / 4 - 1;
            max_stage = std::max(max_stage, bytes);
            k += cnt;
        }
        bsw[b + 1] = (int64_t)sw.size() / 4;
    }
    const int64_t nsw = (int64_t)sw.size() / 4;
    // per-window stream sizes
    std::vector<int64_t> wnear(nw + 1, 0), wfar(nw + 1, 0);
    {
        std::vector<int64_t> kn(nw), kf(nw);
        amgh::parallel_rows(nw, amgh::setup_threads(), [&](int, int64_t w0, int64_t w1) {
            for (int64_t w = w0; w < w1; ++w) {
                const int64_t s = swof[w], b = wblk[w];
                const int64_t lo = bst[b] + sw[4 * s + 2], hi = bst[b] + sw[4 * s + 3];
                int64_t a = 0, f = 0;
                for (int64_t i = wrow[w]; i < wend[w]; ++i) {
                    int64_t nn, nf;
                    counts(i, w, lo, hi, nn, nf);
                    a = std::max(a, nn);
                    f = std::max(f, nf);
                }
                kn[w] = a;
                kf[w] = f;
            }
        });
        for (int64_t w = 0; w < nw; ++w) {
            wnear[w + 1] = wnear[w] + kn[w] * 64;
            wfar[w + 1] = wfar[w] + kf[w] * 64;
        }
    }
    std::vector<int32_t> ncol(std::max<int64_t>(wnear[nw], 1), 0), fcol(std::max<int64_t>(wfar[nw], 1), 0);
    std::vector<double> nval(ncol.size(), 0.0), fval(fcol.size(), 0.0), tinv((size_t)std::max<int64_t>(nw, 1) * TRI, 0.0);
    amgh::parallel_rows(nw, amgh::setup_threads(), [&](int, int64_t w0, int64_t w1) {
        std::vector<double> T(64 * 64), X(64 * 64);
        for (int64_t w = w0; w < w1; ++w) {
            const int64_t s = swof[w], b = wblk[w], base = bst[b];
            const int64_t lo = base + sw[4 * s + 2], hi = base + sw[4 * s + 3];
            const int64_t r0 = wrow[w], m = wend[w] - r0;
            std::fill(T.begin(), T.end(), 0.0);
            for (int64_t i = r0; i < wend[w]; ++i) {
                const int lane = (int)(i - r0);
                int64_t s0, s1, qn = 0, qf = 0;
                side(i, s0, s1);
                if (!upper) T[lane * 64 + lane] = 1.0;
                for (int64_t k = s0; k < s1; ++k) {
                    const int64_t cc = ci[k];
                    if (cc >= r0 && cc < wend[w]) {
                        T[lane * 64 + (cc - r0)] = fv[k];
                    } else if (cc >= lo && cc < hi) {
                        ncol[wnear[w] + qn * 64 + lane] = (int32_t)(cc - lo);
                        nval[wnear[w] + qn * 64 + lane] = fv[k];
                        ++qn;
                    } else {
                        fcol[wfar[w] + qf * 64 + lane] = (int32_t)(cc - base);
                        fval[wfar[w] + qf * 64 + lane] = fv[k];
                        ++qf;
                    }
                }
                if (upper) T[lane * 64 + lane] = fv[dg[i]];
            }
            invert_window_triangle(T, X, m, upper);
            // packed by column k: L -- rows k..63 at 64k - k(k-1)/2 + (row - k); U -- rows 0..k at k(k+1)/2 + row
            double *t = &tinv[(size_t)w * TRI];
            for (int64_t k = 0; k < 64; ++k) {
                if (!upper)
                    for (int64_t i = k; i < 64; ++i) t[64 * k - k * (k - 1) / 2 + (i - k)] = X[i * 64 + k];
                else
                    for (int64_t i = 0; i <= k; ++i) t[k * (k + 1) / 2 + i] = X[i * 64 + k];
            }
        }
    });
    auto up = [&](auto &d, const auto &v) { upload_vec(d, v, c); };
    up(W.bsw, bsw);
    up(W.sw, sw);
    up(W.wnear, wnear);
    up(W.wfar, wfar);
    up(W.ncol, ncol);
    up(W.nval, nval);
    up(W.fcol, fcol);
    up(W.fval, fval);
    up(W.tinv, tinv);
    c.sync();
    W.nwin = nw;
    W.nsw = nsw;
    W.lds_bytes = 576 * 8 + max_stage;  // (the kernel's rows + broadcast slots, then the staged data)
}

// Chain-sweep stream of one triangle (kernels.hip, "chain sweep"): per block
// the fewest lanes per row (1..ilu_chain_max_lpr(), powers of two) that keep
// every lane's share of the block's longest row within 7 entries -- the LDS
// sweep's rule, so blocks whose rows fit 4 lanes get the LDS sweep's lanes and
// sums -- then per level steps of 16 / lpr rows in the level's row order, and
// slices of up to 4 consecutive steps (step q on lanes 16q .. 16q + 15).
// Returns the step count, or -1 when a row does not fit (D and ctx null, fv /
// dinv empty: a dry run that only counts).
static int64_t build_chain_tri(const PCILU::Setup &s, const TriLevels &t, const std::vector<double> &fv,
                               const std::vector<double> &dinv, ChainTri *D, Ctx *ctx) {
    const auto &rp = s.rp, &dg = s.dg, &bst = s.bst, &grp = t.grp, &goff = t.off;
    const auto &ci = s.ci, &order = t.order;
    const bool upper = t.upper;
    const int64_t nblk = (int64_t)bst.size() - 1;
    const int W = ilu_lds_lane_entries(), LMAX = ilu_chain_max_lpr();
    const int32_t PAD = (1 << 18) - 1;  // devutil.hpp SW_ROW_PAD
    auto rlen = [&](int64_t i) -> int64_t { return upper ? rp[i + 1] - dg[i] - 1 : dg[i] - rp[i]; };
    const bool dry = D == nullptr;
    std::vector<int64_t> base(nblk, 0), nsl(nblk, 0), soff(nblk, 0);
    std::vector<int32_t> szs, lpr(nblk, 1), col;
    std::vector<double> val;
    int64_t total = 0;
    for (int64_t b = 0; b < nblk; ++b) {
        const int64_t b0 = bst[b];
        int64_t mx = 0;
        for (int64_t r = grp[goff[b]]; r < grp[goff[b + 1]]; ++r) mx = std::max(mx, rlen(order[r]));
        int l = 1;
        while (l < LMAX && (mx + l - 1) / l > W) l *= 2;
        if ((mx + l - 1) / l > W) return -1;
        lpr[b] = l;
        const int64_t per = 16 / l;
        // steps: [first row, end row) in `order` positions, a level's rows cut every `per`
        std::vector<std::pair<int64_t, int64_t>> steps;
        for (int64_t g = goff[b]; g < goff[b + 1]; ++g)
            for (int64_t r0 = grp[g]; r0 < grp[g + 1]; r0 += per) steps.push_back({r0, std::min(grp[g + 1], r0 + per)});
        total += (int64_t)steps.size();
        if (dry) continue;
        std::vector<int32_t> sizes;
        base[b] = (int64_t)col.size();
        for (size_t s0 = 0; s0 < steps.size(); s0 += 4) {
            const size_t ns = std::min<size_t>(4, steps.size() - s0);
            // 8 entries per lane (header + 7; the lanes per row keep every share <= 7),
            // unused ones (column 0, value 0): the kernel sums all 7 without masking
            const int L = 8;
            const int64_t nl = 16 * (int64_t)ns, sz = nl * L;
            sizes.push_back((int32_t)(sz | (L == 8 ? 1 : 0)));
            const int64_t at = (int64_t)col.size();
            col.resize(at + sz, 0);
            val.resize(at + sz, 0.0);
            for (int64_t lane = 0; lane < nl; ++lane) col[at + lane * L] = PAD;  // lanes without a row
            for (size_t q = 0; q < ns; ++q) {
                for (int64_t r = steps[s0 + q].first; r < steps[s0 + q].second; ++r) {
                    const int64_t rr = r - steps[s0 + q].first;
                    const int64_t i = order[r];
                    const int64_t src = upper ? dg[i] + 1 : rp[i], len = rlen(i);
                    for (int sub = 0; sub < l; ++sub) {
                        const int64_t mine = len > sub ? (len - sub + l - 1) / l : 0;
                        const int64_t e = at + (16 * (int64_t)q + rr * l + sub) * L;
                        col[e] = (int32_t)(i - b0) | (int32_t)(mine << 18);
                        val[e] = upper ? dinv[i] : 0.0;
                        for (int64_t k = 1; k <= mine; ++k) {
                            const int64_t j = (k - 1) * l + sub;
                            col[e + k] = ci[src + j] - (int32_t)b0;
                            val[e + k] = fv[src + j];
                        }
                    }
                }
            }
        }
        nsl[b] = (int64_t)sizes.size();
        soff[b] = (int64_t)szs.size();
        szs.insert(szs.end(), sizes.begin(), sizes.end());
    }
    if (dry) return total;
    Ctx &c = *ctx;
    auto up = [&](auto &d, const auto &v) { upload_vec(d, v, c); };
    up(D->base, base);
    up(D->nsl, nsl);
    up(D->soff, soff);
    up(D->sz, szs);
    up(D->lpr, lpr);
    up(D->col, col);
    up(D->val, val);
    c.sync();
    return total;
}

PCILU::Config PCILU::Config::from_options(const Options &o, const std::string &prefix, unsigned reads) {
    Config cfg;
    cfg.allow_lds = o.flag("pls.ilu_lds", true);
    cfg.gmem_mode = (int)o.integer("pls.ilu_gmem", 0);
    cfg.ring_mode = (int)o.integer("pls.ilu_ring", 1);
    if (reads & LprProfile) {
        cfg.force_lpr = (int)o.integer("pls.sweep_lpr", 0);
        if (o.flag("pls.sweep_profile", false)) cfg.profile_tag = prefix;
    }
    if ((reads & Tuning) && o.has("pls.sweep_tpb")) cfg.tpb_override = (int)o.integer("pls.sweep_tpb", 1024);
    if (reads & Depth) {
        // (<prefix>pls_sweep_depth for one PC; 2, 3 and 4 are bitwise the same sweep)
        const std::string k = o.has(prefix + "pls_sweep_depth") ? prefix + "pls_sweep_depth" : "pls.sweep_depth";
        cfg.lds_depth = (int)o.integer(k, 2);
        if (cfg.lds_depth < 2 || cfg.lds_depth > 4) throw Error(k + " must be 2, 3 or 4");
    }
    if (reads & Tuning) cfg.rr = o.flag("pls.sweep_rr", false);
    if (reads & (Levels | SubLevels)) {
        const std::string k = prefix + ((reads & SubLevels) ? "sub_pc_factor_levels" : "pc_factor_levels");
        const std::string v = o.str(k, "");
        if (!v.empty()) {
            size_t used = 0;
            long long lv = -1;
            try { lv = std::stoll(v, &used); } catch (...) { used = 0; }
            if (used != v.size() || lv < 0 || lv > INT_MAX)
                throw Error("option " + k + ": levels of fill must be a non-negative integer, got '" + v + "'");
            cfg.levels = (int)lv;
            cfg.levels_key = k;
        }
        cfg.iluk_lds_slots = (int)o.integer("pls.iluk_lds_slots", 0);
        const int sl = cfg.iluk_lds_slots;
        if (sl != 0 && (sl < 256 || sl > 8192 || (sl & (sl - 1))))
            throw Error("pls.iluk_lds_slots " + std::to_string(sl) + ": a power of two from 256 to 8192 (0: automatic)");
    }
    return cfg;
}

// F <- the ILU(k) pattern of F (iluk.hip: two searches per row, count / scan / fill / sort), F's
// values in their places and zeros in the new ones.  F is the truncated block, so bjacobi's
// blocks fill separately.
void PCILU::fill_levels(Ctx &c, const Config &cfg) {
    const int64_t n = F.nrows;
    const std::string who = "ILU(" + std::to_string(cfg.levels) + ") symbolic (" + cfg.levels_key + ")";
    if (n == 0) return;
    DBuf<int32_t> fail(1);
    HIPCHK(hipMemsetAsync(fail.p, 0, sizeof(int32_t), c.st));
    auto failed = [&] {
        int32_t h = 0;
        HIPCHK(hipMemcpyAsync(&h, fail.p, sizeof(int32_t), hipMemcpyDeviceToHost, c.st));
        c.sync();
        return h;
    };
    {  // every row needs its diagonal entry: the filled pattern would otherwise invent it
        DBuf<int64_t> dpos(n);
        launch_find_diag(n, F.rp.p, F.ci.p, dpos.p, fail.p, c.st);
        if (failed()) throw Error("ILU(0): missing diagonal entry (PETSc: MAT_FACTOR_STRUCT_ZEROPIVOT)");
    }
    // G(A^T): the block's transposed pattern (unsorted adjacency lists)
    DBuf<int64_t> tcnt(n + 1), trp(n + 1);
    DBuf<int32_t> tci(std::max<int64_t>(F.nnz, 1)), cursor(n);
    HIPCHK(hipMemsetAsync(tcnt.p, 0, sizeof(int64_t) * (n + 1), c.st));
    HIPCHK(hipMemsetAsync(cursor.p, 0, sizeof(int32_t) * n, c.st));
    launch_iluk_transpose_count(n, F.rp.p, F.ci.p, tcnt.p, c.st);
    c.ensure_scan(n);
    exclusive_scan_i64(tcnt.p, trp.p, n, c.scan_tmp.p, c.scan_tmp_bytes, c.st);
    launch_iluk_transpose_fill(n, F.rp.p, F.ci.p, trp.p, cursor.p, tci.p, c.st);
    HIPCHK(hipGetLastError());
    // LDS table of a search: 16 k r slots for rows of at most r entries (half of them usable), 1.8
    // to 48 KB per wave.  Measured on the 2-D N = 6 blocks (r = 23 / 42): 8 r slots held every
    // level-1 search but sent 522 of 676 and 64 of 774 level-2 searches to the global-memory
    // launch, which clears a 131,072-slot table per search; the visited set (vertices < i
    // included) grows faster with the level than the filled row does
    int slot_bits = 8;
    if (cfg.iluk_lds_slots) {
        while ((1 << slot_bits) < cfg.iluk_lds_slots) ++slot_bits;
    } else {
        while (slot_bits < 13 && (1 << slot_bits) < 16 * (int64_t)cfg.levels * F.max_row) ++slot_bits;
    }
    const int gbits = 17;  // global-memory tables: 65,536 visited vertices per search
    DBuf<int32_t> lcnt(n), ucnt(n), ovfA(n), ovfT(n), ovfn(2);
    HIPCHK(hipMemsetAsync(lcnt.p, 0, sizeof(int32_t) * n, c.st));
    HIPCHK(hipMemsetAsync(ovfn.p, 0, sizeof(int32_t) * 2, c.st));
    IlukSearch sa{};
    sa.n = n, sa.rp = F.rp.p, sa.ci = F.ci.p, sa.levels = cfg.levels, sa.slot_bits = slot_bits, sa.transposed = 0;
    sa.lcnt = lcnt.p, sa.ucnt = ucnt.p, sa.ovf_rows = ovfA.p, sa.ovf_n = ovfn.p, sa.fail = fail.p;
    IlukSearch st = sa;
    st.rp = trp.p, st.ci = tci.p, st.transposed = 1, st.ovf_rows = ovfT.p, st.ovf_n = ovfn.p + 1;
    int32_t nov[2] = {0, 0};
    DBuf<int> gtab;
    int ggrid = 0;
    auto pass = [&](bool fill) {
        launch_iluk_search(sa, fill, c.st);
        launch_iluk_search(st, fill, c.st);
        HIPCHK(hipGetLastError());
        if (!fill) {
            HIPCHK(hipMemcpyAsync(nov, ovfn.p, sizeof(nov), hipMemcpyDeviceToHost, c.st));
            c.sync();
            if (nov[0] + nov[1] > 0) {
                ggrid = (int)std::min<int64_t>(std::max(nov[0], nov[1]), 256);
                gtab.alloc((size_t)ggrid * iluk_search_table_ints(1 << gbits));
            }
        }
        IlukSearch ga = sa, gt = st;
        ga.slot_bits = gt.slot_bits = gbits;
        launch_iluk_search_gmem(ga, fill, nov[0], std::min<int>(ggrid, std::max(nov[0], 1)), gtab.p, c.st);
        launch_iluk_search_gmem(gt, fill, nov[1], std::min<int>(ggrid, std::max(nov[1], 1)), gtab.p, c.st);
        HIPCHK(hipGetLastError());
        if (failed())
            throw Error(who + ": a row's search visits more than " + std::to_string(1 << (gbits - 1)) +
                        " vertices; lower the levels of fill");
    };
    pass(false);
    iluk_gmem_rows = (int64_t)nov[0] + nov[1];
    // row lengths -> row pointers; the refusals
    DevCSR G;
    DBuf<int64_t> len(n + 1);
    G.rp.alloc(n + 1);
    launch_iluk_row_len(n, lcnt.p, ucnt.p, len.p, c.st);
    exclusive_scan_i64(len.p, G.rp.p, n, c.scan_tmp.p, c.scan_tmp_bytes, c.st);
    std::vector<int64_t> hrp(n + 1);
    HIPCHK(hipMemcpyAsync(hrp.data(), G.rp.p, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, c.st));
    c.sync();
    int64_t mr = 0;
    for (int64_t i = 0; i < n; ++i) mr = std::max(mr, hrp[i + 1] - hrp[i]);
    if (mr > ilu0_max_row())
        throw Error(who + ": a filled row has " + std::to_string(mr) + " entries, the factorization stages at most " +
                    std::to_string(ilu0_max_row()) + " per row; lower " + cfg.levels_key);
    const int64_t fnnz = hrp[n];
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    // (columns and values now, the sweep tables -- about as much again -- later)
    if (fnnz < 0 || fnnz > INT64_MAX / 64 || (double)fnnz * 12.0 > 0.9 * (double)free_b)
        throw Error(who + ": the filled pattern has " + std::to_string(fnnz) + " entries (" +
                    std::to_string(fnnz * 12 >> 20) + " MiB), " + std::to_string(free_b >> 20) +
                    " MiB of device memory are free; lower " + cfg.levels_key);
    G.ci.alloc(std::max<int64_t>(fnnz, 1));
    G.val.alloc(std::max<int64_t>(fnnz, 1));
    HIPCHK(hipMemsetAsync(G.val.p, 0, sizeof(double) * std::max<int64_t>(fnnz, 1), c.st));
    HIPCHK(hipMemsetAsync(cursor.p, 0, sizeof(int32_t) * n, c.st));
    sa.orp = st.orp = G.rp.p;
    sa.oci = st.oci = G.ci.p;
    sa.cursor = st.cursor = cursor.p;
    pass(true);
    launch_iluk_sort_rows(n, G.rp.p, G.ci.p, mr, fail.p, c.st);
    launch_iluk_scatter(n, F.rp.p, F.ci.p, F.val.p, G.rp.p, G.ci.p, G.val.p, fail.p, c.st);
    HIPCHK(hipGetLastError());
    if (const int32_t h = failed())
        throw Error(who + ": inconsistent filled pattern (code " + std::to_string(h) + ")");
    F.rp = std::move(G.rp);
    F.ci = std::move(G.ci);
    F.val = std::move(G.val);
    F.nnz = fnnz;
    F.max_row = mr;
}

PCILU::PCILU(const DevCSR &M, int64_t nb, Ctx &c, const Config &cfg) {
    const bool trace = std::getenv("PLS_ILU_TRACE") != nullptr && M.nrows > 100000;
    auto tm0 = std::chrono::steady_clock::now();
    auto mark = [&](const char *what) {
        if (!trace) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[pcilu n %lld] %s %.3f s\n", (long long)M.nrows, what,
                std::chrono::duration<double>(t - tm0).count());
        tm0 = t;
    };
    Setup s;
    factor(M, nb, c, cfg, s);
    mark("factor");
    sweep = choose_sweep(s, c, cfg);
    mark("sweep choice");
    build_tables(s, c, cfg);
    mark("sweep tables");
    if (cfg.tpb_override >= 0) lds_tpb = cfg.tpb_override;
    lds_depth = cfg.lds_depth;
    lds_rr = cfg.rr && block_sweep_not_ring();
    profile_tag = cfg.profile_tag;
    const bool windows = sweep == Sweep::Window || sweep == Sweep::WindowRing || sweep == Sweep::LevelsWindowRing;
    if (c.ilu_view) {
        // levels of fill: appended where the option is set (the recorded ILU(0) lines stay as they are)
        char fill[96] = "";
        if (levels > 0)
            snprintf(fill, sizeof(fill), " levels %d fill %.3f (rows through global memory %lld)", levels,
                     nnz_block ? (double)F.nnz / (double)nnz_block : 1.0, (long long)iluk_gmem_rows);
        fprintf(stderr, "[pls ilu] type %s n %lld blocks %lld max_len %lld levels %lld/%lld sweep %s%s%s\n", type.c_str(),
                (long long)n, (long long)nblocks, (long long)max_len, (long long)nlev_L, (long long)nlev_U,
                sweep_kind(),
                windows ? (" (records " + std::to_string(window_records(window_entries_L)) + "/" +
                           std::to_string(window_records(window_entries_U)) + ")").c_str()
                        : "",
                fill);
    }
}

// Extract the block-Jacobi truncation (or the envelope) of M, find its
// diagonal, order the rows by level and factor in place: ILU(0), or the
// symmetric Gauss-Seidel factors.
void PCILU::factor(const DevCSR &M, int64_t nb, Ctx &c, const Config &cfg, Setup &s) {
    exact = cfg.exact_lu;
    sgs = cfg.sgs && !exact;
    type = exact ? "lu" : sgs ? "sgs" : (nb > 1 ? "bjacobi" : "ilu");
    n = s.n = M.nrows;
    nblocks = exact ? 1 : std::max<int64_t>(1, std::min<int64_t>(nb, n));
    if (cfg.bounds && !exact) {  // explicit block starts (nb + 1, from 0 to n, nondecreasing)
        if (cfg.bounds->size() < 2 || cfg.bounds->front() != 0 || cfg.bounds->back() != n)
            throw Error("PCILU: block bounds must run from 0 to n");
        for (size_t k = 0; k + 1 < cfg.bounds->size(); ++k)
            if ((*cfg.bounds)[k + 1] <= (*cfg.bounds)[k]) throw Error("PCILU: empty or decreasing block");
        bstart_h = *cfg.bounds;
        nblocks = (int64_t)bstart_h.size() - 1;
        upload_vec(bstart, bstart_h, c);
    }
    const bool bounds = !bstart_h.empty();
    s.bst = bstart_h;
    max_len = n / nblocks + 1;
    for (int64_t b = 0; bounds && b < nblocks; ++b) max_len = std::max(max_len, s.bst[b + 1] - s.bst[b]);
    if (!bounds) {  // PETSc's bjacobi sizes
        s.bst.assign(nblocks + 1, 0);
        for (int64_t b = 0; b < nblocks; ++b) s.bst[b + 1] = s.bst[b] + n / nblocks + (b < n % nblocks ? 1 : 0);
    }
    WindowSpec w{};
    if (nblocks > 1) {
        w.mode = 1;
        w.nblocks = nblocks;
        w.bstart = bounds ? bstart.p : nullptr;
    } else {
        w.mode = 0;
        w.c0 = 0;
        w.c1 = M.halo ? n : M.ncols;  // distributed: drop ghost columns (rank block only)
    }
    if (exact) envelope_csr(M, F, c);
    else extract_csr(M, 0, n, w, 0, n, F, c);
    nnz_block = F.nnz;
    levels = (!exact && !sgs) ? cfg.levels : 0;
    if (levels > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        fill_levels(c, cfg);
        if (std::getenv("PLS_ILU_TRACE"))  // (fill_levels ends synchronised)
            fprintf(stderr, "[pcilu n %lld] symbolic ILU(%d) + values %.3f s, fill %.3f, rows through global memory %lld\n",
                    (long long)n, levels, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(),
                    nnz_block ? (double)F.nnz / (double)nnz_block : 1.0, (long long)iluk_gmem_rows);
    }
    if (F.max_row > ilu0_max_row()) throw Error("ILU(0): row too long for the LDS-staged factorization");
    diag.alloc(std::max<int64_t>(n, 1));
    dinv.alloc(std::max<int64_t>(n, 1));
    DBuf<int32_t> fail(1);
    HIPCHK(hipMemsetAsync(fail.p, 0, sizeof(int32_t), c.st));
    launch_find_diag(n, F.rp.p, F.ci.p, diag.p, fail.p, c.st);
    auto &rp = s.rp, &dg = s.dg;
    auto &ci = s.ci;
    rp.resize(n + 1), dg.resize(n), ci.resize(F.nnz);
    HIPCHK(hipMemcpyAsync(rp.data(), F.rp.p, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, c.st));
    if (F.nnz) HIPCHK(hipMemcpyAsync(ci.data(), F.ci.p, sizeof(int32_t) * F.nnz, hipMemcpyDeviceToHost, c.st));
    int32_t hfail = 0;
    HIPCHK(hipMemcpyAsync(&hfail, fail.p, sizeof(int32_t), hipMemcpyDeviceToHost, c.st));
    c.sync();
    if (hfail) throw Error("ILU(0): missing diagonal entry (PETSc: MAT_FACTOR_STRUCT_ZEROPIVOT)");
    HIPCHK(hipMemcpyAsync(dg.data(), diag.p, sizeof(int64_t) * n, hipMemcpyDeviceToHost, c.st));
    c.sync();
    // numeric factorization, level by level (global levels of the forward sweep)
    s.levL = level_order(s, false);
    const std::vector<int32_t> &ordL = s.levL.order;
    const std::vector<int64_t> &Lptr = s.levL.grp;
    nlev_L = s.levL.count();
    if (sgs) {
        launch_sgs_factor(n, F.rp.p, F.ci.p, F.val.p, diag.p, dinv.p, fail.p, c.st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&hfail, fail.p, sizeof(int32_t), hipMemcpyDeviceToHost, c.st));
        c.sync();
    } else {
        // LDS sizing: the most staged entries one row needs
        std::vector<int64_t> ms(16, 0);
        amgh::parallel_rows(n, (int)std::min<int64_t>(16, n / 65536), [&](int w, int64_t i0, int64_t i1) {
            for (int64_t i = i0; i < i1; ++i) {
                int64_t tot = 0;
                for (int64_t k = rp[i]; k < dg[i]; ++k) tot += rp[ci[k] + 1] - dg[ci[k]] - 1;
                ms[w] = std::max(ms[w], tot);
            }
        });
        const int64_t max_staged = *std::max_element(ms.begin(), ms.end());
        DBuf<int32_t> rowsL(std::max<int64_t>(n, 1));
        HIPCHK(hipMemcpyAsync(rowsL.p, ordL.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, c.st));
        // one launch where levels are narrow (FE blocks: ~30 rows per level); wide levels
        // (BJACOBI on the headline: thousands of rows per level) keep a launch per level,
        // which there costs less than the per-row flags (setup 1.42 vs 1.73 s at N = 59)
        const bool dep = c.ilu_factor_dep == 1 ? nlev_L > 1 && n / nlev_L <= 2048 : c.ilu_factor_dep == 2;
        if (dep) {  // one launch; rows wait on their pivot rows' flags
            // the launch is deadlock-free only if the draw order is a topological
            // order of the pivot DAG (every pivot row r < i with l_ir != 0 drawn
            // before row i): the lowest unfinished drawn row then always has its
            // pivots done.  level_order gives one by construction; checked here
            // (O(nnz)) so that a wrong order is an error, not a bounded wait
            std::vector<int32_t> pos(n);
            for (int64_t q = 0; q < n; ++q) pos[ordL[q]] = (int32_t)q;
            for (int64_t i = 0; i < n; ++i)
                for (int64_t k = rp[i]; k < dg[i]; ++k)
                    if (pos[ci[k]] >= pos[i])
                        throw Error("ILU(0): factorization draw order is not topological (row " +
                                    std::to_string(i) + " before its pivot row " + std::to_string(ci[k]) + ")");
            DBuf<int32_t> done(std::max<int64_t>(n, 1)), ctr(2);
            launch_ilu0_dep(n, rowsL.p, F.rp.p, F.ci.p, F.val.p, diag.p, dinv.p, fail.p, F.max_row, max_staged,
                            c.ilu0_stage_cap, c.ilu_dep_grid, done.p, ctr.p, c.st);
            HIPCHK(hipGetLastError());
            c.sync();  // (done / ctr freed below)
        } else {
            for (int64_t l = 0; l < nlev_L; ++l)
                launch_ilu0_level(Lptr[l + 1] - Lptr[l], rowsL.p + Lptr[l], F.rp.p, F.ci.p, F.val.p, diag.p, dinv.p,
                                  fail.p, F.max_row, max_staged, c.ilu0_stage_cap, c.st);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&hfail, fail.p, sizeof(int32_t), hipMemcpyDeviceToHost, c.st));
        c.sync();
    }
    if (hfail == 3) throw Error("ILU(0): dependency wait exceeded its bound (set pls.ilu_factor_dep 0)");
    if (hfail) throw Error("ILU(0): zero pivot (PETSc: MAT_FACTOR_NUMERIC_ZEROPIVOT)");
}

// Which kernel sweeps: reads the knobs, the block lengths and the level counts
// (and fills the block-major level groups they are counted from); launches
// nothing and builds no table.
PCILU::Sweep PCILU::choose_sweep(Setup &s, const Ctx &c, const Config &cfg) const {
    const int64_t blen = max_len;
    const bool fits_lds = blen <= ilu_lds_max_rows() && cfg.gmem_mode != 1;
    // Blocks too long for LDS: one workgroup per block with y itself as the
    // block solution when levels are narrow -- FE blocks in a bandwidth-
    // reducing order have ~30-150 rows per level and ~1,400 levels at 3-D
    // N=12, where one launch per level is launch-latency bound (measured
    // ~19 us per level).  Wide levels keep the grid-wide launch per level.
    const bool narrow = nlev_L > 0 && n / nlev_L <= 2048;
    const bool gmem = cfg.allow_lds && !fits_lds && cfg.gmem_mode >= 0 && blen <= ilu_gmem_max_rows() &&
                      (narrow || nblocks >= 64 || cfg.gmem_mode == 1);
    if (!(nblocks >= 64 || (fits_lds && cfg.allow_lds) || gmem))  // global levels
        return cfg.gmem_mode == -2 && !exact ? Sweep::LevelsCsr : Sweep::Levels;
    s.L = block_level_groups(s, s.bst, false);
    s.U = block_level_groups(s, s.bst, true);
    if (!((cfg.allow_lds && fits_lds) || gmem)) return Sweep::Levels;
    const int64_t levL = s.L.count(), lev = levL + s.U.count();
    int64_t nw = 0;  // windows per triangle
    for (int64_t b = 0; b < nblocks; ++b) nw += (s.bst[b + 1] - s.bst[b] + 63) / 64;
    auto ring_fits = [&] {
        return c.window_ring != 0 && blen <= ilu_window_ring_max_rows() &&
               window_max_reach(s) <= ilu_window_ring_rows() - 64;
    };
    auto entries_fit = [&] {
        window_max_entries(s, s.eL, s.eU);
        return std::max(s.eL, s.eU) <= ilu_window_max_entries();
    };
    if (gmem) {
        // the super-window sweep: y-resident blocks (pls.sweep_swin; default where
        // the ring sweep would run)
        if (c.sweep_swin != 0 && (c.sweep_swin == 1 || cfg.ring_mode != 0)) return Sweep::Swin;
        // the window sweep's ring variant on blocks too long for LDS (the classical
        // AMG's np=8 hybrid Gauss-Seidel chunks beyond 19,904 rows: swelling N=160,
        // footing N=80), optionally with the L triangle by levels (the y-resident
        // workgroup sweep; pls.window_mixed).  Cost model, a level ~ a window
        // (measured ~2.4 and ~1.9 us on those chunks): both triangles by levels (the
        // ring sweep) levL + levU, both by windows 2 nw, mixed levL + nw; windows
        // where they save a fifth.  Swelling N=160 (per chunk): L 110 levels, U 666,
        // 403 windows per triangle -- mixed; footing N=80: L 154, U 1,034, 467.
        if (c.sweep_window != 0 && ring_fits()) {
            const int64_t cost_lev = lev, cost_win = 2 * nw, cost_mix = levL + nw;
            const bool mix = c.window_mixed == 1 || (c.window_mixed == -1 && cost_mix < cost_win);
            // (pls.ilu_gmem 1 -- the y-resident workgroup sweep forced on blocks that fit
            // LDS -- keeps that sweep unless the window sweep is forced too)
            if ((c.sweep_window == 1 || (cfg.gmem_mode != 1 && 5 * (mix ? cost_mix : cost_win) <= 4 * cost_lev)) &&
                entries_fit())
                return mix ? Sweep::LevelsWindowRing : Sweep::WindowRing;
        }
        // the ring sweep: y-resident blocks whose every level fits one chunk
        const bool ring = cfg.ring_mode != 0 && std::max(s.L.widest(), s.U.widest()) <= ilu_ring_chunk();
        return ring ? Sweep::Ring : Sweep::Gmem;
    }
    if ((c.sweep_chain != 0 || c.sweep_window == 1) && cfg.force_lpr == 0) {
        // the chain sweep (one wave per block, 16-lane steps in order, up to 32
        // steps of factor data in flight) for deep, narrow level DAGs: measured
        // ~0.77 us per level for the workgroup sweep on the footing smoother
        // chunks; a chain step costs a fraction of that, so chain when steps <=
        // 3.5 x levels (both triangles)
        const std::vector<double> none;
        const int64_t sL = build_chain_tri(s, s.L, none, none, nullptr, nullptr);
        const int64_t sU = sL < 0 ? -1 : build_chain_tri(s, s.U, none, none, nullptr, nullptr);
        const bool deep = sL >= 0 && sU >= 0 && 2 * (sL + sU) <= 7 * lev;
        const bool chain = c.sweep_chain != 0 && sL >= 0 && sU >= 0 && (c.sweep_chain == 1 || deep);
        // the window sweep where the chain would run (or forced): a block's
        // dependent chain becomes its len / 64 windows.  Also where the levels
        // outnumber the windows 2:1 (<= 32 rows per level): the classical AMG's
        // level-0 hybrid Gauss-Seidel chunks under mpirun -np 8 semantics
        // (swelling N=80: 8 chunks of 6,481 rows, ~700 levels per chunk over both
        // triangles) took 790 us per sweep in the workgroup sweep (~1.1 us per
        // level), 745 us in the chain sweep, ~250 us in the window sweep (~1.2 us
        // per window)
        const bool many_levels = lev >= 2 * (2 * nw);
        if ((c.sweep_window == 1 || (c.sweep_window == -1 && c.sweep_chain != 1 && (deep || many_levels))) &&
            blen <= ilu_window_max_rows() && entries_fit())
            // (the ring variant forced: tests compare it with the LDS variant)
            return c.window_ring == 1 && ring_fits() ? Sweep::WindowRing : Sweep::Window;
        if (chain) return Sweep::Chain;
    }
    return Sweep::Lds;
}

// threads per workgroup of the level sweeps: as few waves as the widest
// level's slices need (narrow, deep levels -- FE rows in their natural
// order, nearly one level per row -- pay a workgroup barrier per level: 16
// waves cost ~0.6 us per level, one wave far less).  pls.sweep_tpb overrides.
static int level_sweep_tpb(int64_t widest_level, int max_lpr) {
    const int64_t slices = (std::max<int64_t>(widest_level, 1) * max_lpr + 63) / 64;
    return slices <= 1 ? 64 : slices <= 4 ? 256 : 1024;
}

// The device tables of the chosen kind only, from one host copy of the factor values.
void PCILU::build_tables(Setup &s, Ctx &c, const Config &cfg) {
    const std::vector<int64_t> &rp = s.rp, &dg = s.dg, &bst = s.bst;
    if (s.L.off.empty()) {  // global levels
        const TriLevels levU = level_order(s, true);
        nlev_U = levU.count();
        if (sweep == Sweep::LevelsCsr) {
            upload_vec(lrowsL, s.levL.order, c);
            upload_vec(lrowsU, levU.order, c);
            lptrL = s.levL.grp;
            lptrU = levU.grp;
            c.sync();
        } else {
            build_tri_sell(*this, s, s.levL, Lf, c);
            build_tri_sell(*this, s, levU, Uf, c);
        }
        return;
    }
    nlev_U = s.U.count();
    block_levels_h.resize(nblocks);
    for (int64_t b = 0; b < nblocks; ++b)
        block_levels_h[b] = (s.L.off[b + 1] - s.L.off[b]) + (s.U.off[b + 1] - s.U.off[b]);
    block_start_h = bst;
    build_tri_sell(*this, s, s.L, Lf, c);
    build_tri_sell(*this, s, s.U, Uf, c);
    auto download = [&](const DBuf<double> &d, int64_t count) {
        std::vector<double> h(count);
        if (count) HIPCHK(hipMemcpyAsync(h.data(), d.p, sizeof(double) * count, hipMemcpyDeviceToHost, c.st));
        c.sync();
        return h;
    };
    // (the level slices and the LDS streams are filled on the device)
    const bool fill = sweep == Sweep::Levels || sweep == Sweep::Lds || sweep == Sweep::Gmem;
    const std::vector<double> fv = fill ? std::vector<double>() : download(F.val, F.nnz);
    auto upload_wstart = [&] {  // per block its first window
        upload_vec(wstart, Windows(bst).first, c);
        c.sync();
    };
    switch (sweep) {
    case Sweep::Levels:
    case Sweep::LevelsCsr:
        break;
    case Sweep::Swin:
        build_swin_tri(s, fv, false, Lsw, c);
        build_swin_tri(s, fv, true, Usw, c);
        upload_wstart();
        break;
    case Sweep::Window:
    case Sweep::WindowRing:
    case Sweep::LevelsWindowRing:
        window_entries_L = c.window_kpw == 8 ? 32 : s.eL;
        window_entries_U = c.window_kpw == 8 ? 32 : s.eU;
        build_window_tri(s, fv, false, Lw, c);
        build_window_tri(s, fv, true, Uw, c);
        upload_wstart();
        if (sweep == Sweep::LevelsWindowRing) {
            const int lmax = build_lds_tri(*this, s, s.L, cfg.force_lpr, 16, Ls, c, &block_maxsl_h);
            lds_tpb = level_sweep_tpb(s.L.widest(), lmax);
            zgoff.alloc(nblocks + 1);
            HIPCHK(hipMemsetAsync(zgoff.p, 0, sizeof(int64_t) * (nblocks + 1), c.st));
        }
        break;
    case Sweep::Chain: {
        const std::vector<double> dv = download(dinv, n);
        build_chain_tri(s, s.L, fv, dv, &Lc, &c);
        build_chain_tri(s, s.U, fv, dv, &Uc, &c);
        break;
    }
    case Sweep::Ring:
    case Sweep::Gmem:
    case Sweep::Lds: {
        const bool ring = sweep == Sweep::Ring;
        const int max_lpr = sweep == Sweep::Lds ? 4 : (ring ? 32 : 16);
        RingRows rL, rU;
        if (ring) {
            // rows of a level longest first (slices then take fewer lanes per row
            // as rows get shorter); positions follow this order
            for (TriLevels *t : {&s.L, &s.U}) {
                auto len = [&](int32_t i) { return t->upper ? rp[i + 1] - dg[i] - 1 : dg[i] - rp[i]; };
                for (int64_t g = 0; g < t->count(); ++g)
                    std::stable_sort(t->order.begin() + t->grp[g], t->order.begin() + t->grp[g + 1],
                                     [&](int32_t a, int32_t b) { return len(a) > len(b); });
            }
            rL = ring_tables(s, s.L, fv, Lr, c);
            rU = ring_tables(s, s.U, fv, Ur, c);
            // mapUL[b0 + t] = b0 + (L position of the row at U position t)
            std::vector<int32_t> m(n);
            for (int64_t b = 0; b < nblocks; ++b)
                for (int64_t t = bst[b]; t < bst[b + 1]; ++t) m[t] = (int32_t)(bst[b] + rL.posof[s.U.order[t]]);
            upload_vec(mapUL, m, c);
            c.sync();
        }
        const int lL = build_lds_tri(*this, s, s.L, cfg.force_lpr, max_lpr, Ls, c, &block_maxsl_h, ring ? &rL : nullptr);
        const int lU = build_lds_tri(*this, s, s.U, cfg.force_lpr, max_lpr, Us, c, &block_maxsl_h, ring ? &rU : nullptr);
        lds_tpb = level_sweep_tpb(std::max(s.L.widest(), s.U.widest()), std::max(lL, lU));
        // (the round-robin level sweep, pls.sweep_rr 1, is bitwise the same and was
        // measured slower on the footing N=128 smoother chunks: 0.83 vs 0.77 us per
        // level -- the per-level cost there is not memory latency)
        break;
    }
    }
}

void PCILU::apply_blocks(const double *x, double *y, Ctx &c, int64_t b_lo, int64_t b_hi, int rr_group, int tpb,
                         int depth, int64_t *prof) {
    if (!can_apply_blocks()) throw Error("PCILU: block subsets need the LDS sweep");
    const int rr = rr_group > 0 ? rr_group : (lds_rr ? 1 : 0);
    launch_ilu_blocks_lds(n, nblocks, Lf.goff.p, Ls.gslice.p, Ls.sptr.p, Ls.col.p, Ls.val.p, Ls.lpr.p, Uf.goff.p,
                          Us.gslice.p, Us.sptr.p, Us.col.p, Us.val.p, Us.lpr.p, x, y, c.st, prof, false,
                          tpb > 0 ? tpb : lds_tpb, rr, bstart_h.empty() ? nullptr : bstart.p, max_len, b_lo, b_hi,
                          depth == 2 ? lds_depth : depth);
}

const char *PCILU::sweep_kind() const {
    static const char *const names[] = {"levels", "levels-csr", "lds",         "gmem",               "ring",
                                        "chain",  "window",     "window-ring", "levels+window-ring", "swin"};
    return names[(int)sweep];
}

void PCILU::apply(const double *x, double *y, Ctx &c) {
    const int64_t *bs = bstart_h.empty() ? nullptr : bstart.p;
    switch (sweep) {
    case Sweep::Swin:
        launch_ilu_blocks_swin(n, nblocks, bs, wstart.p, Lsw.bsw.p, Lsw.sw.p, Lsw.wnear.p, Lsw.ncol.p, Lsw.nval.p,
                               Lsw.wfar.p, Lsw.fcol.p, Lsw.fval.p, Lsw.tinv.p, Usw.bsw.p, Usw.sw.p, Usw.wnear.p,
                               Usw.ncol.p, Usw.nval.p, Usw.wfar.p, Usw.fcol.p, Usw.fval.p, Usw.tinv.p, x, y,
                               std::max(Lsw.lds_bytes, Usw.lds_bytes), c.st);
        return;
    case Sweep::Ring: {
        auto &sc = ring_scratch[c.st];  // per stream: the concurrent 3-way sweeps share this PC
        if (sc.first.n < (size_t)n) {
            sc.first.alloc(std::max<int64_t>(n, 1));
            sc.second.alloc(std::max<int64_t>(n, 1));
        }
        launch_ilu_blocks_ring(n, nblocks, Lf.goff.p, Ls.gslice.p, Ls.sptr.p, Ls.col.p, Ls.val.p, Ls.lpr.p, Uf.goff.p,
                               Us.gslice.p, Us.sptr.p, Us.col.p, Us.val.p, Us.lpr.p, Lr.coff.p, Lr.cg.p, Lr.cp.p,
                               Ur.coff.p, Ur.cg.p, Ur.cp.p, Lr.ord.p, mapUL.p, Ur.ord.p, Lr.frp.p, Lr.fcol.p,
                               Lr.fval.p, Ur.frp.p, Ur.fcol.p, Ur.fval.p, x, y, sc.first.p, sc.second.p, c.st,
                               lds_tpb, bs);
        return;
    }
    case Sweep::LevelsWindowRing:  // L: the y-resident level sweep; U: the ring windows
        launch_ilu_blocks_lds(n, nblocks, Lf.goff.p, Ls.gslice.p, Ls.sptr.p, Ls.col.p, Ls.val.p, Ls.lpr.p, zgoff.p,
                              Ls.gslice.p, Ls.sptr.p, Ls.col.p, Ls.val.p, Ls.lpr.p, x, y, c.st, nullptr, true, lds_tpb,
                              0, bs, max_len, -1, -1, 2);
        launch_ilu_blocks_window(n, nblocks, bs, wstart.p, Lw.woff.p, Lw.rec.p, Lw.tinv.p, Uw.woff.p, Uw.rec.p,
                                 Uw.tinv.p, y, y, max_len, c.st, c.window_depth, true, 2, window_entries_L,
                                 window_entries_U);
        return;
    case Sweep::Window:
    case Sweep::WindowRing:
        launch_ilu_blocks_window(n, nblocks, bs, wstart.p, Lw.woff.p, Lw.rec.p, Lw.tinv.p, Uw.woff.p, Uw.rec.p,
                                 Uw.tinv.p, x, y, max_len, c.st, c.window_depth, sweep == Sweep::WindowRing, 3,
                                 window_entries_L, window_entries_U);
        return;
    case Sweep::Chain:
        launch_ilu_blocks_chain(n, nblocks, bs, Lc.base.p, Lc.soff.p, Lc.sz.p, Lc.nsl.p, Lc.lpr.p, Lc.col.p, Lc.val.p,
                                Uc.base.p, Uc.soff.p, Uc.sz.p, Uc.nsl.p, Uc.lpr.p, Uc.col.p, Uc.val.p, x, y, max_len,
                                c.st);
        return;
    case Sweep::Lds:
    case Sweep::Gmem: {
        const bool gmem = sweep == Sweep::Gmem;
        DBuf<int64_t> prof;
        if (!profile_tag.empty()) prof.alloc(nblocks * 8);
        launch_ilu_blocks_lds(n, nblocks, Lf.goff.p, Ls.gslice.p, Ls.sptr.p, Ls.col.p, Ls.val.p, Ls.lpr.p, Uf.goff.p,
                              Us.gslice.p, Us.sptr.p, Us.col.p, Us.val.p, Us.lpr.p, x, y, c.st, prof.p, gmem, lds_tpb,
                              lds_rr ? 1 : 0, bs, max_len, -1, -1, gmem ? 2 : lds_depth);
        if (!profile_tag.empty()) print_profile(prof, c);
        return;
    }
    case Sweep::LevelsCsr:
        for (int64_t l = 0; l < nlev_L; ++l)
            launch_tri_csr_level(lptrL[l + 1] - lptrL[l], lrowsL.p + lptrL[l], F.rp.p, F.ci.p, F.val.p, diag.p,
                                 dinv.p, 0, x, y, c.st);
        for (int64_t l = 0; l < nlev_U; ++l)
            launch_tri_csr_level(lptrU[l + 1] - lptrU[l], lrowsU.p + lptrU[l], F.rp.p, F.ci.p, F.val.p, diag.p,
                                 dinv.p, 1, y, y, c.st);
        return;
    case Sweep::Levels:
        Lf.apply(x, y, c);
        Uf.apply(y, y, c);
        return;
    }
}

// pls.sweep_profile: per-block sweep times (100 MHz wall clock), slowest first, once
void PCILU::print_profile(const DBuf<int64_t> &prof, Ctx &c) {
    std::vector<int64_t> h(nblocks * 8);
    HIPCHK(hipMemcpyAsync(h.data(), prof.p, sizeof(int64_t) * h.size(), hipMemcpyDeviceToHost, c.st));
    c.sync();
    int64_t tmin = INT64_MAX, tmax = 0;
    std::vector<int64_t> order(nblocks);
    for (int64_t b = 0; b < nblocks; ++b) {
        order[b] = b;
        tmin = std::min(tmin, h[b * 8]);
        tmax = std::max(tmax, h[b * 8 + 2]);
    }
    std::sort(order.begin(), order.end(),
              [&](int64_t a, int64_t b) { return h[a * 8 + 2] - h[a * 8] > h[b * 8 + 2] - h[b * 8]; });
    fprintf(stderr, "[sweep %s] %lld blocks, kernel span %.1f us\n", profile_tag.c_str(), (long long)nblocks,
            (tmax - tmin) * 0.01);
    for (int64_t r = 0; r < std::min<int64_t>(nblocks, 12); ++r) {
        const int64_t b = order[r], *p = &h[b * 8];
        fprintf(stderr,
                "  blk %4lld rows %6lld start %+8.1f us  L %7.1f us (%4lld lv, %5lld sl)  U %7.1f us (%4lld lv)"
                "  lanes/row L,U %lld,%lld\n",
                (long long)b, (long long)p[5], (p[0] - tmin) * 0.01, (p[1] - p[0]) * 0.01, (long long)p[3],
                (long long)p[6], (p[2] - p[1]) * 0.01, (long long)p[4], (long long)(p[7] / 10),
                (long long)(p[7] % 10));
    }
    profile_tag.clear();
}

}  // namespace pls
