// runtime.cpp -- device memory, options, timers, operators, preconditioners
// and the fieldsplit PC of libpls.so.  The Krylov solvers are in ksp.cpp, the
// block ILU(0) / Gauss-Seidel preconditioner (PCILU) in ilu.cpp.
#include "runtime.hpp"

#include <sys/mman.h>

#include <algorithm>
#include <thread>
#include <functional>
#include <numeric>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <sstream>

namespace pls {

void *huge_alloc(size_t bytes) {
    const size_t len = (bytes + HUGE_ALLOC_MIN - 1) & ~(HUGE_ALLOC_MIN - 1);
    void *p = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (p == MAP_FAILED) throw std::bad_alloc();
    (void)madvise(p, len, MADV_HUGEPAGE);
    return p;
}
void huge_free(void *p, size_t bytes) {
    if (p) (void)munmap(p, (bytes + HUGE_ALLOC_MIN - 1) & ~(HUGE_ALLOC_MIN - 1));
}

// ============================================================== context ===
static CommSelf g_self_comm;

Ctx::Ctx() {
    comm = &g_self_comm;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    partial.alloc(4096 * 136);
    partial_n = 4096 * 136;
    dscal.alloc(4096);
    HIPCHK(hipHostMalloc((void **)&hscal, sizeof(double) * 4096, hipHostMallocDefault));
    hscal_n = 4096;
}
static constexpr double CANARY_VALUE = -1.2345678901234567e300;

static void alloc_partial(Ctx &c, int64_t count) {
    c.partial.alloc(count + (c.debug_bounds ? Ctx::CANARY : 0));
    c.partial_n = count;
    if (c.debug_bounds) launch_set(Ctx::CANARY, CANARY_VALUE, c.partial.p + count, c.st);
}
void Ctx::set_debug(bool bounds, int64_t cap, bool no_grow, bool unguarded) {
    HIPCHK(hipStreamSynchronize(st));
    debug_bounds = bounds;
    debug_no_grow = no_grow;
    debug_unguarded = unguarded;
    alloc_partial(*this, cap > 0 ? cap : partial_n);
    HIPCHK(hipStreamSynchronize(st));
}
void Ctx::check_bounds() {
    if (!debug_bounds) return;
    std::vector<double> h(CANARY);
    HIPCHK(hipMemcpyAsync(h.data(), partial.p + partial_n, sizeof(double) * CANARY, hipMemcpyDeviceToHost, st));
    sync();
    for (int64_t i = 0; i < CANARY; ++i)
        if (h[i] != CANARY_VALUE)
            throw Error("pls.debug_bounds: the canary behind the reduction partials was overwritten at +" +
                        std::to_string(i) + " (room " + std::to_string(partial_n) + " doubles)");
}
double *Ctx::partials(int64_t n, int64_t cols) {
    const int64_t need = (int64_t)reduce_blocks(n) * std::max<int64_t>(cols, 1);
    if (need > partial_n && !debug_unguarded)
        throw Error("reduction partials: " + std::to_string(cols) + " reductions of " + std::to_string(n) +
                    " entries need " + std::to_string(need) + " doubles, the context holds " +
                    std::to_string(partial_n) + " (missing ensure_partial)");
    return partial.p;
}
double *Ctx::host_scalars(int64_t count) {
    if (count > hscal_n)
        throw Error("host scalar mirror: " + std::to_string(count) + " doubles requested, " + std::to_string(hscal_n) +
                    " held (missing ensure_partial)");
    return hscal;
}
void Ctx::ensure_partial(int64_t n, int64_t cols) {
    const int64_t need = (int64_t)reduce_blocks(n) * std::max<int64_t>(cols, 1);
    if (need > partial_n && !debug_no_grow) {
        HIPCHK(hipStreamSynchronize(st));
        alloc_partial(*this, need);
    }
    if (cols + 2 > hscal_n) {
        HIPCHK(hipStreamSynchronize(st));
        if (hscal) (void)hipHostFree(hscal);
        HIPCHK(hipHostMalloc((void **)&hscal, sizeof(double) * (cols + 2), hipHostMallocDefault));
        hscal_n = cols + 2;
    }
}
Ctx::~Ctx() {
    if (hscal) (void)hipHostFree(hscal);
    if (ev_x) (void)hipEventDestroy(ev_x);
    if (ev_halo) (void)hipEventDestroy(ev_halo);
    if (st_comm) (void)hipStreamDestroy(st_comm);
    if (st) (void)hipStreamDestroy(st);
}
void Ctx::ensure_scan(int64_t n) {
    size_t need = exclusive_scan_tmp_bytes(n);
    if (need > scan_tmp_bytes) {
        scan_tmp.alloc(need);
        scan_tmp_bytes = need;
    }
}
double Ctx::dot(int64_t n, const double *x, const double *y) {
    launch_dot(n, x, y, partials(n, 1), dscal.p, st);
    comm->global_sum_dev(dscal.p, 1, st);
    double *h = host_scalars(1);
    HIPCHK(hipMemcpyAsync(h, dscal.p, sizeof(double), hipMemcpyDeviceToHost, st));
    sync();
    return h[0];
}
double Ctx::norm2(int64_t n, const double *x) {
    launch_dot(n, x, x, partials(n, 1), dscal.p, st);
    comm->global_sum_dev(dscal.p, 1, st);
    double *h = host_scalars(1);
    HIPCHK(hipMemcpyAsync(h, dscal.p, sizeof(double), hipMemcpyDeviceToHost, st));
    sync();
    return std::sqrt(h[0]);
}

// ================================================================== CSR ===
void upload_csr(DevCSR &M, int64_t nrows, int64_t ncols, const int64_t *rp, const int32_t *ci, const double *val,
                Ctx &c) {
    M.nrows = nrows;
    M.ncols = ncols;
    M.nnz = rp[nrows] - rp[0];
    if (rp[0] != 0) throw Error("CSR row_ptr must start at 0");
    int64_t mr = 0;
    for (int64_t i = 0; i < nrows; ++i) {
        const int64_t l = rp[i + 1] - rp[i];
        if (l < 0) throw Error("CSR row_ptr not monotone");
        mr = std::max(mr, l);
        for (int64_t k = rp[i] + 1; k < rp[i + 1]; ++k)
            if (ci[k] <= ci[k - 1]) throw Error("CSR columns must be strictly ascending within a row");
        if (l > 0 && (ci[rp[i]] < 0 || ci[rp[i + 1] - 1] >= ncols)) throw Error("CSR column index out of range");
    }
    M.max_row = mr;
    M.rp.alloc(nrows + 1);
    M.ci.alloc(std::max<int64_t>(M.nnz, 1));
    M.val.alloc(std::max<int64_t>(M.nnz, 1));
    HIPCHK(hipMemcpyAsync(M.rp.p, rp, sizeof(int64_t) * (nrows + 1), hipMemcpyHostToDevice, c.st));
    if (M.nnz) {
        HIPCHK(hipMemcpyAsync(M.ci.p, ci, sizeof(int32_t) * M.nnz, hipMemcpyHostToDevice, c.st));
        HIPCHK(hipMemcpyAsync(M.val.p, val, sizeof(double) * M.nnz, hipMemcpyHostToDevice, c.st));
    }
    c.sync();
}

static int64_t max_row_of(const DBuf<int64_t> &rp, int64_t nrows, Ctx &c) {
    std::vector<int64_t> h(nrows + 1);
    HIPCHK(hipMemcpyAsync(h.data(), rp.p, sizeof(int64_t) * (nrows + 1), hipMemcpyDeviceToHost, c.st));
    c.sync();
    int64_t m = 0;
    for (int64_t i = 0; i < nrows; ++i) m = std::max(m, h[i + 1] - h[i]);
    return m;
}

void extract_csr(const DevCSR &src, int64_t r0, int64_t r1, WindowSpec w, int64_t cshift, int64_t ncols,
                 DevCSR &dst, Ctx &c) {
    const int64_t nl = r1 - r0;
    dst.sell.reset();  // re-extraction (matrix update): the SpMV layout is rebuilt on demand
    dst.halo.reset();
    DBuf<int64_t> len(nl + 1);
    launch_extract_count(src.rp.p, src.ci.p, r0, r1, w, len.p, c.st);
    dst.rp.alloc(nl + 1);
    c.ensure_scan(nl);
    exclusive_scan_i64(len.p, dst.rp.p, nl, c.scan_tmp.p, c.scan_tmp_bytes, c.st);
    int64_t nnz = 0;
    HIPCHK(hipMemcpyAsync(&nnz, dst.rp.p + nl, sizeof(int64_t), hipMemcpyDeviceToHost, c.st));
    c.sync();
    dst.nrows = nl;
    dst.ncols = ncols;
    dst.nnz = nnz;
    dst.ci.alloc(std::max<int64_t>(nnz, 1));
    dst.val.alloc(std::max<int64_t>(nnz, 1));
    launch_extract_fill(src.rp.p, src.ci.p, src.val.p, r0, r1, w, cshift, dst.rp.p, dst.ci.p, dst.val.p, c.st);
    HIPCHK(hipGetLastError());
    dst.max_row = max_row_of(dst.rp, nl, c);
}

// Slice plan of the D16 layout: per 64-row group, 8 lanes per row when the
// group's rows are "wide" (first columns of neighbouring rows more than 4
// apart on average, rows of 16+ entries: a lane-per-row gather would touch a
// cache line per lane), else lane = row.
//
// Rows of very different lengths in one slice pad every lane to the longest
// (FE systems in a bandwidth-reducing order interleave P2 vertex, P2 edge and
// P1 rows of 89..405 entries: ~100 % padding, 1.7x the CSR bytes).  When the
// padding exceeds pls.d16_sigma_pad (15 %), the plan becomes SELL-C-sigma:
// inside windows of pls.d16_sigma (1024) rows the rows are stably sorted by
// length (rowmap[position] = row; the kernel writes y[rowmap[pos]]), and each
// 64-row group of positions takes pls.d16_sorted_lpr (2) lanes per row when
// its rows average 32+ entries (keeps a gather instruction on few cache
// lines), else 1.  Per-row summation order is unchanged for lane-per-row
// slices; it is the sorted plan only if it saves 15 % of the stored entries.
static int64_t d16_plan_stored(const std::vector<int64_t> &rp, const std::vector<int64_t> &sfirst,
                               const std::vector<int32_t> &slpr, const std::vector<int32_t> *rowmap) {
    int64_t stored = 0;
    for (size_t s = 0; s + 1 < sfirst.size(); ++s) {
        const int l = slpr[s];
        int64_t L = 0;
        for (int64_t p = sfirst[s]; p < sfirst[s + 1]; ++p) {
            const int64_t r = rowmap ? (*rowmap)[p] : p;
            L = std::max<int64_t>(L, (rp[r + 1] - rp[r] + l - 1) / l);
        }
        stored += 64 * ((L + 7) & ~(int64_t)7);
    }
    return stored;
}

static void d16_plan(const DevCSR &M, std::vector<int64_t> &sfirst, std::vector<int32_t> &slpr,
                     std::vector<int32_t> &rowmap, Ctx &c, const std::vector<int32_t> *subset = nullptr) {
    const int64_t n = M.nrows;
    std::vector<int64_t> rp(n + 1);
    std::vector<int32_t> c0(n);
    DBuf<int32_t> dc0(std::max<int64_t>(n, 1));
    launch_first_col(n, M.rp.p, M.ci.p, dc0.p, c.st);
    HIPCHK(hipMemcpyAsync(rp.data(), M.rp.p, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, c.st));
    HIPCHK(hipMemcpyAsync(c0.data(), dc0.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c.st));
    c.sync();
    sfirst.clear();
    slpr.clear();
    rowmap.clear();
    if (subset) {
        // the rows left to the D16 part by the B3 layout: always the sorted plan
        std::vector<int32_t> rm(*subset);
        const int64_t m = (int64_t)rm.size();
        for (int64_t w = 0; w < m; w += std::max(c.d16_sigma, 64)) {
            const int64_t e = std::min<int64_t>(m, w + std::max(c.d16_sigma, 64));
            std::stable_sort(rm.begin() + w, rm.begin() + e,
                             [&](int32_t a, int32_t b) { return rp[a + 1] - rp[a] > rp[b + 1] - rp[b]; });
        }
        for (int64_t p = 0; p < m; p += 64) {
            const int64_t e = std::min<int64_t>(m, p + 64);
            int64_t tot = 0;
            for (int64_t q = p; q < e; ++q) tot += rp[rm[q] + 1] - rp[rm[q]];
            const int l = (c.d16_sorted_lpr > 1 && tot >= 32 * (e - p)) ? c.d16_sorted_lpr : 1;
            for (int64_t q = p; q < e; q += 64 / l) {
                sfirst.push_back(q);
                slpr.push_back(l);
            }
        }
        sfirst.push_back(m);
        rowmap.swap(rm);
        return;
    }
    for (int64_t r = 0; r < n; r += 64) {
        bool wide = false;
        if (r + 64 <= n && c0[r] >= 0 && c0[r + 63] >= 0) {
            const int64_t spread = (int64_t)c0[r + 63] - (int64_t)c0[r];
            const int64_t avg = (rp[r + 64] - rp[r]) / 64;
            wide = spread > 4 * 63 && avg >= 16;
        }
        if (wide) {
            const int l = c.d16_wide_lpr;
            for (int q = 0; q < l; ++q) {
                sfirst.push_back(r + (64 / l) * q);
                slpr.push_back(l);
            }
        } else {
            sfirst.push_back(r);
            slpr.push_back(1);
        }
    }
    sfirst.push_back(n);
    if (c.d16_sigma <= 0 || M.halo || n < 64) return;
    const int64_t nnz = rp[n];
    const int64_t stored = d16_plan_stored(rp, sfirst, slpr, nullptr);
    if ((double)stored <= (1.0 + c.d16_sigma_pad) * (double)nnz) return;
    // SELL-C-sigma
    std::vector<int32_t> rm(n);
    std::iota(rm.begin(), rm.end(), 0);
    for (int64_t w = 0; w < n; w += c.d16_sigma) {
        const int64_t e = std::min<int64_t>(n, w + c.d16_sigma);
        std::stable_sort(rm.begin() + w, rm.begin() + e, [&](int32_t a, int32_t b) {
            return rp[a + 1] - rp[a] > rp[b + 1] - rp[b];
        });
    }
    std::vector<int64_t> sf;
    std::vector<int32_t> sl;
    // entries a group of positions [p, e) stores with l lanes per row
    auto group_stored = [&](int64_t p, int64_t e, int l) {
        int64_t st = 0;
        for (int64_t q = p; q < e; q += 64 / l) {
            int64_t L = 0;
            for (int64_t t = q; t < std::min(e, q + 64 / l); ++t) L = std::max<int64_t>(L, (rp[rm[t] + 1] - rp[rm[t]] + l - 1) / l);
            st += 64 * ((L + 7) & ~(int64_t)7);
        }
        return st;
    };
    for (int64_t p = 0; p < n; p += 64) {
        const int64_t e = std::min<int64_t>(n, p + 64);
        int64_t tot = 0;
        for (int64_t q = p; q < e; ++q) tot += rp[rm[q] + 1] - rp[rm[q]];
        // several lanes per row only for long rows, and only when the per-lane
        // share's rounding to 8-entry groups costs little extra padding
        int l = 1;
        if (c.d16_sorted_lpr > 1 && tot >= 32 * (e - p) &&
            (double)group_stored(p, e, c.d16_sorted_lpr) <= 1.05 * (double)group_stored(p, e, 1))
            l = c.d16_sorted_lpr;
        for (int64_t q = p; q < e; q += 64 / l) {
            sf.push_back(q);
            sl.push_back(l);
        }
    }
    sf.push_back(n);
    const int64_t stored2 = d16_plan_stored(rp, sf, sl, &rm);
    if ((double)stored2 > 0.85 * (double)stored) return;
    sfirst.swap(sf);
    slpr.swap(sl);
    rowmap.swap(rm);
}

// SELL/B3: row triples with one column list (the components of a P2 node in
// an FE vector field).  Used when such triples hold >= half the entries; the
// other rows go to a D16 part (returned in `singles`).  Triples are sorted by
// length inside windows of 512 (SELL-C-sigma); slices of 64 / b3_lanes_per_triple() triples.
static bool build_b3(const DevCSR &M, DevSELL &S, std::vector<int32_t> &singles, Ctx &c) {
    const int64_t n = M.nrows;
    if (!c.spmv_b3 || M.halo || n < 192) return false;
    DBuf<uint8_t> df(n);
    launch_triple_flags(n, M.rp.p, M.ci.p, df.p, c.st);
    std::vector<uint8_t> f(n);
    std::vector<int64_t> rp(n + 1);
    HIPCHK(hipMemcpyAsync(f.data(), df.p, n, hipMemcpyDeviceToHost, c.st));
    HIPCHK(hipMemcpyAsync(rp.data(), M.rp.p, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, c.st));
    c.sync();
    std::vector<int32_t> heads;
    singles.clear();
    int64_t tnnz = 0;
    for (int64_t r = 0; r < n;) {
        if (f[r]) {
            heads.push_back((int32_t)r);
            tnnz += 3 * (rp[r + 1] - rp[r]);
            r += 3;
        } else {
            singles.push_back((int32_t)r);
            r += 1;
        }
    }
    if (2 * tnnz < M.nnz) return false;
    const int64_t nt = (int64_t)heads.size(), W = 512;
    for (int64_t w = 0; w < nt; w += W) {
        const int64_t e = std::min(nt, w + W);
        std::stable_sort(heads.begin() + w, heads.begin() + e,
                         [&](int32_t a, int32_t b) { return rp[a + 1] - rp[a] > rp[b + 1] - rp[b]; });
    }
    const int64_t lpt = b3_lanes_per_triple(), per = 64 / lpt, ns = (nt + per - 1) / per;
    std::vector<int64_t> bptr(ns + 1, 0);
    for (int64_t sl = 0; sl < ns; ++sl) {
        int64_t L = 0;
        for (int64_t t = sl * per; t < std::min(nt, sl * per + per); ++t)
            L = std::max<int64_t>(L, (rp[heads[t] + 1] - rp[heads[t]] + lpt - 1) / lpt);
        bptr[sl + 1] = bptr[sl] + 64 * L;
    }
    S.b3_nslices = ns;
    S.b3_ntrip = nt;
    S.b3_stored = bptr[ns];
    S.b3ptr.alloc(ns + 1);
    S.b3map.alloc(std::max<int64_t>(nt, 1));
    S.b3col.alloc(std::max<int64_t>(S.b3_stored, 1));
    S.b3val.alloc(std::max<int64_t>(3 * S.b3_stored, 1));
    HIPCHK(hipMemcpyAsync(S.b3ptr.p, bptr.data(), sizeof(int64_t) * (ns + 1), hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemcpyAsync(S.b3map.p, heads.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice, c.st));
    launch_b3_fill(ns, nt, S.b3ptr.p, S.b3map.p, M.rp.p, M.ci.p, M.val.p, S.b3col.p, S.b3val.p, c.st);
    HIPCHK(hipGetLastError());
    c.sync();
    return true;
}

// Reverse Cuthill-McKee order of a square pattern (host): per component, BFS
// from a pseudo-peripheral vertex visiting neighbours by increasing degree,
// then reversed.  order[new] = old.
static std::vector<int32_t> rcm_order(const hvec<int64_t> &rp, const hvec<int32_t> &ci, int64_t n) {
    std::vector<int32_t> order, lev(n, -1);
    order.reserve(n);
    std::vector<char> done(n, 0);
    auto deg = [&](int32_t v) { return rp[v + 1] - rp[v]; };
    std::vector<int32_t> q, nb;
    auto bfs_last = [&](int32_t s) {  // last vertex of a plain BFS (pseudo-peripheral sweep)
        q.assign(1, s);
        lev[s] = 0;
        for (size_t h = 0; h < q.size(); ++h)
            for (int64_t k = rp[q[h]]; k < rp[q[h] + 1]; ++k)
                if (lev[ci[k]] < 0 && !done[ci[k]]) {
                    lev[ci[k]] = lev[q[h]] + 1;
                    q.push_back(ci[k]);
                }
        const int32_t last = q.back();
        for (int32_t v : q) lev[v] = -1;
        return last;
    };
    for (int64_t s0 = 0; s0 < n;) {
        // s0 again until it is ordered: in a pattern that is not symmetric the sweep can end in
        // vertices s0 reaches that do not reach s0 back
        if (done[s0]) {
            ++s0;
            continue;
        }
        int32_t s = bfs_last(bfs_last((int32_t)s0));
        size_t h = order.size();
        order.push_back(s);
        done[s] = 1;
        for (; h < order.size(); ++h) {
            const int32_t u = order[h];
            nb.clear();
            for (int64_t k = rp[u]; k < rp[u + 1]; ++k)
                if (!done[ci[k]]) {
                    done[ci[k]] = 1;
                    nb.push_back(ci[k]);
                }
            std::stable_sort(nb.begin(), nb.end(), [&](int32_t a, int32_t b) { return deg(a) < deg(b); });
            order.insert(order.end(), nb.begin(), nb.end());
        }
    }
    std::reverse(order.begin(), order.end());
    return order;
}

// The D16 layout of M with rows and columns relabelled by RCM (FE matrices:
// the caller's order interleaves P2 vertex, P2 edge and P1 dofs, so a slice's
// rows gather x from several far-apart ranges); the slices map back to M's
// rows through rowmap, and x is gathered into the RCM order before each product.
static bool build_sell_rcm(DevCSR &M, Ctx &c) {
    const int64_t n = M.nrows;
    const HostCSR H = download(M, c);
    const std::vector<int32_t> ord = rcm_order(H.rp, H.ci, n);
    std::vector<int32_t> inv(n);
    for (int64_t i = 0; i < n; ++i) inv[ord[i]] = (int32_t)i;
    HostCSR P;
    P.nrows = P.ncols = n;
    P.rp.assign(n + 1, 0);
    P.ci.resize(H.ci.size());
    P.v.resize(H.v.size());
    std::vector<std::pair<int32_t, double>> row;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t o = ord[i];
        row.clear();
        for (int64_t k = H.rp[o]; k < H.rp[o + 1]; ++k) row.emplace_back(inv[H.ci[k]], H.v[k]);
        std::sort(row.begin(), row.end(), [](auto &a, auto &b) { return a.first < b.first; });
        for (size_t t = 0; t < row.size(); ++t) {
            P.ci[P.rp[i] + t] = row[t].first;
            P.v[P.rp[i] + t] = row[t].second;
        }
        P.rp[i + 1] = P.rp[i] + (int64_t)row.size();
    }
    DevCSR Mp;
    upload(P, Mp, c);
    const int keep = c.spmv_rcm;
    c.spmv_rcm = 0;
    build_sell(Mp, c);
    c.spmv_rcm = keep;
    if (!Mp.sell || !Mp.sell->d16 || Mp.sell->b3_nslices) return false;
    DevSELL &S = *Mp.sell;
    std::vector<int32_t> rm(n);
    if (S.nrows_mapped) {
        HIPCHK(hipMemcpyAsync(rm.data(), S.rowmap.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c.st));
        c.sync();
        for (auto &r : rm) r = ord[r];
    } else {
        rm = ord;
    }
    S.rowmap.alloc(n);
    S.nrows_mapped = n;
    HIPCHK(hipMemcpyAsync(S.rowmap.p, rm.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, c.st));
    S.xperm.alloc(n);
    HIPCHK(hipMemcpyAsync(S.xperm.p, ord.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, c.st));
    S.nperm = n;
    if (c.rcm_x.n < (size_t)n) c.rcm_x.alloc(n);
    c.sync();
    M.sell = std::move(Mp.sell);
    return true;
}

// Shared delta stream of a filled D16 layout (pls.d16_share; format: kernels.hip).  Auto (-1)
// takes it where a product re-streams the matrix from memory -- the plain layout exceeds
// pls.d16_share_min_bytes, the size of the last-level cache -- and the shared layout is
// smaller; otherwise S stays as it is.  Only the totals come back to the host.
static void d16_share(DevSELL &S, Ctx &c) {
    const int64_t ns = S.nslices;
    if (c.d16_share == 0 || ns == 0 || S.stored == 0) return;
    if (c.d16_share < 0 && S.bytes() <= c.d16_share_min_bytes) return;
    DBuf<uint8_t> cls(ns * 64);
    DBuf<int64_t> cnt(ns + 1), dptr(ns + 1), nshared(1);
    HIPCHK(hipMemsetAsync(nshared.p, 0, sizeof(int64_t), c.st));
    launch_d16_share_classes(ns, S.sptr.p, S.dl.p, cls.p, cnt.p, nshared.p, c.st);
    c.ensure_scan(ns);
    exclusive_scan_i64(cnt.p, dptr.p, ns, c.scan_tmp.p, c.scan_tmp_bytes, c.st);
    int64_t total = 0, shared = 0;
    HIPCHK(hipMemcpyAsync(&total, dptr.p + ns, sizeof(int64_t), hipMemcpyDeviceToHost, c.st));
    HIPCHK(hipMemcpyAsync(&shared, nshared.p, sizeof(int64_t), hipMemcpyDeviceToHost, c.st));
    c.sync();
    if (c.d16_share < 0 && total * 2 + ns * 72 + 8 >= S.stored * 2) return;  // nothing saved
    DBuf<uint16_t> dls(std::max<int64_t>(total, 8));
    launch_d16_share_fill(ns, S.sptr.p, dptr.p, cls.p, S.dl.p, dls.p, c.st);
    HIPCHK(hipGetLastError());
    c.sync();
    S.dl = std::move(dls);  // (frees the plain stream)
    S.dptr = std::move(dptr);
    S.cls = std::move(cls);
    S.dstored = total;
    S.shared_slices = shared;
    ++c.d16_share_built;
}

// The D16 arrays of M for a slice plan (sfirst, slpr, rowmap of d16_plan); rstart: see
// launch_d16_fill.  False (S.d16 unset) when a lane needs more than D16_SEG_MAX segments.
static bool d16_from_plan(const DevCSR &M, DevSELL &S, const std::vector<int64_t> &sf, const std::vector<int32_t> &lp,
                          const std::vector<int32_t> &rm, const int64_t *rstart, Ctx &c) {
    const int64_t ns = (int64_t)lp.size();
    S.sfirst.alloc(ns + 1);
    S.slpr.alloc(std::max<int64_t>(ns, 1));
    HIPCHK(hipMemcpyAsync(S.sfirst.p, sf.data(), sizeof(int64_t) * (ns + 1), hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemcpyAsync(S.slpr.p, lp.data(), sizeof(int32_t) * ns, hipMemcpyHostToDevice, c.st));
    if (!rm.empty()) {
        S.rowmap.alloc(rm.size());
        S.nrows_mapped = (int64_t)rm.size();
        HIPCHK(hipMemcpyAsync(S.rowmap.p, rm.data(), sizeof(int32_t) * rm.size(), hipMemcpyHostToDevice, c.st));
    }
    const int32_t *rmap = rm.empty() ? nullptr : S.rowmap.p;
    DBuf<int32_t> mx(1);
    HIPCHK(hipMemsetAsync(mx.p, 0, sizeof(int32_t), c.st));
    launch_d16_count(ns, S.sfirst.p, S.slpr.p, M.rp.p, M.ci.p, M.nrows, mx.p, c.st, rmap, rstart);
    int32_t h = 0;
    HIPCHK(hipMemcpyAsync(&h, mx.p, sizeof(int32_t), hipMemcpyDeviceToHost, c.st));
    c.sync();
    S.d16 = h <= D16_SEG_MAX;
    S.nsegs = (h <= D16_SEG && c.d16_segs <= D16_SEG) ? D16_SEG : D16_SEG_MAX;
    if (!S.d16) return false;
    S.nslices = ns;
    for (int32_t l : lp) S.wide_slices += (l > 1);
    DBuf<int64_t> slen(ns + 1);
    launch_d16_slice_len(ns, S.sfirst.p, S.slpr.p, M.rp.p, M.nrows, slen.p, c.st, rmap, rstart);
    S.sptr.alloc(ns + 1);
    c.ensure_scan(ns);
    exclusive_scan_i64(slen.p, S.sptr.p, ns, c.scan_tmp.p, c.scan_tmp_bytes, c.st);
    HIPCHK(hipMemcpyAsync(&S.stored, S.sptr.p + ns, sizeof(int64_t), hipMemcpyDeviceToHost, c.st));
    c.sync();
    S.val.alloc(std::max<int64_t>(S.stored, 2));
    S.dl.alloc(std::max<int64_t>(S.stored, 8));
    S.seg.alloc(ns * 64 * S.nsegs);
    launch_d16_fill(ns, S.sfirst.p, S.slpr.p, M.rp.p, M.ci.p, M.val.p, M.nrows, S.sptr.p, S.dl.p, S.val.p, S.seg.p,
                    S.nsegs, c.st, rmap, rstart);
    HIPCHK(hipGetLastError());
    c.sync();
    S.dstored = S.stored;
    d16_share(S, c);
    return true;
}

void build_sell(DevCSR &M, Ctx &c) {
    if (M.sell || M.nrows == 0) return;
    if (c.spmv_rcm != 0 && c.sell_d16 && !c.spmv_b3 && !M.halo && M.nrows == M.ncols && M.nrows >= 16384) {
        bool pads = c.spmv_rcm == 1;
        if (!pads && M.rcm_auto) {  // only where the plain plan pads (FE): the synthetic blocks keep their layout
            std::vector<int64_t> sf;
            std::vector<int32_t> lp, rm;
            d16_plan(M, sf, lp, rm, c);
            pads = !rm.empty();
        }
        if (pads && build_sell_rcm(M, c)) return;
    }
    auto S = std::make_unique<DevSELL>();
    if (c.sell_d16 && M.nnz > 0) {
        std::vector<int64_t> sf;
        std::vector<int32_t> lp, rm, singles;
        const bool b3 = build_b3(M, *S, singles, c);
        d16_plan(M, sf, lp, rm, c, b3 ? &singles : nullptr);
        const int64_t ns = (int64_t)lp.size();
        if (ns == 0) {  // every row in a triple: the B3 part is the whole product
            S->d16 = true;
            M.sell = std::move(S);
            return;
        }
        if (d16_from_plan(M, *S, sf, lp, rm, nullptr, c)) {
            M.sell = std::move(S);
            if (M.halo) classify_halo_slices(M, c);
            return;
        }
        if (b3) {  // the other rows do not fit D16: plain layouts for the whole matrix
            const bool keep = c.spmv_b3;
            c.spmv_b3 = false;
            build_sell(M, c);
            c.spmv_b3 = keep;
            return;
        }
        S = std::make_unique<DevSELL>();
    }
    S->nslices = sell_nslices(M.nrows);
    DBuf<int64_t> slen(S->nslices + 1);
    launch_sell_slice_len(M.nrows, M.rp.p, slen.p, c.st);
    S->sptr.alloc(S->nslices + 1);
    c.ensure_scan(S->nslices);
    exclusive_scan_i64(slen.p, S->sptr.p, S->nslices, c.scan_tmp.p, c.scan_tmp_bytes, c.st);
    HIPCHK(hipMemcpyAsync(&S->stored, S->sptr.p + S->nslices, sizeof(int64_t), hipMemcpyDeviceToHost, c.st));
    c.sync();
    S->val.alloc(std::max<int64_t>(S->stored, 2));
    S->col.alloc(std::max<int64_t>(S->stored, 1));
    launch_sell_fill(M.nrows, M.rp.p, M.ci.p, M.val.p, S->sptr.p, S->col.p, S->val.p, c.st);
    HIPCHK(hipGetLastError());
    c.sync();
    M.sell = std::move(S);
}

void classify_halo_slices(DevCSR &M, Ctx &c) {
    if (!M.halo || !M.sell || !M.sell->d16) return;
    DevSELL &S = *M.sell;
    const int64_t n = M.nrows, ns = S.nslices;
    DBuf<uint8_t> f(std::max<int64_t>(n, 1));
    launch_row_has_ghost(n, M.rp.p, M.ci.p, M.halo->nlocal, f.p, c.st);
    std::vector<uint8_t> hf(std::max<int64_t>(n, 1));
    std::vector<int64_t> sf(ns + 1);
    if (n) HIPCHK(hipMemcpyAsync(hf.data(), f.p, n, hipMemcpyDeviceToHost, c.st));
    HIPCHK(hipMemcpyAsync(sf.data(), S.sfirst.p, sizeof(int64_t) * (ns + 1), hipMemcpyDeviceToHost, c.st));
    c.sync();
    std::vector<int32_t> in, halo;
    for (int64_t s = 0; s < ns; ++s) {
        bool g = false;
        for (int64_t r = sf[s]; r < std::min<int64_t>(sf[s + 1], n) && !g; ++r) g = hf[r] != 0;
        (g ? halo : in).push_back((int32_t)s);
    }
    S.n_in = (int64_t)in.size();
    S.n_halo = (int64_t)halo.size();
    S.s_in.alloc(std::max<int64_t>(S.n_in, 1));
    S.s_halo.alloc(std::max<int64_t>(S.n_halo, 1));
    if (S.n_in) HIPCHK(hipMemcpyAsync(S.s_in.p, in.data(), sizeof(int32_t) * S.n_in, hipMemcpyHostToDevice, c.st));
    if (S.n_halo)
        HIPCHK(hipMemcpyAsync(S.s_halo.p, halo.data(), sizeof(int32_t) * S.n_halo, hipMemcpyHostToDevice, c.st));
    c.sync();
}

void build_low(DevSELL &S, Ctx &c, const std::string &who) {
    if (!S.d16)
        throw Error(who + ": the operator's SpMV layout is " + (S.col.p ? "int32 SELL-64" : "CSR") +
                    ", not SELL-64/D16 (no fp32 value stream for it)");
    if (S.b3_nslices)
        throw Error(who + ": the operator's SpMV layout has a SELL/B3 part (pls.spmv_b3): no fp32 value stream for it");
    if (S.val32.p) return;
    S.val32.alloc(std::max<int64_t>(S.stored, 4));
    DBuf<int32_t> over(1);
    HIPCHK(hipMemsetAsync(over.p, 0, sizeof(int32_t), c.st));
    launch_d16_round_values(S.stored, S.val.p, S.val32.p, over.p, c.st);
    HIPCHK(hipGetLastError());
    int32_t h = 0;
    HIPCHK(hipMemcpyAsync(&h, over.p, sizeof(int32_t), hipMemcpyDeviceToHost, c.st));
    c.sync();
    if (h) {
        S.val32.release();
        throw Error(who + ": a finite matrix value is infinite once rounded to fp32 (|a| > 3.4028235e38)");
    }
}

// the D16 launch of spmv(): over the fp64 value stream, or (low) over the fp32 one
static void d16_product(const DevCSR &M, const DevSELL &S, int64_t count, const int32_t *slist, const double *x,
                        double *y, double alpha, double beta, const double *z, const double *ghost, int64_t nlocal,
                        Ctx &c, bool low) {
    const int32_t *rm = S.nrows_mapped ? S.rowmap.p : nullptr;
    if (low)
        launch_d16_spmv(M.nrows, count, S.streams(), S.val32.p, x, y, alpha, beta, z, M.tag, ghost, nlocal,
                        c.d16_unroll_single, c.d16_xcd, c.st, slist, rm);
    else
        launch_d16_spmv(M.nrows, count, S.streams(), S.val.p, x, y, alpha, beta, z, M.tag, ghost, nlocal, c.d16_unroll,
                        c.d16_xcd, c.st, slist, rm);
}

void spmv(const DevCSR &M, const double *x, double *y, Ctx &c, double alpha, double beta, const double *z, bool low) {
    const double *ghost = nullptr;
    int64_t nlocal = M.ncols;
    if (low && !(M.sell && M.sell->has_low())) throw Error("spmv: the matrix has no fp32 value stream (build_low)");
    if (M.halo && c.halo_overlap && M.sell && M.sell->d16 && M.sell->n_halo + M.sell->n_in == M.sell->nslices) {
        // interior slices on the solver stream while the pack + exchange run on
        // the comm stream; the halo slices after the exchange.  Per-row sums
        // are the kernel's as in the plain path (same result bitwise).  NCCL
        // operations never overlap: the exchange waits for everything before
        // this product on the solver stream, and the solver stream waits for
        // the exchange before the halo slices (and any later collective).
        Halo &H = *M.halo;
        const DevSELL &S = *M.sell;
        if (!c.st_comm) {
            HIPCHK(hipStreamCreateWithFlags(&c.st_comm, hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&c.ev_x, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&c.ev_halo, hipEventDisableTiming));
        }
        HIPCHK(hipEventRecord(c.ev_x, c.st));
        HIPCHK(hipStreamWaitEvent(c.st_comm, c.ev_x, 0));
        d16_product(M, S, S.n_in, S.s_in.p, x, y, alpha, beta, z, nullptr, H.nlocal, c, low);
        launch_pack(H.nsend, H.send_idx.p, x, H.sendbuf.p, c.st_comm);
        c.comm->exchange_dev(H.sendbuf.p, H.scnt, H.soff, H.ghost.p, H.rcnt, H.roff, c.st_comm);
        HIPCHK(hipEventRecord(c.ev_halo, c.st_comm));
        HIPCHK(hipStreamWaitEvent(c.st, c.ev_halo, 0));
        d16_product(M, S, S.n_halo, S.s_halo.p, x, y, alpha, beta, z, H.ghost.p, H.nlocal, c, low);
        return;
    }
    if (M.halo) {
        Halo &H = *M.halo;
        launch_pack(H.nsend, H.send_idx.p, x, H.sendbuf.p, c.st);
        c.comm->exchange_dev(H.sendbuf.p, H.scnt, H.soff, H.ghost.p, H.rcnt, H.roff, c.st);
        ghost = H.ghost.p;
        nlocal = H.nlocal;
        if (!M.sell) throw Error("distributed matrix without SELL layout");
    }
    if (M.sell && M.sell->d16) {
        DevSELL &S = *M.sell;
        if (S.nperm) {  // RCM-relabelled columns: x in that order first (the context's scratch)
            if (c.rcm_x.n < (size_t)S.nperm) {  // a context other than the one the layout was built on
                HIPCHK(hipStreamSynchronize(c.st));
                c.rcm_x.alloc(S.nperm);
            }
            launch_gather_i32(S.nperm, S.xperm.p, x, c.rcm_x.p, c.st);
            x = c.rcm_x.p;
        }
        if (S.b3_nslices)
            launch_b3_spmv(S.b3_nslices, S.b3_ntrip, S.b3ptr.p, S.b3map.p, S.b3col.p, S.b3val.p, x, y, alpha, beta, z,
                           M.tag, c.st);
        d16_product(M, S, S.nslices, nullptr, x, y, alpha, beta, z, ghost, nlocal, c, low);
        return;
    }
    if (M.sell) {
        launch_sell_spmv(M.nrows, M.sell->sptr.p, M.sell->col.p, M.sell->val.p, x, y, alpha, beta, z, M.tag, ghost,
                         nlocal, c.st);
        return;
    }
    launch_spmv(M.nrows, M.nnz, M.rp.p, M.ci.p, M.val.p, x, y, alpha, beta, z, c.st);
}

// the slices slist[0 .. count) of a D16 layout (rows of those slices only; the
// per-row sums are spmv()'s): the 2-way PC's pressure-first pipeline
bool plain_d16(const DevCSR &M) {
    return M.sell && M.sell->d16 && !M.halo && !M.sell->nperm && !M.sell->b3_nslices && !M.sell->nrows_mapped;
}

void spmv_slices(const DevCSR &M, const double *x, double *y, Ctx &c, double alpha, double beta, const double *z,
                 const int32_t *slist, int64_t count, size_t lds_reserve, double *qout, const D16Wide &W) {
    if (!plain_d16(M)) throw Error("spmv_slices: plain D16 layouts only");
    if (qout && M.tag) throw Error("spmv_slices: raw row sums are stored for inner matrices only");
    const DevSELL &S = *M.sell;
    launch_d16_spmv(M.nrows, count, S.streams(), S.val.p, x, y, alpha, beta, z, M.tag, nullptr, M.ncols, c.d16_unroll,
                    c.d16_xcd, c.st, slist, nullptr, lds_reserve, qout ? D16_AUX_STORE : D16_AUX_NONE, qout, W);
}

void spmv_store_sums(const DevCSR &M, const double *x, double *y, Ctx &c, double alpha, double beta, const double *z,
                     double *qout, const D16Wide &W) {
    if (!plain_d16(M) || M.tag) throw Error("spmv_store_sums: plain D16 layouts of inner matrices only");
    const DevSELL &S = *M.sell;
    launch_d16_spmv(M.nrows, S.nslices, S.streams(), S.val.p, x, y, alpha, beta, z, 0, nullptr, M.ncols, c.d16_unroll,
                    c.d16_xcd, c.st, nullptr, nullptr, 0, D16_AUX_STORE, qout, W);
}

// ======================================================= coupling reuse ===
bool build_coupling(const DevCSR &A, int64_t ns, const DevCSR &M, Coupling &R, Ctx &c) {
    R.eligible = false;
    R.fresh_for = nullptr;
    R.reduced = DevSELL();
    R.reuse_rows = 0;
    R.wide_rows = R.wlo = R.whi = 0;
    R.wlpr = 0;
    R.reuse.clear();
    const int64_t n = A.nrows;
    if (!plain_d16(A) || !plain_d16(M)) {
        R.why = "the outer operator's or the coupling block's layout is not plain D16";
        return false;
    }
    if (M.nrows != n - ns || M.ncols != ns || A.ncols != n) {
        R.why = "the coupling block is not rows [ns, n) x columns [0, ns) of the outer operator";
        return false;
    }
    // reuse rows: lane-per-row in A's plan and in M's (1), and with pls.reuse_wide the rows that
    // the same lpr > 1 lanes serve in both (2: their sums are kept per lane, Coupling::qw)
    const DevSELL &SA = *A.sell, &SM = *M.sell;
    std::vector<int64_t> sfa(SA.nslices + 1), sfm(SM.nslices + 1);
    std::vector<int32_t> lpa(SA.nslices), lpm(SM.nslices);
    HIPCHK(hipMemcpyAsync(sfa.data(), SA.sfirst.p, sizeof(int64_t) * sfa.size(), hipMemcpyDeviceToHost, c.st));
    HIPCHK(hipMemcpyAsync(lpa.data(), SA.slpr.p, sizeof(int32_t) * lpa.size(), hipMemcpyDeviceToHost, c.st));
    HIPCHK(hipMemcpyAsync(sfm.data(), SM.sfirst.p, sizeof(int64_t) * sfm.size(), hipMemcpyDeviceToHost, c.st));
    HIPCHK(hipMemcpyAsync(lpm.data(), SM.slpr.p, sizeof(int32_t) * lpm.size(), hipMemcpyDeviceToHost, c.st));
    c.sync();
    std::vector<uint8_t> reuse(n, 0);
    std::vector<int32_t> lanes(n, 0);  // lanes per row in M's plan (0: not an fp row)
    for (int64_t s = 0; s < SM.nslices; ++s)
        for (int64_t r = sfm[s]; r < std::min(sfm[s + 1], M.nrows); ++r) lanes[ns + r] = lpm[s];
    bool wide_ok = c.reuse_wide != 0;
    int64_t wlo = n, whi = 0;
    for (int64_t s = 0; s < SA.nslices; ++s)
        for (int64_t r = sfa[s]; r < std::min(sfa[s + 1], n); ++r) {
            if (lanes[r] == 1 && lpa[s] == 1) {
                reuse[r] = 1;
                R.reuse_rows++;
            } else if (wide_ok && lanes[r] > 1 && lanes[r] == lpa[s]) {
                if (R.wlpr == 0) R.wlpr = lpa[s];
                if (lpa[s] != R.wlpr) {  // (plain plans know one wide lpr; qw is indexed with one)
                    wide_ok = false;
                    continue;
                }
                reuse[r] = 2;
                wlo = std::min(wlo, r);
                whi = std::max(whi, r + 1);
                R.wide_rows++;
            }
        }
    if (!wide_ok && R.wide_rows > 0) {
        for (uint8_t &f : reuse) f = f == 1;
        R.wide_rows = 0;
    }
    if (R.wide_rows == 0) R.wlpr = 0;
    else R.wlo = wlo, R.whi = whi;
    DBuf<uint8_t> dreuse(n);
    DBuf<int64_t> rstart(n);
    DBuf<int32_t> differs(1);
    HIPCHK(hipMemcpyAsync(dreuse.p, reuse.data(), n, hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemsetAsync(differs.p, 0, sizeof(int32_t), c.st));
    launch_coupling_rows(n, ns, A.rp.p, A.ci.p, A.val.p, M.rp.p, M.ci.p, M.val.p, dreuse.p, rstart.p, differs.p, c.st);
    HIPCHK(hipGetLastError());
    int32_t diff = 0;
    HIPCHK(hipMemcpyAsync(&diff, differs.p, sizeof(int32_t), hipMemcpyDeviceToHost, c.st));
    c.sync();
    if (diff) {
        R.why = "the preconditioner's coupling block differs from the outer operator's";
        return false;
    }
    if (R.reuse_rows + R.wide_rows == 0) {
        R.why = "no row is lane-per-row in both layouts";
        R.wide_rows = 0;
        return false;
    }
    // A' on A's own slice plan: a reuse row keeps its lanes per row whatever is left of it, and
    // a wide one every remaining entry on the lane it has in A (the phase rule of k_d16_fill)
    if (!d16_from_plan(A, R.reduced, sfa, lpa, {}, rstart.p, c)) {
        R.why = "the reduced layout does not fit D16";
        R.reduced = DevSELL();
        R.wide_rows = 0;
        return false;
    }
    if (R.q.n != (size_t)n) R.q.alloc(n);
    HIPCHK(hipMemsetAsync(R.q.p, 0, sizeof(double) * n, c.st));
    const size_t nw = (size_t)((R.whi - R.wlo) * R.wlpr);
    if (nw == 0) R.qw.release();
    else if (R.qw.n != nw) R.qw.alloc(nw);
    if (nw) HIPCHK(hipMemsetAsync(R.qw.p, 0, sizeof(double) * nw, c.st));
    c.sync();
    R.why.clear();
    for (uint8_t &f : reuse) f = f != 0;
    R.reuse = std::move(reuse);
    R.eligible = true;
    return true;
}

// ============================================================== options ===
void Options::parse(const char *text) {
    if (!text) return;
    std::istringstream is(text);
    std::string line;
    while (std::getline(is, line)) {
        // trim
        size_t a = line.find_first_not_of(" \t\r");
        if (a == std::string::npos) continue;
        size_t b = line.find_last_not_of(" \t\r");
        line = line.substr(a, b - a + 1);
        size_t sp = line.find(' ');
        std::string k = line.substr(0, sp), v;
        if (sp != std::string::npos) {
            size_t vs = line.find_last_of(' ');
            v = line.substr(vs + 1);
        }
        while (!k.empty() && k[0] == '-') k.erase(0, 1);
        kv[k] = v;
    }
}
std::string Options::str(const std::string &k, const std::string &d) const {
    auto it = kv.find(k);
    return it == kv.end() || it->second.empty() ? d : it->second;
}
double Options::num(const std::string &k, double d) const {
    auto it = kv.find(k);
    if (it == kv.end() || it->second.empty()) return d;
    try { return std::stod(it->second); } catch (...) { throw Error("option " + k + ": not a number: " + it->second); }
}
int64_t Options::integer(const std::string &k, int64_t d) const {
    auto it = kv.find(k);
    if (it == kv.end() || it->second.empty()) return d;
    try { return (int64_t)std::stoll(it->second); } catch (...) { throw Error("option " + k + ": not an integer: " + it->second); }
}
bool Options::flag(const std::string &k, bool d) const {
    auto it = kv.find(k);
    if (it == kv.end()) return d;
    const std::string &v = it->second;
    if (v.empty() || v == "1" || v == "true" || v == "yes" || v == "on" || v == "True" || v == "TRUE") return true;
    return false;
}

// =============================================================== timers ===
Timers::~Timers() {
    for (hipEvent_t e : pool) (void)hipEventDestroy(e);
}
hipEvent_t Timers::ev() {
    if (next == pool.size()) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        pool.push_back(e);
    }
    return pool[next++];
}
void Timers::begin(int cat) {
    if (!enabled) return;
    hipEvent_t e = ev();
    HIPCHK(hipEventRecord(e, st));
    open_stack.push_back(cat);
    open_ev.push_back(e);
}
void Timers::end(int cat) {
    if (!enabled) return;
    if (open_stack.empty() || open_stack.back() != cat) throw Error("timer nesting error");
    hipEvent_t e = ev();
    HIPCHK(hipEventRecord(e, st));
    pending.push_back({cat, open_ev.back(), e});
    open_stack.pop_back();
    open_ev.pop_back();
}
void Timers::flush() {
    for (auto &p : pending) {
        float ms = 0.f;
        HIPCHK(hipEventSynchronize(p.b));
        HIPCHK(hipEventElapsedTime(&ms, p.a, p.b));
        acc[p.cat] += ms * 1e-3;
    }
    pending.clear();
    if (open_stack.empty()) next = 0;
    ++flushes;
}
hipEvent_t Timers::mark(hipStream_t s) {
    if (!enabled) return nullptr;
    hipEvent_t e = ev();
    HIPCHK(hipEventRecord(e, s));
    return e;
}

// The full product: over the fp64 values, or (low) over the fp32 stream of the layout.
void MatOp::product(const double *x, double *y, Ctx &c, bool lo) {
    if (lo) {
        if (!low) throw Error("MatOp::apply_low: the low-precision operator was not asked for");
        // (a new layout: the matrix changed)
        if (!M->sell || !M->sell->has_low()) enable_low(c, "pls_gmres_operator single");
    } else if (!M->sell) {
        build_sell(const_cast<DevCSR &>(*M), c);
    }
    if (timers) timers->begin(T_SPMV);
    spmv(*M, x, y, c, 1.0, 0.0, nullptr, lo);
    if (timers) { timers->end(T_SPMV); timers->spmv_calls++; }
    if (coupling) coupling->n_full++;
}

// The reduced product where the PC's coupling sums belong to x, else the full one.  T_SPMV
// gets the reduced launch and the coupling launches that produced q (together they stream
// the whole of A once), as one call.  low: over the fp32 stream of A'; the reuse rows start
// from the PC's fp64 raw sums, so their coupling entries enter with their fp64 values.
void MatOp::product_after(const PC &pc, const double *x, double *y, Ctx &c, bool lo) {
    Coupling *R = coupling;
    if (!R || !R->eligible || pc.coupling_product() != R || R->fresh_for != x) return product(x, y, c, lo);
    if (lo) {
        if (!low) throw Error("MatOp::apply_after_low: the low-precision operator was not asked for");
        if (!R->reduced.has_low()) build_low(R->reduced, c, "pls_gmres_operator single (reduced outer operator)");
    }
    R->fresh_for = nullptr;
    const DevSELL &S = R->reduced;
    if (timers) timers->begin(T_SPMV);
    if (lo)
        launch_d16_spmv(M->nrows, S.nslices, S.streams(), S.val32.p, x, y, 1.0, 0.0, nullptr, 1, nullptr, M->ncols,
                        c.d16_unroll_single, c.d16_xcd, c.st, nullptr, nullptr, 0, R->q.p, R->wide(0));
    else
        launch_d16_spmv(M->nrows, S.nslices, S.streams(), S.val.p, x, y, 1.0, 0.0, nullptr, 1, nullptr, M->ncols,
                        c.d16_unroll, c.d16_xcd, c.st, nullptr, nullptr, 0, D16_AUX_INIT, R->q.p, R->wide(0));
    if (timers) {
        timers->end(T_SPMV);
        timers->spmv_calls++;
        if (R->spans_flush == timers->flushes)
            for (const Timers::Span &sp : R->spans) timers->add(T_SPMV, sp);
    }
    R->spans.clear();
    R->n_reduced++;
}
void MatOp::apply(const double *x, double *y, Ctx &c) { product(x, y, c, false); }
void MatOp::apply_after(const PC &pc, const double *x, double *y, Ctx &c) { product_after(pc, x, y, c, false); }
void MatOp::apply_low(const double *x, double *y, Ctx &c) { product(x, y, c, true); }
void MatOp::apply_after_low(const PC &pc, const double *x, double *y, Ctx &c) { product_after(pc, x, y, c, true); }

// ---- the low-precision operator (compressed-operator GMRES)
void Op::apply_low(const double *, double *, Ctx &) {
    throw Error("this operator has no low-precision copy (pls_gmres_operator single needs a stored matrix)");
}
void Op::apply_after_low(const PC &, const double *x, double *y, Ctx &c) { apply_low(x, y, c); }

void MatOp::enable_low(Ctx &c, const std::string &who) {
    low = true;
    if (!M->sell) build_sell(const_cast<DevCSR &>(*M), c);
    if (!M->sell) throw Error(who + ": the operator has no rows");
    build_low(*M->sell, c, who);
}
int64_t MatOp::low_bytes() const {
    return (M->sell ? M->sell->low_stream_bytes() : 0) +
           (coupling && coupling->eligible ? coupling->reduced.low_stream_bytes() : 0);
}

void Op::residual(const double *x, const double *b, double *r, Ctx &c) {
    apply(x, r, c);
    launch_waxpby(n, 1.0, b, -1.0, r, r, c.st);
}
void MatOp::residual(const double *x, const double *b, double *r, Ctx &c) {
    if (!M->sell) build_sell(const_cast<DevCSR &>(*M), c);
    if (timers) timers->begin(T_SPMV);
    spmv(*M, x, r, c, -1.0, 1.0, b);
    if (timers) { timers->end(T_SPMV); timers->spmv_calls++; }
    if (coupling) coupling->n_full++;
}

// ====================================================== preconditioners ===
void PCNone::apply(const double *x, double *y, Ctx &c) {
    if (x != y) launch_copy(n, x, y, c.st);
}

PCJacobi::PCJacobi(const DevCSR &M, Ctx &c) {
    type = "jacobi";
    n = M.nrows;
    const HostCSR H = download(M, c);  // diag from a host copy (setup only)
    std::vector<double> d(n, 1.0);
    for (int64_t i = 0; i < n; ++i) {
        double di = 0.0;
        for (int64_t k = H.rp[i]; k < H.rp[i + 1]; ++k)
            if (H.ci[k] == i) { di = H.v[k]; break; }
        d[i] = (di == 0.0) ? 1.0 : 1.0 / di;
    }
    dinv.alloc(std::max<int64_t>(n, 1));
    HIPCHK(hipMemcpyAsync(dinv.p, d.data(), sizeof(double) * n, hipMemcpyHostToDevice, c.st));
    c.sync();
}
void PCJacobi::apply(const double *x, double *y, Ctx &c) { launch_pointwise_mult(n, x, dinv.p, y, c.st); }

PCDenseLU::PCDenseLU(const DevCSR &M, Ctx &c, double u) {
    type = "lu";
    n = M.nrows;
    if (M.ncols != n) throw Error("lu: block is not square");
    ld = std::max<int64_t>(64, (n + 63) / 64 * 64);
    inv.alloc(ld * ld);
    launch_dense_from_csr(n, ld, M.rp.p, M.ci.p, M.val.p, inv.p, c.st);
    DBuf<double> D(64 * 64), P;
    DBuf<int32_t> fail(1), st;
    HIPCHK(hipMemsetAsync(fail.p, 0, sizeof(int32_t), c.st));
    if (u > 0.0 && n > 1) {  // MUMPS-style threshold partial pivoting over every remaining row
        std::vector<int32_t> id(n);
        std::iota(id.begin(), id.end(), 0);
        rowperm.alloc(n);
        HIPCHK(hipMemcpyAsync(rowperm.p, id.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, c.st));
        P.alloc((size_t)n * 64 + panel_fast_doubles());
        st.alloc(3);
        HIPCHK(hipMemsetAsync(st.p, 0, sizeof(int32_t) * 3, c.st));
        c.sync();  // (id)
    }
    launch_dense_invert(ld, inv.p, D.p, fail.p, c.st, n, P.p, rowperm.p, st.p, rowperm.p ? u : 0.0);
    HIPCHK(hipGetLastError());
    int32_t hfail = 0;
    HIPCHK(hipMemcpyAsync(&hfail, fail.p, sizeof(int32_t), hipMemcpyDeviceToHost, c.st));
    if (st.p) HIPCHK(hipMemcpyAsync(piv_stats, st.p, sizeof(int32_t) * 3, hipMemcpyDeviceToHost, c.st));
    c.sync();
    if (hfail) throw Error("LU: zero pivot (PETSc: MAT_FACTOR_NUMERIC_ZEROPIVOT)");
}

void PCDenseLU::apply(const double *x, double *y, Ctx &c) {
    launch_dense_gemv(n, ld, inv.p, x, y, c.st, rowperm.p);
}

void csr_bandwidths(const DevCSR &M, int64_t &kl, int64_t &ku, Ctx &c) {
    const int64_t n = M.nrows;
    kl = ku = 0;
    if (n == 0) return;
    std::vector<int64_t> rp(n + 1);
    std::vector<int32_t> ci(M.nnz);
    HIPCHK(hipMemcpyAsync(rp.data(), M.rp.p, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, c.st));
    if (M.nnz) HIPCHK(hipMemcpyAsync(ci.data(), M.ci.p, sizeof(int32_t) * M.nnz, hipMemcpyDeviceToHost, c.st));
    c.sync();
    for (int64_t i = 0; i < n; ++i) {
        if (rp[i + 1] == rp[i]) continue;
        kl = std::max<int64_t>(kl, i - ci[rp[i]]);
        ku = std::max<int64_t>(ku, ci[rp[i + 1] - 1] - i);
    }
}

PCBandLU::PCBandLU(const DevCSR &M, int64_t kl, int64_t ku, Ctx &c, int64_t spike_plen) {
    type = "lu";
    n = M.nrows;
    if (M.ncols != n) throw Error("lu: block is not square");
    nb = (n + 63) / 64;
    bl = (kl + 63) / 64;
    bu = (ku + 63) / 64;
    const int64_t W = bl + bu + 1;
    T.alloc((size_t)(nb * W) * 4096);
    Dl.alloc((size_t)nb * 4096);
    Du.alloc((size_t)nb * 4096);
    Gl.alloc((size_t)nb * 4096);
    Gu.alloc((size_t)nb * 4096);
    t.alloc(std::max<int64_t>(n, 1));
    G.alloc((size_t)std::max<int64_t>(nb, 1) * 128);
    fail.alloc(1);
    ticket.alloc(1);
    HIPCHK(hipMemsetAsync(G.p, 0, sizeof(uint64_t) * G.n, c.st));
    HIPCHK(hipMemsetAsync(fail.p, 0, sizeof(int32_t), c.st));
    HIPCHK(hipMemsetAsync(ticket.p, 0, sizeof(uint64_t), c.st));
    launch_band_from_csr(n, nb, bl, bu, M.rp.p, M.ci.p, M.val.p, T.p, c.st);
    launch_band_factor(nb, bl, bu, T.p, Dl.p, Du.p, Gl.p, Gu.p, fail.p, c.st);
    HIPCHK(hipGetLastError());
    if (check_fail(c)) throw Error("LU: zero pivot (PETSc: MAT_FACTOR_NUMERIC_ZEROPIVOT)");
    // SPIKE partitions (band.hip): ~16 concurrent chains per triangle (footing
    // N=128 Schur block, 2,064 tile rows: 16 -> 201 it/s, 32 -> 195, 64 -> 194)
    const int64_t bwmax = std::max<int64_t>(std::max(bl, bu), 1);
    int64_t pl = spike_plen < 0 ? std::max(bwmax, (nb + 15) / 16) : spike_plen;
    if (pl > 0) {
        pl = std::max(pl, bwmax);
        pl += pl & 1;  // whole super-rows
    }
    if (pl > 0 && pl < nb && (bl > 0 || bu > 0)) {
        plen = pl;
        spike_tmp.alloc((size_t)std::max<int64_t>(spike_scratch_doubles(bwmax), 1));
        if (bl > 0) {
            Wl.alloc((size_t)(nb * bl) * 4096);
            launch_spike_setup(nb, bl, bu, 0, plen, T.p, Dl.p, Wl.p, c.st);
        }
        if (bu > 0) {
            Wu.alloc((size_t)(nb * bu) * 4096);
            launch_spike_setup(nb, bl, bu, 1, plen, T.p, Du.p, Wu.p, c.st);
        }
        HIPCHK(hipGetLastError());
        c.sync();
    }
}

int32_t PCBandLU::check_fail(Ctx &c) {
    int32_t h = 0;
    HIPCHK(hipMemcpyAsync(&h, fail.p, sizeof(int32_t), hipMemcpyDeviceToHost, c.st));
    c.sync();
    return h;
}

void PCBandLU::apply(const double *x, double *y, Ctx &c) {
    // epochs 2s+1, 2s+2 (never 0); each sweep draws band_sweep_tickets(nb) tickets
    const uint64_t nt = (uint64_t)band_sweep_tickets(nb);
    launch_band_sweep(n, nb, bl, bu, T.p, Dl.p, Gl.p, x, t.p, G.p, ticket.p, sweeps * nt, (uint32_t)(sweeps + 1), 0,
                      fail.p, c.st, plen);
    ++sweeps;
    if (plen > 0 && bl > 0) launch_spike_apply(n, nb, bl, 0, plen, Wl.p, t.p, spike_tmp.p, c.st);
    launch_band_sweep(n, nb, bl, bu, T.p, Du.p, Gu.p, t.p, y, G.p, ticket.p, sweeps * nt, (uint32_t)(sweeps + 1), 1,
                      fail.p, c.st, plen);
    ++sweeps;
    if (plen > 0 && bu > 0) launch_spike_apply(n, nb, bu, 1, plen, Wu.p, y, spike_tmp.p, c.st);
}

std::unique_ptr<PC> make_lu(const DevCSR &M, const Options &o, Ctx &c) {
    const std::string path = o.str("pls.lu_path", "auto");
    if (path != "auto" && path != "dense" && path != "sparse" && path != "band" && path != "envelope")
        throw Error("pls.lu_path " + path + " (auto, dense, sparse, band, envelope)");
    if (path == "dense" || (path == "auto" && M.nrows <= o.integer("pls.lu_dense_max", 32768))) {
        auto pc = std::make_unique<PCDenseLU>(M, c, o.num("pls.lu_pivot_threshold", 0.01));
        if (o.flag("pls.lu_view", false))
            fprintf(stderr, "[dense lu] n %lld: threshold pivoting u = %g: %d rows exchanged, %d pivots below u x "
                    "column max (delayed by MUMPS), %d zero columns\n", (long long)M.nrows,
                    o.num("pls.lu_pivot_threshold", 0.01), pc->piv_stats[0], pc->piv_stats[1], pc->piv_stats[2]);
        return pc;
    }
    // larger blocks: nested dissection + multifrontal LU (the MUMPS stand-in)
    if (path == "sparse" || path == "auto") return make_sparse_lu(M, o, c);
    if (path == "band") {
        int64_t kl = 0, ku = 0;
        csr_bandwidths(M, kl, ku, c);
        // band tiles + the SPIKE spikes (nb x (bl + bu) tiles): ~2x the band (288 GB per
        // MI355X: the 2-D footing N=128 Schur block's 95 GB band + 95 GB of spikes fit).
        // There is no cap and no option that sets one: an allocation that fails is reported
        auto pc = std::make_unique<PCBandLU>(M, kl, ku, c, o.integer("pls.band_spike_plen", -1));
        if (o.flag("pls.lu_view", false))
            fprintf(stderr, "[band lu] n %lld: tile rows %lld, bl %lld, bu %lld, spike plen %lld, partitions %lld\n",
                    (long long)M.nrows, (long long)pc->nb, (long long)pc->bl, (long long)pc->bu, (long long)pc->plen,
                    (long long)(pc->plen > 0 ? (pc->nb + pc->plen - 1) / pc->plen : 1));
        return pc;
    }
    // the envelope (profile) LU: exact, level-scheduled
    PCILU::Config cfg = PCILU::Config::from_options(o, "", 0);
    cfg.exact_lu = true;
    return std::make_unique<PCILU>(M, 1, c, cfg);
}

// Gather a sharded diagonal block -- every rank's MPIAIJ rows with
// block-global columns (Halo::l2g) -- into the global host CSR, in the block's
// global order, on every rank (host allgather, setup only).  srcslot[g]: where
// global row g sits in a padded allgather of the ranks' rows (q * maxloc + i);
// rank_rows: the ranks' row counts when they own contiguous ranges in rank
// order (every single-field block, every caller-assembled one), else empty.
HostCSR gather_block(const DevCSR &M, Ctx &c, const std::string &prefix, std::vector<int64_t> &srcslot,
                     int64_t &maxloc, std::vector<int64_t> &rank_rows) {
    const int64_t nloc = M.nrows;
    const Halo &H = *M.halo;
    if ((int64_t)H.l2g.size() < M.ncols || H.nlocal != M.nrows)
        throw Error("redundant PC (prefix " + prefix + "): block is not a diagonal block of the sharded system");
    Comm &cm = *c.comm;
    const int G = cm.size;
    const HostCSR L = download(M, c);
    std::vector<int64_t> cnt{nloc, (int64_t)L.ci.size()}, all(2 * G);
    cm.allgather_host(cnt.data(), sizeof(int64_t) * 2, all.data());
    int64_t maxnnz = 0, N = 0;
    maxloc = 0;
    for (int q = 0; q < G; ++q) {
        maxloc = std::max(maxloc, all[2 * q]);
        maxnnz = std::max(maxnnz, all[2 * q + 1]);
        N += all[2 * q];
    }
    // message: rows (global ids), row lengths, columns (global), values -- padded to the largest rank's
    const int64_t words = 2 * maxloc + 2 * maxnnz;
    std::vector<int64_t> msg(words, 0), recv((size_t)words * G);
    for (int64_t i = 0; i < nloc; ++i) {
        msg[i] = H.l2g[i];
        msg[maxloc + i] = L.rp[i + 1] - L.rp[i];
    }
    for (size_t k = 0; k < L.ci.size(); ++k) {
        msg[2 * maxloc + k] = H.l2g[L.ci[k]];
        std::memcpy(&msg[2 * maxloc + maxnnz + k], &L.v[k], sizeof(double));
    }
    cm.allgather_host(msg.data(), sizeof(int64_t) * words, recv.data());
    // global CSR: row g from its owner, columns sorted
    std::vector<int64_t> rowlen(N, -1);
    srcslot.assign(N, -1);
    for (int q = 0; q < G; ++q) {
        const int64_t *m = recv.data() + (size_t)words * q;
        for (int64_t i = 0; i < all[2 * q]; ++i) {
            const int64_t g = m[i];
            if (g < 0 || g >= N || rowlen[g] >= 0) throw Error("redundant PC: inconsistent row ownership");
            rowlen[g] = m[maxloc + i];
            srcslot[g] = q * maxloc + i;
        }
    }
    HostCSR Gh;
    Gh.nrows = Gh.ncols = N;
    Gh.rp.assign(N + 1, 0);
    for (int64_t g = 0; g < N; ++g) Gh.rp[g + 1] = Gh.rp[g] + rowlen[g];
    Gh.ci.resize(Gh.rp[N]);
    Gh.v.resize(Gh.rp[N]);
    std::vector<std::pair<int64_t, double>> row;
    for (int q = 0; q < G; ++q) {
        const int64_t *m = recv.data() + (size_t)words * q;
        int64_t k = 0;
        for (int64_t i = 0; i < all[2 * q]; ++i) {
            const int64_t g = m[i], len = m[maxloc + i];
            row.resize(len);
            for (int64_t e = 0; e < len; ++e, ++k) {
                double v;
                std::memcpy(&v, &m[2 * maxloc + maxnnz + k], sizeof(double));
                row[e] = {m[2 * maxloc + k], v};
            }
            std::sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
            for (int64_t e = 0; e < len; ++e) {
                Gh.ci[Gh.rp[g] + e] = (int32_t)row[e].first;
                Gh.v[Gh.rp[g] + e] = row[e].second;
            }
        }
    }
    rank_rows.clear();
    bool contiguous = true;
    int64_t start = 0;
    for (int q = 0; q < G && contiguous; ++q) {
        const int64_t *m = recv.data() + (size_t)words * q;
        for (int64_t i = 0; i < all[2 * q]; ++i)
            if (m[i] != start + i) contiguous = false;
        start += all[2 * q];
    }
    if (contiguous)
        for (int q = 0; q < G; ++q) rank_rows.push_back(all[2 * q]);
    return Gh;
}

// Local rows L (columns: global indices of a column space owned in contiguous
// rank ranges cst[q] .. cst[q + 1]) -> a distributed DevCSR: owned columns ->
// local [0, nlocal), referenced others -> ghosts nlocal + k in global order
// (= owner-major), the halo plan by one alltoallv of index lists, entries of a
// row sorted by local column, the SpMV layout built.  Every rank calls it.
void upload_dist(const HostCSR &L, const std::vector<int64_t> &cst, DevCSR &M, Ctx &c) {
    Comm &cm = *c.comm;
    const int G = cm.size, r = cm.rank;
    if ((int)cst.size() != G + 1) throw Error("upload_dist: one column range per rank expected");
    const int64_t c0 = cst[r], nlocal = cst[r + 1] - cst[r];
    std::vector<int64_t> gh;
    for (int32_t j : L.ci)
        if (j < c0 || j >= c0 + nlocal) gh.push_back(j);
    std::sort(gh.begin(), gh.end());
    gh.erase(std::unique(gh.begin(), gh.end()), gh.end());
    auto H = std::make_shared<Halo>();
    H->nlocal = nlocal;
    H->nghost = (int64_t)gh.size();
    std::vector<std::vector<int64_t>> need(G), asked;
    H->rcnt.assign(G, 0);
    H->roff.assign(G, 0);
    {
        size_t k = 0;
        for (int q = 0; q < G; ++q) {
            H->roff[q] = (int64_t)k;
            while (k < gh.size() && gh[k] < cst[q + 1]) need[q].push_back(gh[k++]);
            H->rcnt[q] = (int64_t)need[q].size();
        }
    }
    cm.alltoallv_i64(need, asked);
    std::vector<int32_t> sidx;
    H->scnt.assign(G, 0);
    H->soff.assign(G, 0);
    for (int q = 0; q < G; ++q) {
        H->soff[q] = (int64_t)sidx.size();
        for (int64_t g : asked[q]) {
            if (g < c0 || g >= c0 + nlocal) throw Error("halo plan: peer asked for a column this rank does not own");
            sidx.push_back((int32_t)(g - c0));
        }
        H->scnt[q] = (int64_t)asked[q].size();
    }
    H->nsend = (int64_t)sidx.size();
    H->send_idx.alloc(std::max<int64_t>(H->nsend, 1));
    if (H->nsend) HIPCHK(hipMemcpyAsync(H->send_idx.p, sidx.data(), sizeof(int32_t) * H->nsend, hipMemcpyHostToDevice, c.st));
    H->sendbuf.alloc(std::max<int64_t>(H->nsend, 1));
    H->ghost.alloc(std::max<int64_t>(H->nghost, 1));
    H->l2g.resize(nlocal + gh.size());
    for (int64_t i = 0; i < nlocal; ++i) H->l2g[i] = c0 + i;
    for (size_t k = 0; k < gh.size(); ++k) H->l2g[nlocal + k] = gh[k];
    HostCSR T;
    T.nrows = L.nrows;
    T.ncols = nlocal + (int64_t)gh.size();
    T.rp.assign(1, 0);
    std::vector<std::pair<int32_t, double>> row;
    for (int64_t i = 0; i < L.nrows; ++i) {
        row.clear();
        for (int64_t k = L.rp[i]; k < L.rp[i + 1]; ++k) {
            const int64_t j = L.ci[k];
            const int32_t lj = (j >= c0 && j < c0 + nlocal)
                                   ? (int32_t)(j - c0)
                                   : (int32_t)(nlocal + (std::lower_bound(gh.begin(), gh.end(), j) - gh.begin()));
            row.push_back({lj, L.v[k]});
        }
        std::sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        for (auto &e : row) {
            T.ci.push_back(e.first);
            T.v.push_back(e.second);
        }
        T.rp.push_back((int64_t)T.ci.size());
    }
    upload(T, M, c);
    M.ncols = T.ncols;
    M.halo = H;
    M.sell.reset();
    build_sell(M, c);
    c.sync();
}

// a single-rank context carrying c's layout options
std::unique_ptr<Ctx> layout_ctx(const Ctx &c) {
    auto self = std::make_unique<Ctx>();
    self->sell_d16 = c.sell_d16;
    self->d16_wide_lpr = c.d16_wide_lpr;
    self->d16_unroll = c.d16_unroll;
    self->d16_xcd = c.d16_xcd;
    self->d16_share = c.d16_share;
    self->d16_share_min_bytes = c.d16_share_min_bytes;
    self->reuse_wide = c.reuse_wide;
    self->d16_unroll_single = c.d16_unroll_single;
    self->d16_segs = c.d16_segs;
    self->d16_sigma = c.d16_sigma;
    self->d16_sigma_pad = c.d16_sigma_pad;
    self->d16_sorted_lpr = c.d16_sorted_lpr;
    self->spmv_b3 = c.spmv_b3;
    self->spmv_rcm = c.spmv_rcm;
    self->sweep_chain = c.sweep_chain;
    self->sweep_window = c.sweep_window;
    self->window_depth = c.window_depth;
    self->window_ring = c.window_ring;
    self->window_mixed = c.window_mixed;
    self->window_kpw = c.window_kpw;
    self->amg_csr_below = c.amg_csr_below;
    return self;
}

// PETSc PCREDUNDANT semantics for PCs that act on a whole parallel block
// (ILU(0), LU, classical / smoothed-aggregation AMG) when the block is
// sharded over G ranks: every rank gathers the block (its MPIAIJ rows with
// block-global column indices, Halo::l2g) into the global matrix in the
// block's global order, builds the PC on it with a single-rank context, and
// per application allgathers x, applies the PC redundantly and keeps its own
// rows.  The result is the one-rank PC's result on the same block, bitwise.
struct PCRedundant : PC {
    std::unique_ptr<Ctx> self;  // own stream, single-rank communicator
    DevCSR Gm;                  // the gathered global block
    std::unique_ptr<PC> inner;
    int64_t nloc = 0, maxloc = 0, N = 0;
    DBuf<int64_t> src, mine;    // xg[g] = gathered[src[g]];  y[i] = yg[mine[i]]
    DBuf<double> sendbuf, gath, xg, yg;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;

    PCRedundant(const std::string &t, const DevCSR &M, Ctx &c,
                const std::function<std::unique_ptr<PC>(const DevCSR &, Ctx &)> &factory, const std::string &prefix,
                GatheredBlock *pre) {
        type = t;
        n = nloc = M.nrows;
        const Halo &H = *M.halo;
        const int G = c.comm->size;
        GatheredBlock own;
        if (!pre) {
            own.G = gather_block(M, c, prefix, own.srcslot, own.maxloc, own.rank_rows);
            pre = &own;
        }
        const HostCSR &Gh = pre->G;
        const std::vector<int64_t> &srcslot = pre->srcslot, &rank_rows = pre->rank_rows;
        maxloc = pre->maxloc;
        N = Gh.nrows;
        self = layout_ctx(c);
        // the ranks' rows: contiguous ranges in rank order -> the inner PC may restate
        // how the reference's PC runs over G ranks (classical AMG: hypre's per-rank
        // HMIS and smoother)
        self->rank_rows = rank_rows;
        upload(Gh, Gm, *self);
        inner = factory(Gm, *self);
        std::vector<int64_t> mg(H.l2g.begin(), H.l2g.begin() + nloc);
        src.alloc(std::max<int64_t>(N, 1));
        mine.alloc(std::max<int64_t>(nloc, 1));
        HIPCHK(hipMemcpyAsync(src.p, srcslot.data(), sizeof(int64_t) * N, hipMemcpyHostToDevice, c.st));
        if (nloc) HIPCHK(hipMemcpyAsync(mine.p, mg.data(), sizeof(int64_t) * nloc, hipMemcpyHostToDevice, c.st));
        sendbuf.alloc(std::max<int64_t>(maxloc, 1));
        HIPCHK(hipMemsetAsync(sendbuf.p, 0, sizeof(double) * std::max<int64_t>(maxloc, 1), c.st));
        gath.alloc(std::max<int64_t>(maxloc * G, 1));
        xg.alloc(std::max<int64_t>(N, 1));
        yg.alloc(std::max<int64_t>(N, 1));
        HIPCHK(hipEventCreateWithFlags(&ev_a, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ev_b, hipEventDisableTiming));
        self->sync();
        c.sync();
    }
    ~PCRedundant() override {
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
    }
    void apply(const double *x, double *y, Ctx &c) override {
        if (nloc) launch_copy(nloc, x, sendbuf.p, c.st);
        c.comm->allgather_dev(sendbuf.p, (int)std::max<int64_t>(maxloc, 1), gath.p, c.st);
        launch_gather(N, src.p, gath.p, xg.p, c.st);
        HIPCHK(hipEventRecord(ev_a, c.st));
        HIPCHK(hipStreamWaitEvent(self->st, ev_a, 0));
        inner->apply(xg.p, yg.p, *self);
        HIPCHK(hipEventRecord(ev_b, self->st));
        HIPCHK(hipStreamWaitEvent(c.st, ev_b, 0));
        launch_gather(nloc, mine.p, yg.p, y, c.st);
    }
    bool holds_ksp() const override { return inner->holds_ksp(); }
    const PC *unwrapped() const override { return inner->unwrapped(); }
};

std::unique_ptr<PC> make_redundant(const std::string &type, const DevCSR &M, Ctx &c,
                                   const std::function<std::unique_ptr<PC>(const DevCSR &, Ctx &)> &factory,
                                   const std::string &prefix, GatheredBlock *pre) {
    return std::make_unique<PCRedundant>(type, M, c, factory, prefix, pre);
}

std::unique_ptr<PC> make_pc(const std::string &type, const DevCSR &M, const Options &o, const std::string &prefix,
                            Ctx &c) {
    if (type == "none") return std::make_unique<PCNone>(M.nrows);
    if (type == "jacobi") return std::make_unique<PCJacobi>(M, c);
    const bool dist = c.comm && c.comm->size > 1;
    // whole-block PCs on a sharded block: gathered and applied redundantly (PCREDUNDANT)
    if (M.halo && (type == "ilu" || type == "lu" || type == "cholesky" || type == "gamg" || type == "hypre")) {
        // PETSc's own ILU refuses a parallel (MPIAIJ) matrix; MUMPS LU and hypre run
        // distributed.  Redundant ILU is an extension, on request only.
        if (type == "ilu" && !o.flag("pls.redundant_ilu", false))
            throw Error("PC type 'ilu' (prefix " + prefix + ") on a matrix sharded over " +
                        std::to_string(c.comm ? c.comm->size : 1) +
                        " ranks: PETSc's ILU does not run on MPIAIJ matrices (use bjacobi, or pls.redundant_ilu 1 "
                        "for the one-rank ILU applied redundantly)");
        GatheredBlock pre;
        bool gathered = false;
        if (type == "hypre" && o.str("pls.hypre", "boomeramg") == "boomeramg") {
            // the Jacobi-type and Chebyshev smoothers are built on one rank's blocks only
            boomeramg_refuse_sharded_relax(o, prefix);
        }
        if (type == "hypre" && o.str("pls.hypre", "boomeramg") == "boomeramg" && o.flag("pls.hypre_dist", true)) {
            // BoomerAMG as under mpirun -np G: the np = G hierarchy, each rank smoothing its
            // own rows (Jacobi across ranks); needs ranks owning contiguous rows in rank order
            pre.G = gather_block(M, c, prefix, pre.srcslot, pre.maxloc, pre.rank_rows);
            gathered = true;
            if (!pre.rank_rows.empty()) return make_boomeramg_dist(M, pre.G, pre.rank_rows, o, prefix, c);
        }
        if (o.flag("pls.redundant_error", false))
            throw Error("PC type '" + type + "' (prefix " + prefix + ") acts on the whole parallel matrix (pls.redundant_error)");
        return make_redundant(type, M, c, [&](const DevCSR &Gm, Ctx &sc) { return make_pc(type, Gm, o, prefix, sc); },
                              prefix, gathered ? &pre : nullptr);
    }
    if (type == "ilu") {
        using Cfg = PCILU::Config;
        return std::make_unique<PCILU>(M, 1, c, Cfg::from_options(o, prefix, Cfg::Tuning | Cfg::Depth | Cfg::Levels));
    }
    if (type == "lu" || type == "cholesky") return make_lu(M, o, c);
    if (type == "bjacobi") {
        // total blocks over all ranks (PCBJacobiSetTotalBlocks): rank r gets
        // B / size (+1 for the first B % size ranks); at least one per rank
        const int64_t nbt = o.integer(prefix + "pc_bjacobi_blocks", dist ? c.comm->size : 1);
        int64_t nb = nbt;
        if (dist) nb = std::max<int64_t>(1, nbt / c.comm->size + (c.comm->rank < nbt % c.comm->size ? 1 : 0));
        const std::string sub = o.str(prefix + "sub_pc_type", "ilu");
        if (sub == "ilu") {
            using Cfg = PCILU::Config;
            return std::make_unique<PCILU>(
                M, nb, c, Cfg::from_options(o, prefix, Cfg::Tuning | Cfg::Depth | Cfg::LprProfile | Cfg::SubLevels));
        }
        if (sub == "jacobi") return std::make_unique<PCJacobi>(M, c);
        if (sub == "none") return std::make_unique<PCNone>(M.nrows);
        throw Error(prefix + "sub_pc_type " + sub + " is not available on the device");
    }
    // overlapping additive Schwarz on one rank (asm.cpp; refuses a sharded matrix itself)
    if (type == "asm") return std::make_unique<PCASM>(M, o, prefix, c);
    if (type == "gamg") return make_amg(M, o, prefix, false, c);
    if (type == "hypre") {
        // hypre is not in this image: classical AMG restating BoomerAMG as the
        // reference configures it (oracle/boomeramg.py); pls.hypre sa selects
        // the smoothed-aggregation AMG instead, pls.hypre error the refusal
        const std::string h = o.str("pls.hypre", "boomeramg");
        if (h == "error")
            throw Error("PC type 'hypre' (prefix " + prefix + ") is not available (pls.hypre error)");
        if (h == "sa" || h == "gamg") return make_amg(M, o, prefix, true, c);
        if (h != "boomeramg") throw Error("pls.hypre " + h + ": expected boomeramg, sa or error");
        return make_boomeramg(M, o, prefix, c);
    }
    throw Error("PC type '" + type + "' (prefix " + prefix +
                ") is not available in this build (supported: none, jacobi, ilu, bjacobi, asm, lu, gamg, hypre)");
}

// =========================================================== fieldsplit ===
void upload(const HostCSR &H, DevCSR &M, Ctx &c) {
    upload_csr(M, H.nrows, H.ncols, H.rp.data(), H.ci.data(), H.v.data(), c);
}

// D2H of a matrix: the host arrays are allocated (zero-filled) on their own
// threads while the row pointers come over; big arrays then move through two
// pinned staging buffers, each chunk spread back by host threads (a pageable
// hipMemcpy of the N=59 s block's 5.1 GB ran at ~5 GB/s)
namespace {
// pinned staging buffers and their events, released on every path (a HIPCHK
// that throws mid-copy must not leak them: ADVICE r04)
struct Staging {
    void *buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    explicit Staging(size_t bytes) {
        for (int b = 0; b < 2; ++b) {
            HIPCHK(hipHostMalloc(&buf[b], bytes, hipHostMallocDefault));
            HIPCHK(hipEventCreateWithFlags(&ev[b], hipEventDisableTiming));
        }
    }
    ~Staging() {
        for (int b = 0; b < 2; ++b) {
            if (ev[b]) (void)hipEventDestroy(ev[b]);
            if (buf[b]) (void)hipHostFree(buf[b]);
        }
    }
    Staging(const Staging &) = delete;
    Staging &operator=(const Staging &) = delete;
};

void d2h_staged(void *dst, const void *src, size_t bytes, Ctx &c) {
    const size_t CH = (size_t)64 << 20;
    if (bytes < 2 * CH) {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c.st));
        c.sync();
        return;
    }
    Staging S(CH);
    const size_t nch = (bytes + CH - 1) / CH;
    auto issue = [&](size_t k) {
        const size_t off = k * CH, len = std::min(CH, bytes - off);
        HIPCHK(hipMemcpyAsync(S.buf[k & 1], (const char *)src + off, len, hipMemcpyDeviceToHost, c.st));
        HIPCHK(hipEventRecord(S.ev[k & 1], c.st));
    };
    issue(0);
    const int T = 8;
    for (size_t k = 0; k < nch; ++k) {
        if (k + 1 < nch) issue(k + 1);  // (the other buffer: its copy-out finished below)
        HIPCHK(hipEventSynchronize(S.ev[k & 1]));
        const size_t off = k * CH, len = std::min(CH, bytes - off);
        std::vector<std::thread> th;
        for (int t = 0; t < T; ++t)
            th.emplace_back([&, t] {
                const size_t a = len * t / T, b = len * (t + 1) / T;
                std::memcpy((char *)dst + off + a, (const char *)S.buf[k & 1] + a, b - a);
            });
        for (auto &x : th) x.join();
    }
}
}  // namespace

HostCSR download(const DevCSR &M, Ctx &c) {
    HostCSR H;
    H.nrows = M.nrows;
    H.ncols = M.ncols;
    H.rp.resize(M.nrows + 1);
    {
        // (joined on every path: a HIPCHK that throws below must not destroy joinable threads)
        std::thread tci([&] { H.ci.resize(M.nnz); }), tv([&] { H.v.resize(M.nnz); });
        struct Join {
            std::thread &a, &b;
            ~Join() {
                if (a.joinable()) a.join();
                if (b.joinable()) b.join();
            }
        } join{tci, tv};
        HIPCHK(hipMemcpyAsync(H.rp.data(), M.rp.p, sizeof(int64_t) * (M.nrows + 1), hipMemcpyDeviceToHost, c.st));
        c.sync();
    }
    if (M.nnz) {
        d2h_staged(H.ci.data(), M.ci.p, sizeof(int32_t) * M.nnz, c);
        d2h_staged(H.v.data(), M.val.p, sizeof(double) * M.nnz, c);
    }
    return H;
}

namespace {
// rows `rows`, columns mapped by cmap (-1: dropped); cmap is monotone on the
// kept columns, so rows stay sorted (MatCreateSubMatrix with sorted ISs)
HostCSR submatrix(const HostCSR &M, const std::vector<int32_t> &rows, const std::vector<int32_t> &cmap,
                  int64_t ncols) {
    HostCSR S;
    S.nrows = (int64_t)rows.size();
    S.ncols = ncols;
    S.rp.assign(1, 0);
    for (int32_t r : rows) {
        for (int64_t k = M.rp[r]; k < M.rp[r + 1]; ++k) {
            const int32_t m = cmap[M.ci[k]];
            if (m >= 0) {
                S.ci.push_back(m);
                S.v.push_back(M.v[k]);
            }
        }
        S.rp.push_back((int64_t)S.ci.size());
    }
    return S;
}

// MatSchurComplementGetPmat, AINV_DIAG: D - C diag(A)^-1 B.  diag reciprocal
// keeps zeros (VecReciprocal); AinvB = row-scaled B; the product row i sums
// over k ascending (MatMatMult, sorted algorithm); then MatAYPX(S, -1, D).
HostCSR selfp(const HostCSR &A, const HostCSR &B, const HostCSR &C, const HostCSR &D) {
    std::vector<double> dinv(A.nrows, 0.0);
    for (int64_t i = 0; i < A.nrows; ++i)
        for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k)
            if (A.ci[k] == i) dinv[i] = A.v[k] != 0.0 ? 1.0 / A.v[k] : 0.0;
    std::vector<double> bs(B.v.size());
    for (int64_t i = 0; i < B.nrows; ++i)
        for (int64_t k = B.rp[i]; k < B.rp[i + 1]; ++k) bs[k] = dinv[i] * B.v[k];
    HostCSR S;
    S.nrows = D.nrows;
    S.ncols = D.ncols;
    std::vector<double> acc(D.ncols, 0.0);
    std::vector<char> mark(D.ncols, 0);
    std::vector<int32_t> cols;
    for (int64_t i = 0; i < C.nrows; ++i) {
        cols.clear();
        for (int64_t kk = C.rp[i]; kk < C.rp[i + 1]; ++kk) {
            const int32_t k = C.ci[kk];
            const double a = C.v[kk];
            for (int64_t jj = B.rp[k]; jj < B.rp[k + 1]; ++jj) {
                const int32_t j = B.ci[jj];
                if (!mark[j]) {
                    mark[j] = 1;
                    acc[j] = 0.0;
                    cols.push_back(j);
                }
                acc[j] += a * bs[jj];
            }
        }
        for (int64_t kk = D.rp[i]; kk < D.rp[i + 1]; ++kk)
            if (!mark[D.ci[kk]]) {
                mark[D.ci[kk]] = 2;  // D only
                cols.push_back(D.ci[kk]);
            }
        std::sort(cols.begin(), cols.end());
        int64_t dk = D.rp[i];
        for (int32_t j : cols) {
            double dv = 0.0;
            bool hasd = false;
            while (dk < D.rp[i + 1] && D.ci[dk] < j) ++dk;
            if (dk < D.rp[i + 1] && D.ci[dk] == j) {
                dv = D.v[dk];
                hasd = true;
            }
            double out;
            if (mark[j] == 2) out = dv;
            else out = hasd ? dv - acc[j] : -acc[j];
            S.ci.push_back(j);
            S.v.push_back(out);
            mark[j] = 0;
        }
        S.rp.push_back((int64_t)S.ci.size());
    }
    return S;
}


// S x = A11 x - A10 A00^-1 A01 x (MatMult_SchurComplement; inner solve = the split-0 KSP)
struct SchurOp : Op {
    const DevCSR *A01, *A10, *A11;
    KSP *k0;
    DBuf<double> w1, w2, w3;
    SchurOp(const DevCSR *a01, const DevCSR *a10, const DevCSR *a11, KSP *k) : A01(a01), A10(a10), A11(a11), k0(k) {
        n = a11->nrows;
        w1.alloc(std::max<int64_t>(a01->nrows, 1));
        w2.alloc(std::max<int64_t>(a01->nrows, 1));
        w3.alloc(std::max<int64_t>(n, 1));
    }
    void apply(const double *x, double *y, Ctx &c) override {
        spmv(*A01, x, w1.p, c);
        k0->solve(w1.p, w2.p, c);
        spmv(*A10, w2.p, w3.p, c);
        spmv(*A11, x, y, c, 1.0, -1.0, w3.p);
    }
};
}  // namespace

PCFieldSplit::PCFieldSplit(const DevCSR &M, const std::vector<int32_t> &s0, const std::vector<int32_t> &s1,
                           const Options &o, const std::string &prefix, Ctx &c) {
    type = "fieldsplit";
    n = M.nrows;
    if (M.halo) throw Error(prefix + "pc_type fieldsplit: not available with several ranks");
    n0 = (int64_t)s0.size();
    n1 = (int64_t)s1.size();
    if (n0 == 0 || n1 == 0 || n0 + n1 != n)
        throw Error(prefix + "pc_type fieldsplit: the two splits must be non-empty and cover the block (" +
                    std::to_string(n0) + " + " + std::to_string(n1) + " of " + std::to_string(n) + " rows)");
    ftype = o.str(prefix + "pc_fieldsplit_type", "multiplicative");
    if (ftype != "additive" && ftype != "multiplicative" && ftype != "schur")
        throw Error(prefix + "pc_fieldsplit_type " + ftype + " is not available (additive, multiplicative, schur)");
    const HostCSR Mh = download(M, c);
    std::vector<int32_t> m0(n, -1), m1(n, -1);
    for (int64_t i = 0; i < n0; ++i) m0[s0[i]] = (int32_t)i;
    for (int64_t i = 0; i < n1; ++i) m1[s1[i]] = (int32_t)i;
    const HostCSR h00 = submatrix(Mh, s0, m0, n0), h01 = submatrix(Mh, s0, m1, n1);
    const HostCSR h10 = submatrix(Mh, s1, m0, n0), h11 = submatrix(Mh, s1, m1, n1);
    upload(h00, A00, c);
    upload(h01, A01, c);
    upload(h10, A10, c);
    upload(h11, A11, c);
    for (DevCSR *B : {&A01, &A10, &A11}) build_sell(*B, c);
    const std::string p0 = prefix + "fieldsplit_0_", p1 = prefix + "fieldsplit_1_";
    k0 = make_ksp(p0, o, &A00, &A00, "preonly", "ilu", c);
    if (ftype == "schur") {
        fact = o.str(prefix + "pc_fieldsplit_schur_fact_type", "full");
        if (fact != "diag" && fact != "lower" && fact != "upper" && fact != "full")
            throw Error(prefix + "pc_fieldsplit_schur_fact_type " + fact + " is not available");
        scale = o.num(prefix + "pc_fieldsplit_schur_scale", -1.0);
        const std::string pre = o.str(prefix + "pc_fieldsplit_schur_precondition", "a11");
        const DevCSR *pmat = &A11;
        if (pre == "selfp") {
            upload(selfp(h00, h01, h10, h11), Sp, c);
            pmat = &Sp;
        } else if (pre != "a11") {
            throw Error(prefix + "pc_fieldsplit_schur_precondition " + pre + " is not available (selfp, a11)");
        }
        k1 = make_ksp(p1, o, nullptr, pmat, "gmres", "ilu", c);
        k1->owned_op = std::make_unique<SchurOp>(&A01, &A10, &A11, k0.get());
        k1->A = k1->owned_op.get();
        k1->n = n1;
    } else {
        k1 = make_ksp(p1, o, &A11, &A11, "preonly", "ilu", c);
    }
    for (auto *b : {&x0, &y0, &t0}) b->alloc(std::max<int64_t>(n0, 1));
    for (auto *b : {&x1, &y1, &t1}) b->alloc(std::max<int64_t>(n1, 1));
    is0.alloc(std::max<int64_t>(n0, 1));
    is1.alloc(std::max<int64_t>(n1, 1));
    if (n0) HIPCHK(hipMemcpyAsync(is0.p, s0.data(), sizeof(int32_t) * n0, hipMemcpyHostToDevice, c.st));
    if (n1) HIPCHK(hipMemcpyAsync(is1.p, s1.data(), sizeof(int32_t) * n1, hipMemcpyHostToDevice, c.st));
    c.sync();
}

// PCApply_FieldSplit / PCApply_FieldSplit_Schur
void PCFieldSplit::apply(const double *x, double *y, Ctx &c) {
    launch_pack(n0, is0.p, x, x0.p, c.st);
    launch_pack(n1, is1.p, x, x1.p, c.st);
    auto x1_minus_A10 = [&](const double *v) { spmv(A10, v, t1.p, c, -1.0, 1.0, x1.p); };   // t1 = x1 - A10 v
    auto x0_minus_A01 = [&](const double *v) { spmv(A01, v, t0.p, c, -1.0, 1.0, x0.p); };   // t0 = x0 - A01 v
    if (ftype == "additive") {
        k0->solve(x0.p, y0.p, c);
        k1->solve(x1.p, y1.p, c);
    } else if (ftype == "multiplicative" || fact == "lower") {
        k0->solve(x0.p, y0.p, c);
        x1_minus_A10(y0.p);
        k1->solve(t1.p, y1.p, c);
    } else if (fact == "diag") {
        k0->solve(x0.p, y0.p, c);
        k1->solve(x1.p, y1.p, c);
        launch_scale(n1, scale, y1.p, c.st);
    } else if (fact == "upper") {
        k1->solve(x1.p, y1.p, c);
        x0_minus_A01(y1.p);
        k0->solve(t0.p, y0.p, c);
    } else {  // full
        k0->solve(x0.p, y0.p, c);
        x1_minus_A10(y0.p);
        k1->solve(t1.p, y1.p, c);
        x0_minus_A01(y1.p);
        k0->solve(t0.p, y0.p, c);
    }
    launch_unpack(n0, is0.p, y0.p, y, c.st);
    launch_unpack(n1, is1.p, y1.p, y, c.st);
}

}  // namespace pls
