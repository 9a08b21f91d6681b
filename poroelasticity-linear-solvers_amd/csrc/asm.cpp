// asm.cpp -- PCASM: PETSc's overlapping additive Schwarz on one rank (pc_type asm; kernels in
// asm.hip, the fused application in sweep_lds.hip).  DESIGN.md section 24.
//
// Setup, all on the device: grow the subdomains (count, scan, fill), build the extended
// block-diagonal matrix E = diag(M[I_b, I_b]) (count, scan, fill) and the transpose map of the
// summed outputs, then hand E with the subdomain bounds to a PCILU -- its block truncation is a
// no-op on E, and factorisation, ILU(k), the sweep choice and every table builder serve asm
// unchanged.  The host sees the B + 1 subdomain offsets and E's row pointers' last entry only.
#include "runtime.hpp"

#include <algorithm>
#include <climits>
#include <cstdio>

namespace pls {

static int64_t asm_integer(const Options &o, const std::string &k, int64_t dflt, const char *what) {
    const std::string v = o.str(k, "");
    if (v.empty()) return dflt;
    size_t used = 0;
    long long x = 0;
    try { x = std::stoll(v, &used); } catch (...) { used = 0; }
    if (used != v.size()) throw Error("option " + k + ": " + what + " must be an integer, got '" + v + "'");
    return (int64_t)x;
}

PCASM::PCASM(const DevCSR &M, const Options &o, const std::string &prefix, Ctx &c) {
    type = "asm";
    n = M.nrows;
    // ---- options and refusals (each names its key and the condition)
    if (M.halo)
        throw Error("option " + prefix + "pc_type asm (prefix " + prefix + ") on a matrix sharded over " +
                    std::to_string(c.comm ? c.comm->size : 1) +
                    " ranks: overlap across ranks is not available (use bjacobi)");
    const std::string local = o.str(prefix + "pc_asm_local_type", "additive");
    if (local != "additive")
        throw Error("option " + prefix + "pc_asm_local_type " + local + ": only additive is available");
    const std::string sub = o.str(prefix + "sub_pc_type", "ilu");
    if (sub != "ilu") throw Error("option " + prefix + "sub_pc_type " + sub + ": asm's subdomain PC is ilu only");
    overlap = asm_integer(o, prefix + "pc_asm_overlap", 1, "the overlap");
    if (overlap < 0 || overlap > INT_MAX)
        throw Error("option " + prefix + "pc_asm_overlap " + std::to_string(overlap) + ": the overlap must be a non-negative integer");
    static const char *const names[] = {"restrict", "basic", "interpolate", "none"};
    const std::string tn = o.str(prefix + "pc_asm_type", "restrict");
    int t = 0;
    while (t < 4 && tn != names[t]) ++t;
    if (t == 4) throw Error("option " + prefix + "pc_asm_type " + tn + ": expected restrict, basic, interpolate or none");
    atype = (Type)t;
    // No default for the block count.  PETSc's is one block per rank, which on one rank is plain ilu
    // under another name; a database that names asm without saying how many subdomains it wants is
    // refused as it was before asm existed, instead of quietly running ILU.
    if (o.str(prefix + "pc_asm_blocks", "").empty())
        throw Error("PC type 'asm' (prefix " + prefix + ") needs option " + prefix +
                    "pc_asm_blocks, the total number of subdomains (1: the whole block, which is ilu)");
    nblocks = asm_integer(o, prefix + "pc_asm_blocks", 1, "the number of blocks");
    if (nblocks < 1 || nblocks > n)
        throw Error("option " + prefix + "pc_asm_blocks " + std::to_string(nblocks) + ": expected 1 to the block's " +
                    std::to_string(n) + " rows");
    if (n >= INT32_MAX) throw Error("option " + prefix + "pc_type asm: rows are 32-bit indices, the block has " + std::to_string(n));
    const bool want_fused = o.flag("pls.asm_fused", true);

    // ---- subdomains: count, scan, fill
    const int grid = (int)std::min<int64_t>(nblocks, ASM_GROW_GRID);
    const int64_t nw = (n + 31) / 32;
    DBuf<unsigned> bits((size_t)grid * 3 * nw);
    HIPCHK(hipMemsetAsync(bits.p, 0, sizeof(unsigned) * bits.n, c.st));
    DBuf<int64_t> cnt(nblocks + 1);
    ptr.alloc(nblocks + 1);
    launch_asm_grow(false, grid, n, nblocks, (int)overlap, M.rp.p, M.ci.p, bits.p, nw, cnt.p, nullptr, nullptr, nullptr,
                    c.st);
    HIPCHK(hipGetLastError());
    c.ensure_scan(std::max(nblocks, n));
    exclusive_scan_i64(cnt.p, ptr.p, nblocks, c.scan_tmp.p, c.scan_tmp_bytes, c.st);
    ptr_h.resize(nblocks + 1);
    HIPCHK(hipMemcpyAsync(ptr_h.data(), ptr.p, sizeof(int64_t) * (nblocks + 1), hipMemcpyDeviceToHost, c.st));
    c.sync();
    ne = ptr_h[nblocks];
    for (int64_t b = 0; b < nblocks; ++b) largest = std::max(largest, ptr_h[b + 1] - ptr_h[b]);
    if (ne >= (int64_t)INT32_MAX)
        throw Error("option " + prefix + "pc_type asm: the subdomains hold " + std::to_string(ne) +
                    " rows in all, extended positions are 32-bit (lower " + prefix + "pc_asm_overlap or " + prefix +
                    "pc_asm_blocks)");
    // PCILU's extraction launches 64 work-items per row, and one dispatch holds 2^32 of them
    if (ne >= ((int64_t)1 << 26))
        throw Error("option " + prefix + "pc_type asm: the subdomains hold " + std::to_string(ne) +
                    " rows in all, the factorisation takes fewer than " + std::to_string((int64_t)1 << 26) +
                    " (lower " + prefix + "pc_asm_overlap, or change " + prefix + "pc_asm_blocks)");
    gidx.alloc(std::max<int64_t>(ne, 1));
    own.alloc(std::max<int64_t>(ne, 1));
    launch_asm_grow(true, grid, n, nblocks, (int)overlap, M.rp.p, M.ci.p, bits.p, nw, nullptr, ptr.p, gidx.p, own.p,
                    c.st);
    HIPCHK(hipGetLastError());

    // ---- the extended matrix: count, scan, fill
    DevCSR E;
    E.nrows = E.ncols = ne;
    {
        DBuf<int64_t> len(ne + 1);
        E.rp.alloc(ne + 1);
        launch_asm_extend(false, ne, n, nblocks, ptr.p, gidx.p, M.rp.p, M.ci.p, M.val.p, len.p, nullptr, nullptr,
                          nullptr, c.st);
        HIPCHK(hipGetLastError());
        c.ensure_scan(ne);
        exclusive_scan_i64(len.p, E.rp.p, ne, c.scan_tmp.p, c.scan_tmp_bytes, c.st);
        HIPCHK(hipMemcpyAsync(&E.nnz, E.rp.p + ne, sizeof(int64_t), hipMemcpyDeviceToHost, c.st));
        c.sync();  // (bits and len are freed below)
    }
    bits.release();
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const double need = (double)E.nnz * 12.0 + (double)(ne + 1) * 8.0;
    if (E.nnz < 0 || need > 0.9 * (double)free_b)
        throw Error("option " + prefix + "pc_type asm: the extended matrix has " + std::to_string(E.nnz) + " entries (" +
                    std::to_string((int64_t)(need / 1048576.0)) + " MiB), " + std::to_string(free_b >> 20) +
                    " MiB of device memory are free; lower " + prefix + "pc_asm_overlap");
    E.ci.alloc(std::max<int64_t>(E.nnz, 1));
    E.val.alloc(std::max<int64_t>(E.nnz, 1));
    launch_asm_extend(true, ne, n, nblocks, ptr.p, gidx.p, M.rp.p, M.ci.p, M.val.p, nullptr, E.rp.p, E.ci.p, E.val.p,
                      c.st);
    HIPCHK(hipGetLastError());
    E.max_row = M.max_row;  // (a bound: E's rows are M's with entries dropped)

    // ---- the transpose map of the summed outputs
    {
        DBuf<int64_t> tc(n + 1);
        DBuf<int32_t> cursor(std::max<int64_t>(n, 1));
        tptr.alloc(n + 1);
        tpos.alloc(std::max<int64_t>(ne, 1));
        opos.alloc(std::max<int64_t>(n, 1));
        HIPCHK(hipMemsetAsync(tc.p, 0, sizeof(int64_t) * (n + 1), c.st));
        HIPCHK(hipMemsetAsync(cursor.p, 0, sizeof(int32_t) * std::max<int64_t>(n, 1), c.st));
        launch_asm_transpose_count(ne, gidx.p, own.p, tc.p, opos.p, c.st);
        exclusive_scan_i64(tc.p, tptr.p, n, c.scan_tmp.p, c.scan_tmp_bytes, c.st);
        launch_asm_transpose_fill(ne, n, gidx.p, tptr.p, cursor.p, tpos.p, c.st);
        HIPCHK(hipGetLastError());
        c.sync();
    }

    // ---- the subdomain solves: PCILU over E with the subdomain bounds (nblocks == 1: plain ilu)
    using Cfg = PCILU::Config;
    Cfg cfg = Cfg::from_options(o, prefix, Cfg::SubLevels | Cfg::Tuning | Cfg::Depth | Cfg::LprProfile);
    if (nblocks > 1) cfg.bounds = &ptr_h;
    inner = std::make_unique<PCILU>(E, nblocks, c, cfg);
    fused = want_fused && inner->sweep == PCILU::Sweep::Lds && inner->profile_tag.empty();
    if (c.ilu_view)
        fprintf(stderr, "[pls asm] prefix %s blocks %lld overlap %lld type %s rows %lld (%.3f n) largest %lld fused %s\n",
                prefix.c_str(), (long long)nblocks, (long long)overlap, names[t], (long long)ne,
                n ? (double)ne / (double)n : 0.0, (long long)largest, fused ? "yes" : "no");
}

void PCASM::apply(const double *x, double *y, Ctx &c) {
    Scratch &s = scratch[c.st];  // per stream: the concurrent 3-way sweeps may share a PC's type, never its vectors
    const size_t m = (size_t)std::max<int64_t>(ne, 1);
    PCILU &I = *inner;
    if (fused) {
        const bool direct = mask_out();
        // x == y with the direct store: another workgroup gathers overlap rows of x that this
        // one overwrites in y -- apply from a copy of x
        if (direct && x == y) {
            if (s.xc.n < (size_t)n) s.xc.alloc(std::max<int64_t>(n, 1));
            launch_copy(n, x, s.xc.p, c.st);
            x = s.xc.p;
        }
        if (!direct && s.ye.n < m) s.ye.alloc(m);
        launch_asm_blocks_lds(nblocks, ptr.p, I.max_len, I.Lf.goff.p, I.Ls.gslice.p, I.Ls.sptr.p, I.Ls.col.p, I.Ls.val.p,
                              I.Ls.lpr.p, I.Uf.goff.p, I.Us.gslice.p, I.Us.sptr.p, I.Us.col.p, I.Us.val.p, I.Us.lpr.p,
                              gidx.p, own.p, mask_in() ? 1 : 0, direct ? 1 : 0, x, direct ? y : s.ye.p, I.lds_tpb,
                              I.lds_rr ? 1 : 0, c.st);
        if (!direct) launch_asm_combine(n, 0, opos.p, tptr.p, tpos.p, s.ye.p, y, c.st);
        return;
    }
    // generic path, any inner sweep.  x == y is no hazard here: the gather has read all of x
    // before the combine writes y (one stream)
    if (s.xe.n < m) s.xe.alloc(m);
    if (s.ye.n < m) s.ye.alloc(m);
    launch_asm_gather(ne, gidx.p, own.p, mask_in() ? 1 : 0, x, s.xe.p, c.st);
    I.apply(s.xe.p, s.ye.p, c);
    launch_asm_combine(n, mask_out() ? 1 : 0, opos.p, tptr.p, tpos.p, s.ye.p, y, c.st);
}

}  // namespace pls
