// bccols.cpp -- BcColumns (bccols.hpp): detection and split of a bc.apply block on the device,
// and the lift in front of a solve.  DESIGN.md section 25.
//
// Setup: flag the constrained rows, scan, compact; count every row's entries in constrained
// columns, scan the counts and the rows that have any, compact, copy the block and fill -- C's
// entries in stored order, the copy's values zeroed.  The host reads back three counts.  A block
// without constrained rows, or whose constrained columns are already zero, is not copied: the
// block itself is K' then, and the solves are bitwise those of keep.
#include "bccols.hpp"

#include <climits>

namespace pls {

void BcColumns::build(const DevCSR &K, int mode_, const std::string &key, Ctx &c) {
    mode = mode_;
    n = K.nrows;
    nbc = nmoved = nrc = 0;
    if (n >= INT32_MAX)
        throw Error(key + ": rows are 32-bit indices, the block has " + std::to_string(n));
    if (n == 0) return;
    // ---- detection: a flag per row, its scan, the ascending list
    DBuf<uint8_t> flag8(n);
    DBuf<int64_t> flag(n + 1), pos(n + 1);
    HIPCHK(hipMemsetAsync(flag.p + n, 0, sizeof(int64_t), c.st));
    launch_bc_flag(n, K.rp.p, K.ci.p, K.val.p, flag8.p, flag.p, c.st);
    HIPCHK(hipGetLastError());
    c.ensure_scan(n);
    exclusive_scan_i64(flag.p, pos.p, n, c.scan_tmp.p, c.scan_tmp_bytes, c.st);
    HIPCHK(hipMemcpyAsync(&nbc, pos.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, c.st));
    c.sync();
    if (nbc == 0) return;
    bc_rows.alloc(nbc);
    launch_bc_compact(n, flag.p, pos.p, bc_rows.p, c.st);
    // ---- split, count pass: entries per row, and the rows that have any
    DBuf<int64_t> cnt(n + 1), has(n + 1), cptr(n + 1), hpos(n + 1);
    HIPCHK(hipMemsetAsync(cnt.p + n, 0, sizeof(int64_t), c.st));
    HIPCHK(hipMemsetAsync(has.p + n, 0, sizeof(int64_t), c.st));
    launch_bc_split_count(n, K.rp.p, K.ci.p, K.val.p, flag8.p, cnt.p, has.p, c.st);
    HIPCHK(hipGetLastError());
    exclusive_scan_i64(cnt.p, cptr.p, n, c.scan_tmp.p, c.scan_tmp_bytes, c.st);
    exclusive_scan_i64(has.p, hpos.p, n, c.scan_tmp.p, c.scan_tmp_bytes, c.st);
    HIPCHK(hipMemcpyAsync(&nmoved, cptr.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, c.st));
    HIPCHK(hipMemcpyAsync(&nrc, hpos.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, c.st));
    c.sync();
    if (nmoved == 0) {  // (nothing to move: the block is its own K')
        nrc = 0;
        return;
    }
    // ---- K': the block's copy
    Kp.nrows = K.nrows;
    Kp.ncols = K.ncols;
    Kp.nnz = K.nnz;
    Kp.max_row = K.max_row;
    Kp.tag = K.tag;
    Kp.rcm_auto = K.rcm_auto;
    Kp.rp.alloc(n + 1);
    Kp.ci.alloc(std::max<int64_t>(K.nnz, 1));
    Kp.val.alloc(std::max<int64_t>(K.nnz, 1));
    HIPCHK(hipMemcpyAsync(Kp.rp.p, K.rp.p, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToDevice, c.st));
    HIPCHK(hipMemcpyAsync(Kp.ci.p, K.ci.p, sizeof(int32_t) * K.nnz, hipMemcpyDeviceToDevice, c.st));
    HIPCHK(hipMemcpyAsync(Kp.val.p, K.val.p, sizeof(double) * K.nnz, hipMemcpyDeviceToDevice, c.st));
    // ---- split, fill pass
    crow.alloc(nrc);
    crp.alloc(nrc + 1);
    cci.alloc(nmoved);
    cval.alloc(nmoved);
    launch_bc_compact(n, has.p, hpos.p, crow.p, c.st);
    launch_bc_split_fill(n, Kp.rp.p, Kp.ci.p, Kp.val.p, flag8.p, cptr.p, cci.p, cval.p, c.st);
    launch_bc_rowptr(nrc, n, crow.p, cptr.p, crp.p, c.st);
    if (mode == LIFT) {
        const int64_t nw = (n + 31) / 32;
        mask.alloc(nw);
        base.alloc(nw);
        bl.alloc(n);
        launch_bc_mask(n, has.p, hpos.p, mask.p, base.p, c.st);
    }
    HIPCHK(hipGetLastError());
    c.sync();  // (the flags and the scans are freed here)
}

const double *BcColumns::lift(const double *b, Ctx &c) {
    launch_bc_lift(n, b, mask.p, base.p, crp.p, cci.p, cval.p, bl.p, c.st);
    return bl.p;
}

int64_t BcColumns::bytes() const {
    return (int64_t)(Kp.rp.n * sizeof(int64_t) + Kp.ci.n * sizeof(int32_t) + Kp.val.n * sizeof(double) +
                     bc_rows.n * sizeof(int32_t) + crow.n * sizeof(int32_t) + crp.n * sizeof(int64_t) +
                     cci.n * sizeof(int32_t) + cval.n * sizeof(double) + mask.n * sizeof(uint32_t) +
                     base.n * sizeof(int32_t) + bl.n * sizeof(double));
}

}  // namespace pls
