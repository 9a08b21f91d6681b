// bccols.hpp -- Dirichlet columns of a bc.apply block (<prefix>pls_bc_columns keep | lift | drop;
// kernels in bccols.hip, host code in bccols.cpp).  DESIGN.md section 25.  A KSP owns one
// BcColumns when the option is not keep (runtime.hpp declares the type only).
//
// dolfin's bc.apply replaces a constrained row of a block K by an identity row and keeps the
// row's column, so K is not symmetric.  Row i being an identity row, x_i = b_i in K x = b, and
// column i can move to the right-hand side: K = K' + C with C the off-diagonal entries in
// constrained columns, K^-1 b = K'^-1 (b - C b).  K' is symmetric wherever the assembled form was.
//   lift   every solve forms b' = b - C b first and solves K' x = b'
//   drop   K' without the correction: another preconditioner (what a CPU oracle handed a
//          column-zeroed P computes)
#pragma once
#include "runtime.hpp"

namespace pls {

// -------------------------------------------------------------- launchers --
// flag8[i] = flag[i] = 1 where row i is constrained: its diagonal is stored and equals 1.0
// exactly, every other stored value of the row is 0.0.  One wave per row.
void launch_bc_flag(int64_t n, const int64_t *rp, const int32_t *ci, const double *val, uint8_t *flag8,
                    int64_t *flag, hipStream_t st);
// out[pos[i]] = i for every i with flag[i] != 0 (pos: the exclusive scan of flag): ascending
void launch_bc_compact(int64_t n, const int64_t *flag, const int64_t *pos, int32_t *out, hipStream_t st);
// cnt[i] = the stored nonzero values of row i in constrained columns other than i; has[i] = cnt[i] > 0
void launch_bc_split_count(int64_t n, const int64_t *rp, const int32_t *ci, const double *val,
                           const uint8_t *flag8, int64_t *cnt, int64_t *has, hipStream_t st);
// Row i's moved entries to (cci, cval) from cptr[i] on, in stored order; every value of row i in a
// constrained column other than i becomes 0.0 in val (the copy's values, in place).
void launch_bc_split_fill(int64_t n, const int64_t *rp, const int32_t *ci, double *val, const uint8_t *flag8,
                          const int64_t *cptr, int32_t *cci, double *cval, hipStream_t st);
// the compact row pointers: crp[k] = cptr[crow[k]], crp[nrc] = cptr[n]
void launch_bc_rowptr(int64_t nrc, int64_t n, const int32_t *crow, const int64_t *cptr, int64_t *crp,
                      hipStream_t st);
// the lift's row map: bit i of mask is has[i], base[w] = C rows below row 32 w (hpos: the scan of has)
void launch_bc_mask(int64_t n, const int64_t *has, const int64_t *hpos, uint32_t *mask, int32_t *base,
                    hipStream_t st);
// out = b - C b, every entry of out written by the thread that owns it (out is not b)
void launch_bc_lift(int64_t n, const double *b, const uint32_t *mask, const int32_t *base, const int64_t *crp,
                    const int32_t *cci, const double *cval, double *out, hipStream_t st);

// ---------------------------------------------------------------- the split --
struct BcColumns {
    enum Mode { KEEP = 0, LIFT = 1, DROP = 2 };
    int mode = KEEP;
    int64_t n = 0;
    int64_t nbc = 0;     // constrained rows
    int64_t nmoved = 0;  // entries moved to C
    int64_t nrc = 0;     // rows of C
    DevCSR Kp;           // K' (empty while nothing moved: the block itself serves)
    DBuf<int32_t> bc_rows;  // the constrained rows, ascending
    DBuf<int32_t> crow;     // C: its rows, ascending ...
    DBuf<int64_t> crp;      // ... their row pointers (nrc + 1) ...
    DBuf<int32_t> cci;      // ... and entries, columns ascending within a row
    DBuf<double> cval;
    DBuf<uint32_t> mask;  // lift: one bit per row of the block, set on C's rows
    DBuf<int32_t> base;   // lift: C rows in front of each mask word
    DBuf<double> bl;      // lift: b'
    // detect and split K on the device; the host sees the three counts only
    void build(const DevCSR &K, int mode, const std::string &key, Ctx &c);
    bool has_copy() const { return nmoved > 0; }
    bool lifting() const { return mode == LIFT && nmoved > 0; }
    // b' = b - C b into bl; returns bl.p
    const double *lift(const double *b, Ctx &c);
    int64_t bytes() const;
};

}  // namespace pls
