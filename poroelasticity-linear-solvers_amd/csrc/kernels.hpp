// kernels.hpp -- host launchers of the HIP/CDNA4 kernels (kernels.hip, ilu0.hip, sweep_lds.hip).
// Every launcher enqueues on `st` and never synchronises.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pls {

// ----------------------------------------------------------------- synth --
struct SynthDev {
    int32_t dim;
    uint64_t seed;
    double delta;
    int64_t n[3];
    int64_t off[3];
    int32_t cnt[6];
    const int32_t *offs[6];  // device pointers, sorted offsets per forward block
    // rows generated: local row l in [rloff[f], rloff[f] + rlen[f]) is global
    // row off[f] + rlo[f] + (l - rloff[f]) (identity for a single rank)
    int64_t rlo[3], rlen[3], rloff[3], nrows;
};
void launch_synth_count(const SynthDev &S, int64_t *row_len, hipStream_t st);
void launch_synth_fill(const SynthDev &S, int variant, const int64_t *row_ptr, int32_t *col,
                       double *val, hipStream_t st);
void launch_synth_rhs(const SynthDev &S, uint64_t seed, double *b, hipStream_t st);

// ---------------------------------------------------------------- CSR ops --
// Exclusive scan of n+1 entries: in[0..n) lengths -> out[0..n] offsets.
void exclusive_scan_i64(const int64_t *in, int64_t *out, int64_t n, void *tmp, size_t tmp_bytes,
                        hipStream_t st);
size_t exclusive_scan_tmp_bytes(int64_t n);

// Column-window extraction: rows [r0, r1) of (rp, ci, val); keep entries with
// column in the window of the row; output columns shifted by -cshift.
//   mode 0: window [c0, c1) for every row
//   mode 1: block-Jacobi window of the row's block, blocks over [0, r1-r0)
//           with PETSc sizes (first nb % .. blocks one longer), cshift = r0
struct WindowSpec {
    int mode;
    int64_t c0, c1;
    int64_t nblocks;                  // mode 1
    const int64_t *bstart = nullptr;  // mode 1: explicit block starts (nblocks + 1, device), else PETSc sizes
};
void launch_extract_count(const int64_t *rp, const int32_t *ci, int64_t r0, int64_t r1,
                          WindowSpec w, int64_t *row_len, hipStream_t st);
void launch_extract_fill(const int64_t *rp, const int32_t *ci, const double *val, int64_t r0,
                         int64_t r1, WindowSpec w, int64_t cshift, const int64_t *out_rp,
                         int32_t *out_ci, double *out_val, hipStream_t st);

// y = alpha * (M x) + beta * z     (z may be null when beta == 0)
void launch_spmv(int64_t nrows, int64_t nnz, const int64_t *rp, const int32_t *ci,
                 const double *val, const double *x, double *y, double alpha, double beta,
                 const double *z, hipStream_t st);

// ----------------------------------------------------------------- BLAS-1 --
void launch_copy(int64_t n, const double *x, double *y, hipStream_t st);
void launch_copy_probe(int64_t n, const double *x, double *y, int mode /*0 copy, 1 read*/, hipStream_t st);
void launch_set(int64_t n, double a, double *y, hipStream_t st);
void launch_scale(int64_t n, double a, double *y, hipStream_t st);
// y = a*x + b*y
void launch_axpby(int64_t n, double a, const double *x, double b, double *y, hipStream_t st);
// the same with a = *pa, b = *pb read on the device; a no-op when *skip (device-resident CG)
void launch_axpby_dev(int64_t n, const double *pa, const double *x, const double *pb, double *y, const int64_t *skip,
                      hipStream_t st);
// device-resident CG (KSP::solve_cg_dev): scalar state S (doubles) / I (ints) and its phases
enum CgS { CG_BETA, CG_BETAOLD, CG_DPI, CG_A, CG_NEGA, CG_BB, CG_ONE, CG_RNORM, CG_RNORM0, CG_TTOL, CG_SLOT, CG_SLOT2,
           CG_NS = 16 };
enum CgI { CG_DONE, CG_ITS, CG_REASON, CG_HCOUNT, CG_NI = 8 };
enum CgPhase { CG_TOP, CG_MID, CG_POST, CG_END };
struct CgParams {
    double rtol, atol, dtol;
    int64_t maxit;
    int norm;  // 0 none, else the norm of S[CG_SLOT] is the residual norm
    int r_rtol, r_atol, r_dtol, r_nan, r_its, r_indef_pc, r_indef_mat;  // the KSPConvergedReason codes
};
void launch_cg_state(int phase, int64_t i, double *S, int64_t *I, double *hist, const CgParams &p, hipStream_t st);
// BiCGStab (KSP::solve_bcgs / solve_bcgs_dev): scalar state S (doubles), the ints of CgI, and its phases.
// BC_SLOT0.. receive the sums of the reducing kernels (one, two and two rows).
enum BcS { BC_RHO, BC_RHOOLD, BC_ALPHA, BC_NEGALPHA, BC_OMEGA, BC_NEGOMEGA, BC_OMEGAOLD, BC_BETA, BC_C1, BC_ONE,
           BC_RNORM0, BC_TTOL, BC_SLOT0, BC_SLOT1, BC_NS = 16 };
enum BcPhase { BC_MID1, BC_MID2, BC_POST };
struct BcgsParams {
    CgParams c;                 // tolerances, max_it, norm and the reasons of the convergence test
    int r_breakdown, r_pending;  // r_pending: (t, t) == 0, the driver decides on the host
};
// what a reducing kernel does with its block's sums: ticket == nullptr, write them as
// partials (launch_final and launch_bcgs_state follow); else the last block to arrive
// sums them into S[BC_SLOT0..], runs state phase `phase` of iteration i and resets the ticket
struct BcgsFuse {
    unsigned *ticket;
    int phase;
    int64_t i;
    double *S;
    int64_t *I;
    double *hist;
    BcgsParams p;
};
void launch_bcgs_state(int phase, int64_t i, double *S, int64_t *I, double *hist, const BcgsParams &p,
                       hipStream_t st);
// p = r - S[BC_C1] v + S[BC_BETA] p
void launch_bcgs_p(int64_t n, const double *r, const double *v, double *p, const double *S, const int64_t *skip,
                   hipStream_t st);
// w = *pa x + *pb y
void launch_waxpby_dev(int64_t n, const double *pa, const double *x, const double *pb, const double *y, double *w,
                       const int64_t *skip, hipStream_t st);
// (x, y) -> row 0
void launch_bcgs_dot(int64_t n, const double *x, const double *y, double *partial, const BcgsFuse &f,
                     const int64_t *skip, hipStream_t st);
// (s, t) -> row 0, (t, t) -> row 1, one pass
void launch_dot2(int64_t n, const double *s, const double *t, double *partial, const BcgsFuse &f, const int64_t *skip,
                 hipStream_t st);
// x += S[BC_ALPHA] p + S[BC_OMEGA] s, r = s - S[BC_OMEGA] t; (r, r) -> row 0, (r, rp) -> row 1
void launch_bcgs_update(int64_t n, const double *p, const double *s, const double *t, const double *rp, double *x,
                        double *r, double *partial, const BcgsFuse &f, const int64_t *skip, hipStream_t st);
// out[j] = sum over blocks of row j of the partials (j < rows), in the fixed order
void launch_final(int64_t n, int rows, const double *partial, double *out, hipStream_t st);
// w = a*x + b*y  (out of place)
void launch_waxpby(int64_t n, double a, const double *x, double b, const double *y, double *w,
                   hipStream_t st);
void launch_pointwise_mult(int64_t n, const double *x, const double *d, double *y, hipStream_t st);
// AMG smoother step: d = a d + bc (dinv . r); x += d.  flags 1: d not read
// (d = bc (dinv . r)); flags 2: x not read (x = d)
void launch_cheb_step(int64_t n, const double *dinv, const double *r, double *d, double *x, double a, double bc,
                      int flags, hipStream_t st);
// polynomial KSP update: out = a pm1 + b pk + c t, t = dinv ? dinv . z : z; a null pm1 / pk
// term is omitted; out may alias pm1 or pk
void launch_poly_update(int64_t n, double a, const double *pm1, double b, const double *pk, double c,
                        const double *dinv, const double *z, double *out, hipStream_t st);
void launch_zero_entries(int64_t m, const int32_t *idx, double *y, hipStream_t st);
void launch_gather(int64_t n, const int64_t *idx, const double *x, double *y, hipStream_t st);
void launch_scatter(int64_t n, const int64_t *idx, const double *x, double *y, hipStream_t st);

// deterministic reductions: fixed grid (depends only on n)
int reduce_blocks(int64_t n);
// The four kernels over the Krylov basis V, stored in fp64 or (compressed-basis GMRES,
// pls_gmres_basis single) in fp32; w and all sums fp64.  Columns 512-B aligned: ldv a multiple
// of 64 doubles / 128 floats.
// partial[j*NB + b] for j < k :  dot(v_j, w) ; then final into out[j]
void launch_mdot(int64_t n, int k, const double *V, int64_t ldv, const double *w, double *partial, double *out,
                 hipStream_t st);
void launch_mdot(int64_t n, int k, const float *V, int64_t ldv, const double *w, double *partial, double *out,
                 hipStream_t st);
void launch_dot(int64_t n, const double *x, const double *y, double *partial, double *out,
                hipStream_t st);
// out = ||x||_2 (sqrt of sum of squares)
void launch_norm2(int64_t n, const double *x, double *partial, double *out, hipStream_t st);
// w -= sum_j h[j] * V[:, j] (h on device, j < k); out = ||w||_2^2 (local) when out != null
void launch_maxpy_norm(int64_t n, int k, const double *V, int64_t ldv, const double *h_dev, double *w,
                       double *partial, double *out, hipStream_t st);
void launch_maxpy_norm(int64_t n, int k, const float *V, int64_t ldv, const double *h_dev, double *w, double *partial,
                       double *out, hipStream_t st);
// one modified Gram-Schmidt step: w -= (*hprev) vprev (vprev != null), then (w, vj) over the
// updated w, (w, w) when vj is null.  ticket != null: the last block to arrive writes the sum
// to *out (a zeroed ticket word; one launch); else partial[block] (launch_final follows)
void launch_mgs_step(int64_t n, const double *vprev, const double *hprev, const double *vj, double *w, double *partial,
                     double *out, unsigned *ticket, hipStream_t st);
// (fp32 basis: no single-launch sums, ticket is null -- partial[block] always, launch_final follows)
void launch_mgs_step(int64_t n, const float *vprev, const double *hprev, const float *vj, double *w, double *partial,
                     double *out, unsigned *ticket, hipStream_t st);
// y = sum_j c[j] * V[:, j] (c on device)
void launch_lincomb(int64_t n, int k, const double *V, int64_t ldv, const double *c_dev, double *y,
                    hipStream_t st);
void launch_lincomb(int64_t n, int k, const float *V, int64_t ldv, const double *c_dev, double *y, hipStream_t st);
// Fischer guess, model 2 (ksp_guess_type fischer): the space's update after a solve.  X, B: the
// stored columns (stride ldv, a multiple of 64 doubles; columns 512-B aligned), m < GUESS_MAX of
// them; x, y = A x (16-B aligned); alpha = B^T y on the device.  Writes x - X alpha and
// y - B alpha into column m of X and B and ||y - B alpha||^2 (rank-local) into *out.  x == nullptr:
// in place on the pair already in column m (the second Gram-Schmidt pass).
static constexpr int GUESS_MAX = 64;
void launch_guess_update(int64_t n, int m, double *X, double *B, int64_t ldv, const double *alpha_dev,
                         const double *x, const double *y, double *partial, double *out, hipStream_t st);
// u *= a, v *= a (both 16-B aligned)
void launch_scale2(int64_t n, double a, double *u, double *v, hipStream_t st);
// Compressed-basis GMRES: the new basis vector, vf = fl32(a w), vd = vf promoted to fp64, one pass
void launch_scale_round(int64_t n, double a, const double *w, float *vf, double *vd, hipStream_t st);
// TSQR step (Anderson least squares): R of each TSQR rows-per-block row chunk of the
// m <= 16 columns, written as rows [b m, b m + m) of a column-major matrix (leading dim ldo)
int tsqr_rows_per_block();
void launch_tsqr(int64_t n, int m, const double *const *cols_dev, double *Rout, int64_t ldo, hipStream_t st);

// ------------------------------------- ILU(0), level tables, level sweeps (ilu0.hip) --
// Factor the rows of one level in place (original CSR): lu, diag pos, dinv.
// max_row: longest row of the matrix (<= ilu0_max_row(); staged in LDS).
int ilu0_max_row();
// max_staged: the most upper-part entries of one row's pivots (LDS sizing)
// test knobs (pls.ilu0_stage, pls.ilu_dep_grid): stage_cap < 0 default,
// 0 no staged pivots, > 0 at most that many staged entries; grid_cap > 0 caps
// k_ilu0_dep's persistent grid (1: one workgroup), 0 none
void launch_ilu0_level(int64_t nrows_level, const int32_t *rows, const int64_t *rp,
                       const int32_t *ci, double *lu, const int64_t *diag, double *dinv,
                       int32_t *fail, int64_t max_row, int64_t max_staged, int stage_cap, hipStream_t st);
// all levels in one launch (rows in level order; done: n flags, ctr: 2 ints -- scratch)
void launch_ilu0_dep(int64_t n, const int32_t *rows, const int64_t *rp, const int32_t *ci, double *lu,
                     const int64_t *diag, double *dinv, int32_t *fail, int64_t max_row, int64_t max_staged,
                     int stage_cap, int grid_cap, int32_t *done, int32_t *ctr, hipStream_t st);
void launch_find_diag(int64_t n, const int64_t *rp, const int32_t *ci, int64_t *diag, int32_t *fail,
                      hipStream_t st);
// Symmetric Gauss-Seidel "factors" in ILU(0) storage (hypre relax type 6 as a
// preconditioner M = (D + L) D^-1 (D + U)): strict-lower entries scaled by the
// column's 1/a_jj (the unit lower factor I + L D^-1), diagonal and upper kept
// (the upper factor D + U), dinv = 1/a_ii; fail |= 2 on a zero diagonal.
void launch_sgs_factor(int64_t n, const int64_t *rp, const int32_t *ci, double *lu, const int64_t *diag,
                       double *dinv, int32_t *fail, hipStream_t st);
// Level-ordered triangular factor storage ("row r of level order"): build
void launch_lvl_count(int64_t n, const int32_t *order, const int64_t *rp, const int64_t *diag,
                      int upper, int64_t *len, hipStream_t st);
void launch_lvl_fill(int64_t n, const int32_t *order, const int64_t *rp, const int32_t *ci,
                     const double *lu, const int64_t *diag, int upper, const int64_t *out_rp,
                     int32_t *out_ci, double *out_val, hipStream_t st);
// One level of the forward (unit lower) sweep: y[i] = b[i] - sum l_ij y[j]
// One level of the backward sweep:           y[i] = (y[i] - sum u_ij y[j]) * dinv[i]
void launch_trsv_level(int64_t r0, int64_t r1, const int32_t *row_of, const int64_t *rp,
                       const int32_t *ci, const double *val, const double *dinv_lvl,
                       const double *b, double *y, int lanes_per_row, hipStream_t st);

// Block-Jacobi sweep: blocks independent, one workgroup per block.
// blk_off[b]..blk_off[b+1] index lvl_ptr (row boundaries of block b's levels).
void launch_trsv_blocks(int64_t nblocks, const int64_t *blk_off, const int64_t *lvl_ptr, const int32_t *row_of,
                        const int64_t *rp, const int32_t *ci, const double *val, const double *dinv_lvl,
                        const double *b, double *y, int lanes_per_row, hipStream_t st);

// ------------------------------------------------- ILU(k) symbolic phase (iluk.hip) --
// The pattern of the levels-of-fill factorization from one
// breadth-first search per row of G(A) (U parts) and of G(A^T) (L parts, by columns).
struct IlukSearch {
    int64_t n;          // searches of the whole launch: rows 0 .. n - 1
    const int64_t *rp;  // the graph searched: the block's pattern, or its transpose (rows need not be sorted)
    const int32_t *ci;
    int levels;      // k >= 1
    int slot_bits;   // log2 of a search's hash table slots
    int transposed;  // 0: entries (i, t) of the search from i; 1: entries (t, i)
    int32_t *lcnt, *ucnt;  // entries left / right of the diagonal per row (the count pass writes them)
    int32_t *ovf_rows, *ovf_n;  // count pass: the rows whose search outgrew its LDS table
    const int64_t *orp;  // fill pass: the filled pattern's row pointers, columns (unsorted), L cursors
    int32_t *oci, *cursor;
    int32_t *fail;  // |= 1: a search outgrew the global-memory table too
};
int64_t iluk_search_table_ints(int slots);  // ints of one search's table and queue
// the transposed pattern: column counts (cnt: n + 1 zeroed entries), then the columns (cursor: n zeroed)
void launch_iluk_transpose_count(int64_t n, const int64_t *rp, const int32_t *ci, int64_t *cnt, hipStream_t st);
void launch_iluk_transpose_fill(int64_t n, const int64_t *rp, const int32_t *ci, const int64_t *trp, int32_t *cursor,
                                int32_t *tci, hipStream_t st);
// every row with tables in LDS; then the listed rows with tables in global memory (gtab: grid tables)
void launch_iluk_search(const IlukSearch &a, bool fill, hipStream_t st);
void launch_iluk_search_gmem(const IlukSearch &a, bool fill, int64_t nlist, int grid, int *gtab, hipStream_t st);
void launch_iluk_row_len(int64_t n, const int32_t *lcnt, const int32_t *ucnt, int64_t *len, hipStream_t st);
// sort every row's columns ascending (fail |= 2: a duplicate column)
void launch_iluk_sort_rows(int64_t n, const int64_t *rp, int32_t *ci, int64_t max_row, int32_t *fail, hipStream_t st);
// the block's values into the filled pattern (dval zeroed; fail |= 4: an entry without a place)
void launch_iluk_scatter(int64_t n, const int64_t *srp, const int32_t *sci, const double *sval, const int64_t *drp,
                         const int32_t *dci, double *dval, int32_t *fail, hipStream_t st);

// ------------------- SpMV layouts, block sweeps (kernels.hip, sweep_lds.hip) --
// SELL-64 (sliced ELLPACK, slice = 64 rows = one wave)
int64_t sell_nslices(int64_t nrows);
void launch_sell_slice_len(int64_t nrows, const int64_t *rp, int64_t *slen /* nslices+1 */, hipStream_t st);
void launch_sell_fill(int64_t nrows, const int64_t *rp, const int32_t *ci, const double *val, const int64_t *sptr,
                      int32_t *scol, double *sval, hipStream_t st);
// tag 1 = the outer operator A (separate kernel symbol in profiles);
// ghost != null: columns >= nlocal read ghost[c - nlocal] (halo entries)
void launch_sell_spmv(int64_t nrows, const int64_t *sptr, const int32_t *scol, const double *sval, const double *x,
                      double *y, double alpha, double beta, const double *z, int tag, const double *ghost,
                      int64_t nlocal, hipStream_t st);
// SELL-64 / D16 (16-bit column deltas, D16_SEG segment bases per lane, 1 or 8 lanes per row)
constexpr int D16_SEG = 4;      // segment bases per lane (rows of a single rank)
constexpr int D16_SEG_MAX = 8;  // ... with halo columns (own s/f/p + a neighbour's s/f/p)
// rstart (all three): where each row's entries begin inside [rp[row], rp[row + 1]) -- a layout
// without the rows' first columns (the reduced outer operator); null: rp[row].  A row of
// lpr > 1 lanes keeps each remaining entry on the lane it has in the full row: the phase
// (rstart[row] - rp[row]) % lpr shifts the lanes (d16_first, kernels.hip); phase 0 is the
// layout without rstart
void launch_d16_slice_len(int64_t nslices, const int64_t *sfirst, const int32_t *slpr, const int64_t *rp,
                          int64_t nrows, int64_t *slen /* nslices+1 */, hipStream_t st,
                          const int32_t *rowmap = nullptr /* slice position -> row (SELL-C-sigma) */,
                          const int64_t *rstart = nullptr);
void launch_d16_count(int64_t nslices, const int64_t *sfirst, const int32_t *slpr, const int64_t *rp,
                      const int32_t *ci, int64_t nrows, int32_t *maxseg, hipStream_t st,
                      const int32_t *rowmap = nullptr, const int64_t *rstart = nullptr);
void launch_d16_fill(int64_t nslices, const int64_t *sfirst, const int32_t *slpr, const int64_t *rp,
                     const int32_t *ci, const double *val, int64_t nrows, const int64_t *sptr, uint16_t *dl,
                     double *dv, int32_t *seg, int nsegs /* D16_SEG or D16_SEG_MAX */, hipStream_t st,
                     const int32_t *rowmap = nullptr, const int64_t *rstart = nullptr);
// Shared delta streams: the classes of every slice of a filled layout (cls: nslices * 64;
// cnt: nslices + 1, stored deltas per slice, to be scanned into dptr; *nshared += slices with
// fewer than 64 classes), then the shared stream dls from the plain one dl (kernels.hip)
void launch_d16_share_classes(int64_t nslices, const int64_t *sptr, const uint16_t *dl, uint8_t *cls, int64_t *cnt,
                              int64_t *nshared, hipStream_t st);
void launch_d16_share_fill(int64_t nslices, const int64_t *sptr, const int64_t *dptr, const uint8_t *cls,
                           const uint16_t *dl, uint16_t *dls, hipStream_t st);
// The coupling block of the outer operator: rows [ns, n) x columns [0, ns) of A (sorted
// columns) against the block M the preconditioner multiplies with.  rstart[r] = the first
// entry of row r with a column >= ns where reuse[r], else rp[r]; *differs = 1 when a row's
// coupling entries are not M's row in count, columns and value bits.
void launch_coupling_rows(int64_t n, int64_t ns, const int64_t *rp, const int32_t *ci, const double *val,
                          const int64_t *mrp, const int32_t *mci, const double *mval, const uint8_t *reuse,
                          int64_t *rstart, int32_t *differs, hipStream_t st);
// raw row sums of lane-per-row slices (launch_d16_spmv's aux): stored, or the initial value
constexpr int D16_AUX_NONE = 0, D16_AUX_STORE = 1, D16_AUX_INIT = 2;
// ... and the raw sums of the single lanes of rows served by lpr > 1 lanes, for the rows
// [lo, hi) of the launch's layout: q[(row - lo) * lpr + lane of the row], stored or taken as
// initial values with the same aux mode.  lpr 0: no such rows.
struct D16Wide {
    double *q = nullptr;
    int64_t lo = 0, hi = 0;
    int lpr = 0;
};
void launch_first_col(int64_t nrows, const int64_t *rp, const int32_t *ci, int32_t *c0, hipStream_t st);
// the streams of a D16 layout that a launch reads beside the values (DevSELL::streams fills it)
struct D16Streams {
    const int64_t *sptr, *sfirst;
    const int32_t *slpr;
    const uint16_t *dl;
    const int32_t *seg;
    int nsegs;
    // shared delta stream (pls.d16_share): dl is then addressed through dptr (nslices + 1) and
    // cls (a class per lane); both null: one delta pack per lane at the value stream's offsets
    const int64_t *dptr = nullptr;
    const uint8_t *cls = nullptr;
};
void launch_d16_spmv(int64_t nrows, int64_t nslices, const D16Streams &L, const double *dv, const double *x, double *y,
                     double alpha, double beta, const double *z, int tag, const double *ghost, int64_t nlocal,
                     int unroll /* 8-entry groups per lane in flight: 1, 2 or 4 */,
                     int d16_xcd /* workgroup -> slice order: 0 round-robin over the 8 XCDs, 1 XCD-contiguous
                                    ranges (pls.d16_xcd); it sets the grid rounding and the kernel's map */,
                     hipStream_t st,
                     const int32_t *slist = nullptr /* nslices entries: the slices to process */,
                     const int32_t *rowmap = nullptr /* slice position -> row (SELL-C-sigma) */,
                     size_t lds_reserve = 0 /* dynamic LDS per workgroup, unused: keeps the product's
                                               workgroups off CUs whose LDS a sweep holds */,
                     int aux_mode = D16_AUX_NONE, double *aux = nullptr /* nrows: raw row sums, see D16_AUX_* */,
                     const D16Wide &W = D16Wide());
// Compressed-operator GMRES (pls_gmres_operator single): a D16 layout's values once more in fp32,
// dv32[base + (k / 4) * 256 + lane * 4 + k % 4], rounded to nearest even from the fp64 stream
// (stored: the layout's padded entries; *overflow = 1 when a finite value rounds to an infinity) ...
void launch_d16_round_values(int64_t stored, const double *dv, float *dv32, int32_t *overflow, hipStream_t st);
// ... and launch_d16_spmv over that stream (the same kernel): x, products and sums fp64, in the
// same order.  unroll: 1, 2, 4 or 8; aux_init != null: D16_AUX_INIT (plain layouts on one rank, tag 1)
void launch_d16_spmv(int64_t nrows, int64_t nslices, const D16Streams &L, const float *dv32, const double *x, double *y,
                     double alpha, double beta, const double *z, int tag, const double *ghost, int64_t nlocal,
                     int unroll, int d16_xcd, hipStream_t st, const int32_t *slist = nullptr,
                     const int32_t *rowmap = nullptr, size_t lds_reserve = 0, const double *aux_init = nullptr,
                     const D16Wide &W = D16Wide());
// One smoothing step of BoomerAMG's Jacobi-type and Chebyshev relaxations (boomeramg.cpp):
//   res = b[i] - sum_j a_ij x[j],  dn = a d[i] + g (m[i] res),  x_new[i] = x[i] + dn
// RELAX_READ_D: the a d[i] term is formed (else it is absent, not multiplied by zero);
// RELAX_WRITE_D: d[i] = dn; RELAX_X_ZERO (launch_relax_step only): x is not read, x_new = dn.
// m res and g (m res) are rounded products, a d[i] + . one fma: relax_dn in kernels.hip.
constexpr int RELAX_READ_D = 1, RELAX_WRITE_D = 2, RELAX_X_ZERO = 4;
// ... as one launch over a D16 layout (k_d16_spmv's epilogue D16_AUX_RELAX; fp64 values, no
// ghost columns, no slice list; rowmap allowed).  x_new must not alias x.
constexpr int D16_AUX_RELAX = 3;
void launch_d16_relax(int64_t nrows, int64_t nslices, const D16Streams &L, const double *dv, const double *x,
                      double *x_new, const double *b, const double *m, double *d, double a, double g, int flags,
                      int unroll, int d16_xcd, hipStream_t st, const int32_t *rowmap);
// ... and elementwise from a residual res formed before (any layout): x_new may alias x.
void launch_relax_step(int64_t n, const double *res, const double *x, double *x_new, const double *m, double *d,
                       double a, double g, int flags, hipStream_t st);
// SELL/B3: row triples sharing one column list (FE vector fields), see kernels.hip
void launch_triple_flags(int64_t n, const int64_t *rp, const int32_t *ci, uint8_t *flag, hipStream_t st);
int b3_lanes_per_triple();
void launch_b3_fill(int64_t nslices, int64_t ntrip, const int64_t *bptr, const int32_t *tmap, const int64_t *rp,
                    const int32_t *ci, const double *val, int32_t *bcol, double *bval, hipStream_t st);
void launch_b3_spmv(int64_t nslices, int64_t ntrip, const int64_t *bptr, const int32_t *tmap, const int32_t *bcol,
                    const double *bval, const double *x, double *y, double alpha, double beta, const double *z,
                    int tag, hipStream_t st);
// flag[r] = 1 when row r (sorted columns) references a ghost column (>= nlocal)
void launch_row_has_ghost(int64_t nrows, const int64_t *rp, const int32_t *ci, int64_t nlocal, uint8_t *flag,
                          hipStream_t st);

// Level-aligned SELL-64 triangular factors (see sweep_lds.hip)
void launch_tri_fill(int64_t nslices, const int32_t *slot_row, const int32_t *slot_len, const int64_t *rp,
                     const int32_t *ci, const double *lu, const int64_t *diag, const double *dinv, int upper,
                     const int64_t *sptr, int32_t *ocol, double *oval, double *odinv, hipStream_t st);
void launch_tri_blocks(int64_t nblocks, const int64_t *goff, const int64_t *gslice, const int64_t *sptr,
                       const int32_t *slot_row, const int32_t *slot_len, const int32_t *col, const double *val,
                       const double *sdinv, const double *b, double *y, hipStream_t st);
// one level of a triangular sweep from the factored CSR, 16 lanes per row (sweep_lds.hip)
void launch_tri_csr_level(int64_t m, const int32_t *rows, const int64_t *rp, const int32_t *ci, const double *val,
                          const int64_t *diag, const double *dinv, int upper, const double *b, double *y,
                          hipStream_t st);
void launch_tri_group(int64_t s0, int64_t s1, const int64_t *sptr, const int32_t *slot_row, const int32_t *slot_len,
                      const int32_t *col, const double *val, const double *sdinv, const double *b, double *y,
                      hipStream_t st);

// Block-Jacobi ILU(0) apply, one workgroup per block, levels separated by
// workgroup barriers (forward + backward in one launch).  Block solution
// resident in LDS when every block has <= ilu_lds_max_rows() rows; gmem: kept
// in y instead (blocks of up to ilu_gmem_max_rows() rows).
int ilu_lds_max_rows();
int ilu_gmem_max_rows();
void launch_ilu_blocks_lds(int64_t n, int64_t nblocks, const int64_t *Lgoff, const int64_t *Lgslice,
                           const int64_t *Lsptr, const int32_t *Lcol, const double *Lval, const int32_t *Llpr,
                           const int64_t *Ugoff, const int64_t *Ugslice, const int64_t *Usptr, const int32_t *Ucol,
                           const double *Uval, const int32_t *Ulpr, const double *x, double *y, hipStream_t st,
                           int64_t *prof = nullptr, bool gmem = false, int tpb = 1024, int rr = 0,
                           const int64_t *bstart = nullptr, int64_t max_len = 0, int64_t blk_lo = 0,
                           int64_t blk_hi = -1,  // blocks [blk_lo, blk_hi) only (blk_hi < 0: all)
                           int depth = 2);       // levels in flight: 2, or 6 with tpb <= 512

int ilu_lds_lane_entries();
// super-window sweep (blocks too long for LDS): see kernels.hip
void launch_ilu_blocks_swin(int64_t n, int64_t nblocks, const int64_t *bstart, const int64_t *wstart,
                            const int64_t *Lbsw, const int64_t *Lsw, const int64_t *Lwnear, const int32_t *Lncol,
                            const double *Lnval, const int64_t *Lwfar, const int32_t *Lfcol, const double *Lfval,
                            const double *Ltinv, const int64_t *Ubsw, const int64_t *Usw, const int64_t *Uwnear,
                            const int32_t *Uncol, const double *Unval, const int64_t *Uwfar, const int32_t *Ufcol,
                            const double *Ufval, const double *Utinv, const double *x, double *y, int64_t lds_bytes,
                            hipStream_t st);
int ilu_swin_lds_budget();  // bytes of LDS a super-window's staged inverses + near streams may take
// The chain sweep (kernels.hip, k_ilu_blocks_chain): one wave per LDS-resident
// block walks its slices in order with ilu_chain_depth() slices in flight
// (deep, narrow level DAGs).  Per triangle and block: first slice's entry
// (base), its first slice in the size array sz (soff), the slice count (nsl),
// lanes per row (lpr, 1..ilu_chain_max_lpr()).
int ilu_chain_depth();
int ilu_chain_max_lpr();
void launch_ilu_blocks_chain(int64_t n, int64_t nblocks, const int64_t *bstart, const int64_t *Lbase,
                             const int64_t *Lsoff, const int32_t *Lsz, const int64_t *Lnsl, const int32_t *Llpr,
                             const int32_t *Lcol, const double *Lval, const int64_t *Ubase, const int64_t *Usoff,
                             const int32_t *Usz, const int64_t *Unsl, const int32_t *Ulpr, const int32_t *Ucol,
                             const double *Uval, const double *x, double *y, int64_t max_len, hipStream_t st);
// The window sweep (kernels.hip, k_ilu_blocks_window): LDS-resident blocks in
// windows of 64 rows; per block its first window wstart[b] (nblocks + 1); per
// triangle and window the off-window stream [woff[w], woff[w + 1]) ([k][lane]
// SELL of 12-byte records: value, block-local column) and the window's
// inverse in column pairs,
// tinv[w * 4096 + (k / 2) * 128 + lane * 2 + k % 2].
// The record streams carry ilu_window_stream_pad() entries of padding at
// their end (the staging copies read a fixed count); blocks of at most
// ilu_window_max_rows() rows.
int ilu_window_max_rows();
int ilu_window_stream_pad();
int ilu_window_max_entries();  // off-window entries per row the kernel handles
// The ring variant (ring = true): blocks longer than LDS, up to
// ilu_window_ring_max_rows() rows, y as the block solution and an LDS ring of
// ilu_window_ring_rows() rows for the off-window terms -- no row may depend on
// one more than ilu_window_ring_rows() - 64 rows away (the caller checks)
int ilu_window_ring_rows();
int64_t ilu_window_ring_max_rows();
void launch_ilu_blocks_window(int64_t n, int64_t nblocks, const int64_t *bstart, const int64_t *wstart,
                              const int64_t *Lwoff, const int32_t *Lrec, const double *Ltinv, const int64_t *Uwoff,
                              const int32_t *Urec, const double *Utinv, const double *x, double *y, int64_t max_len,
                              hipStream_t st, int depth = 2, bool ring = false, int tri = 3,
                              int max_entries_L = 32, int max_entries_U = 32);  // (rows' most off-window entries)
int window_records(int max_entries);  // stream records per wave and window (4, 6, 8) for that many entries
// (depth: windows of data in flight, 2 or 3; pls.window_depth; the ring variant: 2;
// tri (ring variant): 1 the L sweep, 2 the U sweep on y (holding L's solution), 3 both)
// The ring sweep (sweep_lds.hip, k_ilu_blocks_ring): blocks of narrow levels whose
// every level has <= ilu_ring_chunk() rows; per triangle chunk tables (coff per
// block, cg first level, cp [start, end) positions), level orders ordL / ordU
// (position -> row), mapUL (U position -> yL index), scratch yL / yU (n each).
int ilu_ring_slots();
int ilu_ring_lane_entries();  // factor entries per lane per pipeline slot of the ring sweep
int ilu_ring_chunk();
void launch_ilu_blocks_ring(int64_t n, int64_t nblocks, const int64_t *Lgoff, const int64_t *Lgslice,
                            const int64_t *Lsptr, const int32_t *Lcol, const double *Lval, const int32_t *Llpr,
                            const int64_t *Ugoff, const int64_t *Ugslice, const int64_t *Usptr, const int32_t *Ucol,
                            const double *Uval, const int32_t *Ulpr, const int64_t *Lcoff, const int64_t *Lcg,
                            const int64_t *Lcp, const int64_t *Ucoff, const int64_t *Ucg, const int64_t *Ucp,
                            const int32_t *ordL, const int32_t *mapUL, const int32_t *ordU, const int64_t *Lfrp,
                            const int32_t *Lfcol, const double *Lfval, const int64_t *Ufrp, const int32_t *Ufcol,
                            const double *Ufval, const double *x, double *y, double *yL, double *yU, hipStream_t st, int tpb = 1024, const int64_t *bstart = nullptr);
// LDS-kernel stream layout (header entry per lane, lanes-per-row slices, block-local columns)
void launch_lds_fill(int64_t nslices, const int32_t *s_start, const int32_t *s_n, const int32_t *s_lpr,
                     const int32_t *order, const int64_t *rp, const int32_t *ci, const double *lu, const int64_t *diag,
                     const double *dinv, int upper, int64_t n, int64_t nb, const int64_t *sptr2, int32_t *ocol,
                     double *oval, hipStream_t st, bool wide = false,
                     const int32_t *posof = nullptr /* ring sweep: row -> block-local level-order position */,
                     const int32_t *row_lo = nullptr /* ring sweep: entries with position < row_lo[row] are far */, const int64_t *bstart = nullptr);

// distribution helpers
void launch_flag_ghosts(int64_t nnz, const int32_t *ci, const int32_t *own, uint8_t *flag, hipStream_t st);
void launch_remap_cols(int64_t nnz, int32_t *ci, const int32_t *gmap, hipStream_t st);
void launch_sort_rows(int64_t n, const int64_t *rp, int32_t *ci, double *val, hipStream_t st);
void launch_pack(int64_t m, const int32_t *idx, const double *x, double *buf, hipStream_t st);   // buf[k] = x[idx[k]]
void launch_unpack(int64_t m, const int32_t *idx, const double *buf, double *x, hipStream_t st); // x[idx[k]] = buf[k]

// ------------------------------------------------- dense exact LU (dense.hip) --
// M: ld x ld row-major (ld = 64 * ceil(n / 64)); pads are identity rows.
void launch_dense_from_csr(int64_t n, int64_t ld, const int64_t *rp, const int32_t *ci, const double *val, double *M,
                           hipStream_t st);
// In place M := M^-1 by blocked Gauss-Jordan; D: 64 x 64 scratch; *fail |= 1 on
// a zero pivot.  With u > 0 and P (n x 64 scratch) each tile column's pivots are
// chosen over rows [64 k, n) by threshold partial pivoting (MUMPS CNTL(1) = u;
// P then holds n x 64 + panel_fast_doubles(): the panel and the fast path's scratch),
// the rows exchanged in M and rowperm (initialised to the identity): M := (Pi M)^-1;
// stats[3] as launch_mf_panel_pivot.  u = 0: no pivoting (rounds 1-5).
void launch_dense_invert(int64_t ld, double *M, double *D, int32_t *fail, hipStream_t st, int64_t n = 0,
                         double *P = nullptr, int32_t *rowperm = nullptr, int32_t *stats = nullptr, double u = 0.0);
// y = M[:n, :n] x  (rowperm: y = M xp, xp[c] = x[rowperm[c]])
void launch_dense_gemv(int64_t n, int64_t ld, const double *M, const double *x, double *y, hipStream_t st,
                       const int32_t *rowperm = nullptr);
// Block-diagonal dense operators (hybrid Gauss-Seidel chunks of the AMG): chunk
// c holds rows [cptr[c], cptr[c+1]) and its ld x ld row-major block at
// M + c ld^2; cof[i] = chunk of row i.  y = blockdiag(M_c) x.
void launch_bdense_gemv(int64_t n, int64_t ld, const int32_t *cof, const int64_t *cptr, const double *M,
                        const double *x, double *y, hipStream_t st);
// rows r < n of the ld x ld block M scaled by d[r]
void launch_dense_rowscale(int64_t n, int64_t ld, const double *d, double *M, hipStream_t st);
// C = A B, all ld x ld row-major (ld a multiple of 64)
void launch_dense_gemm(int64_t ld, const double *A, const double *B, double *C, hipStream_t st);

// ------------------------------------------- multifrontal LU (dense.hip) --
// Frontal matrices of one level of the assembly tree (sparse_lu.cpp): front f
// is a dense ld x ld row-major block (ld = 64 ldt) at W + ws; its first p rows /
// columns are the pivots (padded to 64 pt), the rest the update rows (q real).
struct MFront {
    int64_t ws;
    int32_t ldt, pt, p, q;
};
// identity on the padding pivots [p, 64 pt) of every front
void launch_mf_pad(int nf, const MFront *F, int max_pad, double *W, hipStream_t st);
// W[dst[k]] = val[src[k]] (original entries into their fronts)
void launch_mf_scatter(int64_t m, const int64_t *dst, const int64_t *src, const double *val, double *W,
                       hipStream_t st);
// Extend-add of children's update blocks into their parents (one child per
// parent per launch, so no two children of a parent race).
struct MChild {
    int64_t src_ws, dst_ws, map_off;
    int32_t src_ld, src_pp, dst_ld, q;
};
void launch_mf_extend(int nc, const MChild *C, int max_q, const int32_t *maps, const double *Wprev, double *Wcur,
                      hipStream_t st);
// Step k of the partial Gauss-Jordan elimination of every front's pivot tiles
// (front := [F11^-1, F11^-1 F12; -F21 F11^-1, F22 - F21 F11^-1 F12]); D: nf
// 64 x 64 scratch tiles.  A pivot of magnitude <= tau (after partial pivoting
// inside the tile) is replaced by +-tau and counted in fail[1] (static
// pivoting); with tau = 0 an exact zero pivot sets fail[0] instead.
void launch_mf_gj_step(int nf, const MFront *F, int max_ldt, int k, double *W, double *D, int32_t *fail,
                       double tau, hipStream_t st);
// Threshold partial pivoting (MUMPS CNTL(1) = u) before step k: front f's tile-k
// pivots chosen among its fully-summed rows [64 k, p) (update rows the threshold's
// reference), rows exchanged in W and in rowperm + pst[f] (front-local original
// row per position); P + soff[f]: (p + q) x 64 scratch.  stats: [0] rows
// exchanged, [1] pivots below u x column max (MUMPS would delay them; dflag + pst[f]:
// 1 at those columns), [2] zero columns.  S (nf x panel_fast_doubles() scratch;
// max_rows >= every front's p + q): the parallel fast path for panels that keep
// every diagonal pivot (dense.hip k_panel_tile / k_panel_rows); the one-workgroup
// panel runs only where it does not hold.
void launch_mf_panel_pivot(int nf, const MFront *F, const int64_t *pst, const int64_t *soff, int k, double *W,
                           double *P, int32_t *rowperm, int32_t *stats, double u, hipStream_t st,
                           int32_t *dflag = nullptr, double *S = nullptr, int64_t max_rows = 0);
int panel_fast_doubles();
// Persistent factors: rows [0, 64 pt) of the front (U part, ld wide) to U + uoff
// and rows [64 pt, 64 pt + q) x columns [0, 64 pt) (X part) to X + xoff.
struct MStore {
    int64_t uoff, xoff;
};
void launch_mf_store(int nf, const MFront *F, const MStore *S, int max_rows, const double *W, double *U, double *X,
                     hipStream_t st);
// Solve (ND order).  Per front: pivots at z/x[pstart, +p), update rows = slist[soff, +q).
struct MSolve {
    int64_t pstart, qoff, uoff, xoff, soff;
    int32_t p, q, pp, ld;
};
// forward, gather: level row k = (front rf[k], local row rl[k]); v = b (pivot rows) +
// the children's contributions cu[cidx[cptr[k] ..]]; pivot rows -> z, update rows -> acc
void launch_mf_fwd_gather(int64_t m, const int32_t *rf, const int32_t *rl, const MSolve *S, const int64_t *cptr,
                          const int64_t *cidx, const double *b, const double *cu, double *z, double *acc,
                          hipStream_t st);
// forward, update rows: cu = acc + X z_p (one wave per row)
void launch_mf_fwd_gemv(int64_t m, const int32_t *rf, const int32_t *rl, const MSolve *S, const double *X,
                        const double *z, const double *acc, double *cu, hipStream_t st);
// backward, pivot rows: x_p = F11^-1 z_p - G12 x(slist) (one wave per row)
void launch_mf_bwd(int64_t m, const int32_t *rf, const int32_t *rl, const MSolve *S, const double *U,
                   const int32_t *slist, const double *z, double *x, hipStream_t st);
// y[perm[i]] = x[i] / x[i] = b[perm[i]]
void launch_gather_i32(int64_t n, const int32_t *perm, const double *b, double *x, hipStream_t st);
void launch_scatter_i32(int64_t n, const int32_t *perm, const double *x, double *y, hipStream_t st);

// ------------------------------------------------- banded exact LU (band.hip) --
// T: nb tile rows x (bl + bu + 1) tiles of 64 x 64 (see band.hip); padding
// rows past n are identity rows.
void launch_band_from_csr(int64_t n, int64_t nb, int64_t bl, int64_t bu, const int64_t *rp, const int32_t *ci,
                          const double *val, double *T, hipStream_t st);
// In place LU without pivoting; Dl / Du: nb inverted diagonal triangles;
// Gl[I] = Dl_I L_{I,I-1}, Gu[I] = Du_I U_{I,I+1} (the sweeps' near tiles);
// *fail |= 1 on a zero pivot.
void launch_band_factor(int64_t nb, int64_t bl, int64_t bu, double *T, double *Dl, double *Du, double *Gl,
                        double *Gu, int32_t *fail, hipStream_t st);
// One triangular sweep (upper 0: L with Dl, Gl; 1: U with Du, Gu), y != b.
// Gr: 128 tagged granules per tile row (zeroed once); epoch: fresh per sweep,
// never 0; ticket_base: tickets drawn by earlier sweeps (band_sweep_tickets
// per sweep) on `ticket`; *fail |= 2 if a spin gave up.
int64_t band_sweep_tickets(int64_t nb);
void launch_band_sweep(int64_t n, int64_t nb, int64_t bl, int64_t bu, const double *T, const double *Dinv,
                       const double *Gn, const double *b, double *y, uint64_t *Gr, uint64_t *ticket,
                       uint64_t ticket_base, uint32_t epoch, int upper, int32_t *fail, hipStream_t st, int64_t plen = 0);
// SPIKE partitioned sweeps (band.hip): spikes W (nb x bw tiles) of a triangle
// (upper = 0: L / Dl, bw = bl; 1: U / Du, bw = bu) for partitions of plen
// positions; apply = the corrections after a launch_band_sweep(..., plen).
void launch_spike_setup(int64_t nb, int64_t bl, int64_t bu, int upper, int64_t plen, const double *T,
                        const double *Dinv, double *Wt, hipStream_t st);
void launch_spike_apply(int64_t n, int64_t nb, int64_t bw, int upper, int64_t plen, const double *Wt, double *y,
                        double *scratch, hipStream_t st);
int64_t spike_scratch_doubles(int64_t bw);  // scratch of launch_spike_apply

// --------------------------------------- overlapping additive Schwarz (asm.hip) --
// Subdomain growth: `grid` workgroups (at most ASM_GROW_GRID), each with 3 x nw words of `bits`
// (nw = (n + 31) / 32; zero on entry, left zero).  fill false: cnt[b] = |I_b|; fill true:
// rows[ptr[b] ..] = I_b ascending and own = 1 on the rows of the block's own range.
static constexpr int ASM_GROW_GRID = 256;
void launch_asm_grow(bool fill, int grid, int64_t n, int64_t nb, int overlap, const int64_t *rp, const int32_t *ci,
                     unsigned *bits, int64_t nw, int64_t *cnt, const int64_t *ptr, int32_t *rows, uint8_t *own,
                     hipStream_t st);
// The extended matrix: row e = row rows[e] of M restricted to its block's set, columns renumbered to
// extended positions (ascending).  fill false: len[e]; fill true: eci / eval at erp[e].
void launch_asm_extend(bool fill, int64_t ne, int64_t n, int64_t nb, const int64_t *ptr, const int32_t *rows,
                       const int64_t *rp, const int32_t *ci, const double *val, int64_t *len, const int64_t *erp,
                       int32_t *eci, double *eval, hipStream_t st);
// Per global row its extended positions in ascending block order (tptr from the scan of cnt), and
// opos[r], the position that owns row r.
void launch_asm_transpose_count(int64_t ne, const int32_t *rows, const uint8_t *own, int64_t *cnt, int32_t *opos,
                                hipStream_t st);
void launch_asm_transpose_fill(int64_t ne, int64_t n, const int32_t *rows, const int64_t *tptr, int32_t *cursor,
                               int32_t *tpos, hipStream_t st);
void launch_asm_gather(int64_t ne, const int32_t *gidx, const uint8_t *own, int mask_in, const double *x, double *xe,
                       hipStream_t st);
void launch_asm_combine(int64_t n, int mask_out, const int32_t *opos, const int64_t *tptr, const int32_t *tpos,
                        const double *ye, double *y, hipStream_t st);
// The fused application over LDS-resident subdomains (sweep_lds.hip, beside k_ilu_blocks_lds whose
// sweep_block it calls): gather through gidx with the input mask, both sweeps, then owned rows
// straight to y[gidx[e]] (direct) or every row to y[e] (the extended vector; k_asm_combine follows).
void launch_asm_blocks_lds(int64_t nblocks, const int64_t *bstart, int64_t max_len, const int64_t *Lgoff,
                           const int64_t *Lgslice, const int64_t *Lsptr, const int32_t *Lcol, const double *Lval,
                           const int32_t *Llpr, const int64_t *Ugoff, const int64_t *Ugslice, const int64_t *Usptr,
                           const int32_t *Ucol, const double *Uval, const int32_t *Ulpr, const int32_t *gidx,
                           const uint8_t *own, int mask_in, int direct, const double *x, double *y, int tpb, int rr,
                           hipStream_t st);

}  // namespace pls
