/*
 * pls.h -- C-ABI of the MI355X-native block-preconditioned Krylov solver
 * ("pls" = poroelastic linear solver).  Plain pointers and sizes, no torch or
 * PETSc types.  Every entry point returns 0 on success and a nonzero status on
 * failure; pls_last_error() then returns a thread-local message (the Python
 * facade raises RuntimeError with it).
 *
 * Which reference interface each entry point replaces (reference = the
 * nabw/poroelasticity-linear-solvers tree):
 *
 *   pls_create          Preconditioner(index_map, A, P, P_diff, parameters,
 *                       bcs_sub_pressure)      lib/Preconditioner.py:263-276
 *                       + Solver(A, b, PC, parameters, index_map)
 *                                               lib/Solver.py:54-62
 *                       + IndexSet contract     lib/IndexSet.py:29-67
 *   pls_setup           Preconditioner.get_pc() -> PreconditionerCC.setUp
 *                                               lib/Preconditioner.py:120-139,282-291
 *                       + Solver.create_solver  lib/Solver.py:64-103
 *   pls_pc_apply        PreconditionerCC.apply(pc, x, y)
 *                                               lib/Preconditioner.py:141-250
 *   pls_solve           Solver.solve(b, x) -> KSPSolve / AAR.solve
 *                                               lib/Solver.py:148-152, lib/AAR.py:46-128
 *   pls_get_result      Solver.getIterationNumber / KSPGetConvergedReason /
 *                       residual history        lib/Solver.py:145-146
 *   pls_get_timings     PreconditionerCC.print_timings / Solver.print_timings
 *                                               lib/Preconditioner.py:252-260, lib/Solver.py:154-155
 *   pls_destroy         (object lifetime; PETSc XXXDestroy)
 *
 * Device-resident variants (inputs already in HBM, field-major order) exist
 * for benchmarks and for the synthetic generator of SURVEY.md 8(d).
 */
#ifndef PLS_H
#define PLS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLS_ABI_VERSION 1

/* Host CSR (local rows): row_ptr[nrows+1] int64, col[nnz] int32, val[nnz] f64.
 * Columns inside a row must be sorted ascending (PETSc AIJ convention).       */
typedef struct pls_csr {
    int64_t nrows;
    int64_t ncols;
    const int64_t *row_ptr;
    const int32_t *col;
    const double *val;
} pls_csr;

typedef struct pls_handle pls_handle;
typedef struct pls_comm pls_comm;

/* Host allgather callback: every rank passes `bytes` bytes, receives
 * size * bytes (rank order) into recv.  Returns 0 on success.               */
typedef int (*pls_allgather_fn)(const void *send, int64_t bytes, void *recv, void *user);

/* Result of the last solve (KSPGetIterationNumber / KSPGetConvergedReason /
 * residual history as KSPSetResidualHistory records it).                      */
typedef struct pls_result {
    int32_t its;          /* outer iterations                                   */
    int32_t reason;       /* KSPConvergedReason value (AAR: 2 rtol, 3 atol, -3 its) */
    double rnorm;         /* last residual norm the outer solver tested        */
    int32_t pc_applies;   /* block-PC applications during the solve            */
    int32_t history_len;  /* entries available through pls_get_history         */
} pls_result;

/* Accumulated timers in seconds (names of lib/Preconditioner.py:35-39 and
 * lib/Solver.py:62), measured with HIP events on the solver stream.         */
typedef struct pls_timings {
    double pc_total;      /* t_total  */
    double pc_solid;      /* t_solid  */
    double pc_fluid;      /* t_fluid  */
    double pc_press;      /* t_press  */
    double pc_alloc;      /* t_alloc (field gathers/scatters; 0 in field-major layout) */
    double solver_total;  /* Solver.t_total */
    double spmv_total;    /* outer MatMult time */
    int64_t spmv_calls;
} pls_timings;

/* Synthetic 3-field system; generated directly in HBM.     */
typedef struct pls_synth_spec {
    int32_t dim;          /* 2 or 3                                            */
    int32_t N;            /* elements per side                                 */
    uint64_t seed;
    double delta;         /* diagonal shift                                    */
} pls_synth_spec;

int pls_abi_version(void);
const char *pls_last_error(void);
int pls_device_count(int *count);
int pls_set_device(int device);

/* Options: newline-separated "key value" (or "key") lines.  Keys prefixed
 * "pls." are the reference's parameter dict entries ("pls.solver_type gmres",
 * "pls.pc_type diagonal", "pls.inner_ksp_type preonly", ...); every other key
 * is a PETSc options-database entry without its leading '-' ("s_pc_type ilu",
 * "global_ksp_pc_side right", ...), resolved with setFromOptions precedence.
 * KSP types ("pls.solver_type", "pls.inner_ksp_type", "<prefix>ksp_type" for
 * global_ s_ f_ p_ diff_ fp_ fp_fieldsplit_{0,1}_): gmres, fgmres (right
 * preconditioning only; "<prefix>ksp_gmres_restart", default 30), cg, bcgs
 * (left or right), preonly; "pls.solver_type" also takes aar.  Any other type
 * is an error that lists these.  "pls.bcgs_device 0" keeps BiCGStab's scalars
 * on the host, "pls.bcgs_fused_reduce 0" gives its sums a final launch of
 * their own (both bitwise the default).
 * gmres and fgmres orthogonalise with classical Gram-Schmidt
 * ("<prefix>ksp_gmres_classicalgramschmidt", the default), refined as
 * "<prefix>ksp_gmres_cgs_refinement_type" says (refine_never, the default,
 * refine_ifneeded, refine_always; anything else is an error), or with modified
 * Gram-Schmidt ("<prefix>ksp_gmres_modifiedgramschmidt", which wins over the
 * classical flag, as in PETSc, and ignores the refinement type).  Other KSP
 * types ignore the three.  "pls.gmres_mgs_fused 1" finishes each modified
 * Gram-Schmidt sum in the step's own launch (one rank; bitwise the default).
 * Levels of fill: "<prefix>pc_factor_levels k" for pc_type ilu and
 * "<prefix>sub_pc_factor_levels k" for bjacobi's ilu blocks (each block's own
 * truncated matrix) factor on PETSc's ILU(k) pattern (natural ordering, sum
 * rule; built on the device); k = 0, the default, is ILU(0).  A negative or
 * non-integer k is an error that names the key; so are a filled row longer
 * than the factorization stages and a filled pattern beyond the free device
 * memory.  pls_get_ilu_fill reports the fill.
 * Dirichlet columns: "<prefix>pls_bc_columns keep | lift | drop" for the inner
 * prefixes s_ f_ p_ diff_ fp_ fp_fieldsplit_{0,1}_ (keep, the default, builds
 * nothing; any other value is an error that lists the three).  A row of the
 * block whose stored diagonal is 1.0 exactly and whose other stored values are
 * all 0.0 is a constrained row, as dolfin's bc.apply leaves it.  lift and drop
 * give the KSP a copy K' of its block with every value in a constrained column
 * outside that column's own row set to 0.0 (the pattern is kept); operator, PC
 * and SpMV layout are built from K'.  lift also keeps the moved nonzeros C and
 * starts every solve of that KSP with b' = b - C b, which solves the block as
 * given: K^-1 b = K'^-1 (b - C b).  drop applies no correction and is another
 * preconditioner.  Refused, naming the key: a KSP that was handed its PC (fp_
 * over a fieldsplit: use fp_fieldsplit_{0,1}_), an operator that is not a
 * stored matrix (the Schur split), operator and preconditioner matrices that
 * differ, a sharded block.  pls_update_matrices detects and splits again.
 * pls_get_bc_columns_stats / pls_get_bc_columns_matrix report the split.
 * BoomerAMG smoothers: "<prefix>pc_hypre_boomeramg_relax_type_all" takes
 * symmetric-SOR/Jacobi (the default: hybrid symmetric Gauss-Seidel), Jacobi,
 * l1scaled-Jacobi or Chebyshev; any other value is an error that lists the
 * four.  On a level with operator A: Jacobi m_i = w / a_ii with w =
 * "<prefix>pc_hypre_boomeramg_relax_weight_all" (default 1.0), l1scaled-Jacobi
 * m_i = sign(a_ii) / sum_j |a_ij| (m_i = 1 where the denominator is zero); a
 * sweep over a set I (all rows with no_CF, else C then F going down and F then
 * C going up) is x += M_I (b - A x), grid_sweeps_all rounds of it.  Chebyshev
 * ignores the C/F sets: each round is "<prefix>pls_boomeramg_chebyshev_order"
 * (1-4, default 2) steps of the Jacobi-preconditioned Chebyshev recurrence on
 * [f lmax, lmax], lmax = 1.1 x the power-iteration estimate of D^-1 A (15
 * steps, rounded to fp32), f = "<prefix>pls_boomeramg_chebyshev_fraction" (in
 * (0, 1), default 0.3).  Out-of-range values are errors that name the key; so
 * is a sharded block with a type other than the default; the three keys are
 * checked whatever the type.  Every step is one launch over a level whose
 * layout is SELL-64/D16 without an RCM relabelling or a SELL/B3 part; other
 * levels, and "pls.amg_relax_fused 0", run the residual and an elementwise
 * step (the same bits).  The three need a symmetric block to
 * keep CG's preconditioner symmetric ("<prefix>pls_bc_columns lift").
 * pls_get_boomeramg_relax reports the smoother.                              */

/* Build a solver from host CSR matrices in the caller's (e.g. dolfin
 * interleaved) ordering plus the field index sets (sorted global indices of
 * each field, lib/IndexSet.py:38-41).  Pdiff may be NULL unless pc type is a
 * 3-way variant.  bcs_sub_p: positions inside the p sub-vector with pressure
 * Dirichlet BCs (lib/Poromechanics.py:48-55).                               */
int pls_create(const pls_csr *A, const pls_csr *P, const pls_csr *Pdiff,
               const int32_t *is_s, int64_t ns, const int32_t *is_f, int64_t nf,
               const int32_t *is_p, int64_t np, const int32_t *bcs_sub_p, int64_t nbc,
               const char *options, pls_handle **out);

/* Build a solver whose A, P, P_diff, index sets and pressure BCs come from the
 * seeded synthetic generator, directly on the device, field-major order.     */
int pls_create_synthetic(const pls_synth_spec *spec, const char *options, pls_handle **out);

/* ---- distributed solve (one process per GPU) ----------
 * Row slabs per field (PETSc ownership split), halo exchange before each
 * SpMV, deterministic global sums (allgather + rank-ordered sum), block-Jacobi
 * inner blocks per rank.  Replaces the reference's MPI data parallelism
 * (mpirun -np 8, paper-scripts/robustness_2d.sh:29; PETSc MPIAIJ + VecScatter,
 * lib/Solver.py:151, lib/Preconditioner.py:170-234).                        */
int pls_rccl_unique_id(char out[128]);
int pls_comm_create_rccl(const char id[128], int rank, int size, pls_comm **out);
int pls_comm_create_callback(int rank, int size, pls_allgather_fn fn, void *user, pls_comm **out);
int pls_comm_destroy(pls_comm *comm);
/* Each rank generates and owns its slabs of the synthetic system; the handle
 * must be destroyed before its communicator.  Vectors of the device entry
 * points are rank-local ([s_r | f_r | p_r]).                                 */
int pls_create_synthetic_dist(const pls_synth_spec *spec, const char *options, pls_comm *comm, pls_handle **out);
/* Mean latency of one global sum of `count` doubles (allgather + rank-ordered
 * sum + the stream sync the Krylov loop performs), over `reps` calls; the
 * reference's MPI_Allreduce inside VecMDot / VecNorm.                       */
int pls_bench_global_sum(pls_handle *h, int32_t count, int32_t reps, double *sec_per_call);
/* Multi-rank pls_create from the caller's matrices -- what the reference
 * drivers hold under mpirun (paper-scripts/robustness_2d.sh:29): on every rank
 * A, P, P_diff are the rank's MPIAIJ rows (A.getValuesCSR() of the operator of
 * lib/Solver.py:151: nrows = this rank's rows, ncols = the global n, global
 * column indices), rows [row_start, row_start + ns + nf + np) of the global
 * (dolfin) numbering; is_s / is_f / is_p are the global indices of the dofs
 * this rank owns (dofmap().dofs(), lib/IndexSet.py:38-41; 2-way: fp = their
 * sorted union, the all-gather of lib/IndexSet.py:49 happens inside);
 * bcs_sub_p = positions inside this rank's p sub-vector
 * (lib/Poromechanics.py:48-55).  Field blocks take the row ownership of the
 * rank-local index sets, as PETSc's createSubMatrix (lib/Preconditioner.py:
 * 61-74) gives them.  Collective over comm; host vectors of pls_solve /
 * pls_pc_apply / pls_matmult are this rank's rows in the caller's order.   */
int pls_create_dist(const pls_csr *A, const pls_csr *P, const pls_csr *Pdiff, int64_t row_start, const int32_t *is_s,
                    int64_t ns, const int32_t *is_f, int64_t nf, const int32_t *is_p, int64_t np,
                    const int32_t *bcs_sub_p, int64_t nbc, const char *options, pls_comm *comm, pls_handle **out);

int pls_setup(pls_handle *h);
/* New values (or patterns) of A / P / P_diff (NULL: unchanged), caller's
 * ordering as in pls_create.  The block PC is set up again before the next
 * solve -- PETSc's PCSetUp on an operator state change, which the reference
 * triggers every time step by re-applying BCs to A and P
 * (lib/Poromechanics.py:70-86, lib/Solver.py:105 set_up).  Outer solver,
 * AAR and inner Anderson histories persist, as the reference's objects do;
 * so does the outer solver's Fischer guess space (-global_ksp_guess_type
 * fischer) unless A is non-NULL: a new A empties it and counts a reset
 * (PETSc's operator-state check).  Inner solvers are built again, their
 * guess spaces with them.                                                  */
int pls_update_matrices(pls_handle *h, const pls_csr *A, const pls_csr *P, const pls_csr *P_diff);
/* Set / override one option ("key", "value" or NULL for a flag).  Options of
 * the outer solver ("pls.solver_*", "pls.aar_*", "global_*") may change until
 * pls_create_solver (or the first solve); PC options until pls_setup.        */
int pls_set_option(pls_handle *h, const char *key, const char *value);
/* Solver.create_solver (lib/Solver.py:64-103): build the outer KSP / AAR.    */
int pls_create_solver(pls_handle *h);
int pls_destroy(pls_handle *h);

/* Global size n and field sizes of a handle.                                 */
int pls_get_sizes(pls_handle *h, int64_t *n, int64_t *ns, int64_t *nf, int64_t *np, int64_t *nnz_A);

/* Host-vector entry points (caller's ordering, length n).  pls_solve and
 * pls_solve_device write x; they also read it, as the initial guess, when
 * -global_ksp_initial_guess_nonzero is set and -global_ksp_guess_type is
 * none -- and only then (a Fischer guess is formed from b alone).           */
int pls_pc_apply(pls_handle *h, const double *x, double *y);
int pls_solve(pls_handle *h, const double *b, double *x, pls_result *res);
int pls_matmult(pls_handle *h, const double *x, double *y);
/* y = A^ x with the low-precision copy of the outer operator that
 * -<prefix>pls_gmres_operator single multiplies with: A's SELL-64/D16 layout,
 * every stored value rounded to nearest-even fp32 once (the fp32 stream is
 * built on demand); x, y, every product and every sum are fp64.  An error
 * when A's layout is int32 SELL-64 or CSR, has a SELL/B3 part, or holds a
 * finite value that is infinite in fp32.                                     */
int pls_matmult_single(pls_handle *h, const double *x, double *y);

/* Device-vector entry points: d_b / d_x are device pointers in the handle's
 * internal field-major order (no host traffic, no permutation).             */
int pls_solve_device(pls_handle *h, const double *d_b, double *d_x, pls_result *res);
int pls_pc_apply_device(pls_handle *h, const double *d_x, double *d_y);
int pls_matmult_device(pls_handle *h, const double *d_x, double *d_y);
/* pls_matmult_single on device vectors (with pls.reuse_coupling_probe and an
 * outer solver with pls_gmres_operator single: the low product as GMRES forms
 * it after a preconditioner application).                                    */
int pls_matmult_single_device(pls_handle *h, const double *d_x, double *d_y);
/* Synthetic right-hand side (field-major) written to a device vector.        */
int pls_synthetic_rhs_device(pls_handle *h, uint64_t seed, double *d_b);
/* Device buffer helpers (so hosts without a GPU runtime binding can drive it) */
int pls_device_alloc(int64_t bytes, void **d_ptr);
int pls_device_free(void *d_ptr);
int pls_memcpy_h2d(void *d_dst, const void *h_src, int64_t bytes);
int pls_memcpy_d2h(void *h_dst, const void *d_src, int64_t bytes);

int pls_get_result(pls_handle *h, pls_result *res);
int pls_get_history(pls_handle *h, double *hist, int32_t cap);
int pls_get_timings(pls_handle *h, pls_timings *t);
int pls_reset_timings(pls_handle *h);
/* Totals of one inner (or the outer) KSP since the handle's setup, by options
 * prefix ("s_", "f_", "p_", "diff_", "fp_", "fp_fieldsplit_0_", ..., "global_"):
 * stats[0] solves, [1] iterations, [2] most iterations of one solve, [3] solves
 * that ended with a negative KSPConvergedReason (PETSc's -ksp_converged_reason
 * per solve, summed; the reference's own output is the outer count only,
 * lib/AbstractPhysics.py:77-78), [4] the most recent such reason (0: none).  */
int pls_get_ksp_stats(pls_handle *h, const char *prefix, int64_t stats[5]);
/* The orthogonalisation of the gmres / fgmres KSP with this prefix since setup:
 * stats[0] Arnoldi steps orthogonalised, [1] second classical Gram-Schmidt
 * passes performed, [2] the scheme (0 CGS refine_never, 1 refine_ifneeded,
 * 2 refine_always, 3 modified Gram-Schmidt).  An unknown prefix or a KSP of
 * another type is an error.                                                 */
int pls_get_gmres_orthog_stats(pls_handle *h, const char *prefix, int64_t stats[3]);
/* The Krylov basis of the gmres / fgmres KSP with this prefix
 * (<prefix>pls_gmres_basis): stats[0] its precision (0 double, 1 single),
 * [1] bytes of the basis allocation, and since setup [2] cycles ended because
 * the estimate had fallen by <prefix>pls_gmres_basis_drop, [3] converged
 * estimates confirmed against the true residual at the next cycle start,
 * [4] confirmations that failed and led to another cycle ([2]-[4] stay 0 with
 * a double basis).  An unknown prefix or a KSP of another type is an error.  */
int pls_get_gmres_basis_stats(pls_handle *h, const char *prefix, int64_t stats[5]);
/* The operator inside the Arnoldi step of the gmres / fgmres KSP with this
 * prefix (<prefix>pls_gmres_operator, with <prefix>pls_gmres_basis single
 * only): stats[0] its precision (0 double, 1 single), [1] bytes of the fp32
 * value streams its operator holds (the reduced layout of the coupling reuse
 * included), and since setup [2] products with the low-precision operator,
 * [3] fp64 products (cycle-start residuals, the guesses' products; with a
 * double operator also the Arnoldi products of the fp32-basis cycle).  An
 * unknown prefix or a KSP of another type is an error.                       */
int pls_get_gmres_operator_stats(pls_handle *h, const char *prefix, int64_t stats[4]);
/* The initial guess of the KSP with this prefix (-<prefix>ksp_guess_type
 * none|fischer, -<prefix>ksp_guess_fischer_model 2,<size>,
 * -<prefix>ksp_guess_fischer_tol; -global_ksp_initial_guess_nonzero for the
 * outer solver).  Fischer's model 2, the least-squares projection valid for a
 * nonsymmetric operator, is the only model built and the default here
 * (PETSc's default is model 1, which needs a symmetric operator).  stats[0]
 * type (0 none, 1 fischer), [1] columns stored now, [2] size, and since setup
 * [3] guesses formed, [4] updates skipped (the new direction was dependent),
 * [5] resets (the space was full, or A changed).  *last_reduction:
 * ||b - A x0|| / ||b|| of the most recent solve that started from a guess,
 * NaN before the first and for b = 0 (where rnorm0 is the first residual's,
 * as from a zero guess).  An unknown prefix is an error.                     */
int pls_get_ksp_guess_stats(pls_handle *h, const char *prefix, int64_t stats[6], double *last_reduction);
/* What the callers of pls_solve need to know about the KSP with this prefix,
 * from the library's own reading of the options (the solver is created if it
 * was not yet): *reads_x = 1 when x is an input of the solve -- the prefix is
 * "global_", -global_ksp_initial_guess_nonzero is set and no Fischer guess
 * replaces it -- else 0 (also with pls.solver_type aar); *seconds = HIP-event
 * time the most recent solve spent on its guess (forming x0, r0 = b - A x0 and
 * the norms before the zero-guess solve, x = x0 + d and the space's update
 * after it) with pls.ksp_guess_timing 1, else NaN.                          */
int pls_get_ksp_guess_info(pls_handle *h, const char *prefix, int64_t *reads_x, double *seconds);
/* Coupling reuse (option pls.reuse_coupling): products with the outer operator
 * since the last pls_reset_timings, [0] reduced ones that continued the block
 * preconditioner's coupling product, [1] full ones; [2] 1 when the reduced
 * path is eligible for the next solve (decided when the solver is created and
 * again after pls_update_matrices), else 0.                                  */
int pls_get_reuse_stats(pls_handle *h, int64_t stats[3]);
/* The rows of the coupling reuse by kind (zeros while not eligible): stats[0]
 * rows served by several lanes whose sums are continued lane by lane (option
 * pls.reuse_wide: -1 wherever the reuse is eligible, 0 never), [1] their lanes
 * per row, [2] the lane-per-row reuse rows, [3] the bytes one reduced outer
 * product streams from its layout.                                           */
int pls_get_reuse_wide(pls_handle *h, int64_t stats[4]);
/* The rows of the coupling reuse: mask[i] = 1 (n bytes, the caller's row
 * order) where the reduced outer product starts row i from the block
 * preconditioner's raw sum, all 0 while the reduced path is not eligible.    */
int pls_get_reuse_rows(pls_handle *h, uint8_t *mask);
/* The eigenvalue bounds of the chebyshev KSP with this prefix: out[0] emin and
 * [1] emax as used, [2] the smallest and [3] the largest real part of the
 * estimate's Hessenberg eigenvalues (NaN when the bounds were given with
 * <prefix>ksp_chebyshev_eigenvalues).  An unknown prefix, a KSP of another type
 * or one that has not run a solve since it was set up is an error.           */
int pls_get_chebyshev_bounds(pls_handle *h, const char *prefix, double out[4]);
/* Levels of fill of the ilu / bjacobi(ilu) PC of the KSP with this prefix:
 * stats[0] the levels k (<prefix>pc_factor_levels, <prefix>sub_pc_factor_levels),
 * [1] stored entries of the (block-truncated) matrix before the fill, [2] after
 * it (the factors' entries), [3] the longest filled row.  With k = 0, [2] = [1].
 * An unknown prefix, or a PC that is not ILU / BJACOBI(ILU), is an error.     */
int pls_get_ilu_fill(pls_handle *h, const char *prefix, int64_t stats[4]);
/* The overlapping additive Schwarz PC (<prefix>pc_type asm) of the KSP with this
 * prefix: stats[0] blocks (<prefix>pc_asm_blocks), [1] overlap
 * (<prefix>pc_asm_overlap), [2] <prefix>pc_asm_type as 0 restrict, 1 basic,
 * 2 interpolate, 3 none, [3] the rows of all subdomains together, [4] the rows
 * of the largest, [5] 1 when the fused kernel serves the application (the
 * subdomains fit LDS and pls.asm_fused is not 0), else 0.  An unknown prefix,
 * or a PC that is not asm, is an error.                                      */
int pls_get_asm_stats(pls_handle *h, const char *prefix, int64_t stats[6]);
/* Its subdomains: ptr[blocks + 1] offsets into rows[stats[3]], each subdomain's
 * rows ascending, numbered within the block the prefix solves (field-major
 * order).  rows may be NULL to read the offsets alone.                       */
int pls_get_asm_rows(pls_handle *h, const char *prefix, int64_t *ptr, int32_t *rows);
/* The Dirichlet-column split (<prefix>pls_bc_columns) of the KSP with this
 * prefix: stats[0] the mode, 0 keep, 1 lift, 2 drop, [1] the constrained rows
 * found, [2] the entries moved to C, [3] the rows of C, [4] the bytes the KSP
 * holds for K', C and (lift) the row map and b'.  With keep [1]-[4] are 0; a
 * block in which nothing moves is not copied ([4] is then the row list's
 * 4 x [1] bytes).  Sets the preconditioner up if
 * it was not yet.  An unknown prefix is an error.                             */
int pls_get_bc_columns_stats(pls_handle *h, const char *prefix, int64_t stats[5]);
/* The split itself: bc_rows[stats[1]] the constrained rows, ascending; C as CSR
 * over all rows of the block, c_rp[n + 1], c_ci[stats[2]], c_val[stats[2]],
 * columns ascending.  Rows and columns are numbered within the block the prefix
 * solves (field-major order).  Any pointer may be NULL.                       */
int pls_get_bc_columns_matrix(pls_handle *h, const char *prefix, int32_t *bc_rows, int64_t *c_rp, int32_t *c_ci,
                              double *c_val);
/* The smoother of the BoomerAMG stand-in (<prefix>pc_type hypre) of the KSP with
 * this prefix: stats[0] the relax type, 0 symmetric-SOR/Jacobi, 1 Jacobi,
 * 2 l1scaled-Jacobi, 3 Chebyshev, [1] the smoothed levels, [2] the Chebyshev
 * order, [3] the levels whose steps are the fused launch, and for the most
 * recent application [4] fused step launches, [5] elementwise step launches
 * (the steps from a zero iterate, and those of the other levels).  lambda[l],
 * l < cap: level l's eigenvalue estimate (0 for the other types and past the
 * last level); may be NULL with cap 0.  Sets the preconditioner up if it was
 * not yet.  An unknown prefix, or a PC that is not that AMG, is an error.     */
int pls_get_boomeramg_relax(pls_handle *h, const char *prefix, int64_t stats[6], double *lambda, int32_t cap);
/* One smoothing step of those relax types on the outer operator A, in the
 * layout pls_matmult multiplies with (a diagnostic; host vectors of length n,
 * the caller's order): x_new = x + dn, dn = a d + g (m (b - A x)), d = dn.
 * d may be NULL: the a d term is then absent and nothing is stored.  fused 1
 * asks for the single launch, which serves SELL-64/D16 layouts without an RCM
 * relabelling or a SELL/B3 part; *was_fused says whether it ran, else the
 * product and an elementwise step did.                                       */
int pls_relax_step(pls_handle *h, const double *m, const double *b, const double *x, double *d, double a, double g,
                   int32_t fused, double *x_new, int32_t *was_fused);
/* Eigenvalues of the leading m x m part (1 <= m <= 64) of an upper Hessenberg
 * matrix stored by columns, H[i + j * ldh]; entries below the subdiagonal are
 * not read.  Host code (shifted QR, no LAPACK, no device): re[k] + i im[k], in
 * no particular order.  Returns nonzero when the iteration does not converge
 * or an argument is out of range (no error message is set).                  */
int pls_hessenberg_eigenvalues(int m, const double *H, int ldh, double *re, double *im);

/* Export a device matrix of the handle to host CSR (tests / parity):
 * which: 0 = A, 1 = P, 2 = P_diff (field-major order).  Call once with
 * col == NULL to get nrows/nnz, then with buffers sized accordingly.        */
int pls_export_matrix(pls_handle *h, int which, int64_t *nrows, int64_t *nnz,
                      int64_t *row_ptr, int32_t *col, double *val);
/* Export the field-major permutation: perm[internal] = caller index.         */
int pls_get_permutation(pls_handle *h, int64_t *perm);

/* Host-only query of the classical AMG behind -pc_type hypre (no device
 * needed; test and inspection entry): level `level` of the hierarchy that
 * options' <prefix>pc_hypre_boomeramg_* build from A (petsc-options-inexact:
 * 16-24): n, nc, nnz of P (of the coarsest operator when level ==
 * *nlevels - 1); when non-NULL, cf[n] (1 C / -1 F) and P's CSR arrays
 * (p_rp[n + 1], p_ci[nnz], p_v[nnz]).                                        */
int pls_boomeramg_host_level(const pls_csr *A, const char *options, const char *prefix, int64_t level,
                             int64_t *nlevels, int64_t *n, int64_t *nc, int64_t *p_nnz, int8_t *cf, int64_t *p_rp,
                             int32_t *p_ci, double *p_v);

/* Host-only analysis of the sparse LU (the MUMPS stand-in behind -pc_type lu
 * past pls.lu_dense_max rows; petsc-options-exact:11-35,
 * petsc-options-inexact:105-106) that `options` would build on A: ordering
 * (pls.lu_nd*) and symbolic factorization only, no device needed.
 * stats[0..9]: n, fronts, tree levels, largest front (p + q), factor doubles
 * stored and read once per solve (sum p (p + 2 q)), the fronts' dense
 * workspace doubles (64-row tiles, summed over fronts), factorization flops,
 * ordering s, symbolic s, largest separator.  When non-NULL: perm[n] (ND
 * position -> row), front_of[n] (position -> front, fronts numbered in
 * postorder so every front's pivots are contiguous) and parent[fronts]
 * (-1 at the root); call with them NULL first to learn the front count.    */
int pls_sparse_lu_analyze(const pls_csr *A, const char *options, double *stats, int64_t nstats, int32_t *perm,
                          int32_t *front_of, int32_t *parent);

/* Standalone inner Anderson mixing (lib/AndersonAcceleration.py:8-78): the
 * object a caller's own fixed-point loop holds, as the reference's
 * PreconditionerCC holds one per inner block (lib/Preconditioner.py:248-249).
 *   pls_anderson_create   AndersonAcceleration(order), vectors of length n
 *                         (AndersonAcceleration.py:8-17)
 *   pls_anderson_next     get_next_vector(gk) (AndersonAcceleration.py:19-78):
 *                         d_gk (device, length n) is replaced by the mixed
 *                         iterate x_k, in place as the reference's
 *                         self.xk.copy(gk); F / X histories persist across
 *                         calls, the least squares is Householder QR (TSQR)
 *   pls_anderson_destroy  frees the object and its stream.
 * Single-rank: the reference's scatter-to-rank-0 least squares over MPI is
 * the handle's inner accel path (option pls.inner_accel_order) at G > 1.    */
typedef struct pls_anderson pls_anderson;
int pls_anderson_create(int32_t order, int64_t n, pls_anderson **out);
int pls_anderson_next(pls_anderson *a, double *d_gk);
int pls_anderson_destroy(pls_anderson *a);

/* Kernel micro-entry points used by bench.py's roofline leg (device ptrs):
 * y = A x on the handle's A, repeated `reps` times; returns the mean device
 * time per launch in seconds measured with HIP events on the solver stream. */
int pls_bench_spmv(pls_handle *h, const double *d_x, double *d_y, int32_t reps, double *sec_per_launch);
/* The same for the low-precision product of pls_matmult_single_device.      */
int pls_bench_spmv_single(pls_handle *h, const double *d_x, double *d_y, int32_t reps, double *sec_per_launch);
/* Layout of A's SpMV copy: d16 = 1 for SELL-64/D16 (16-bit column deltas),
 * 0 for SELL-64 (int32 columns); matrix_bytes = bytes one product streams
 * from the matrix arrays (padding included).  Option "pls.sell_d16 0"
 * forces the int32 layout.                                                   */
int pls_spmv_layout(pls_handle *h, int32_t *d16, int64_t *matrix_bytes);
/* The same for the low-precision product: d16 = 1 where A's layout can carry
 * the fp32 value stream (SELL-64/D16 without a SELL/B3 part), matrix_bytes =
 * bytes one low product streams, 4 B per stored entry for the values instead
 * of 8 (0 where d16 = 0).                                                    */
int pls_spmv_layout_single(pls_handle *h, int32_t *d16, int64_t *matrix_bytes);
/* Shared delta streams of a SELL-64/D16 layout (options pls.d16_share -1 auto /
 * 0 never / 1 always, pls.d16_share_min_bytes): which = 0 A's layout, 1 the
 * reduced outer layout of the coupling reuse (zeros while not eligible).
 * stats[0] 1 when the layout's deltas are a shared stream, [1] its slices,
 * [2] those with fewer than 64 classes, [3] the 16-bit deltas it stores
 * (the padded entries when not shared), [4] layouts this handle has built
 * with a shared stream so far (inner blocks included).                       */
int pls_get_d16_share(pls_handle *h, int32_t which, int64_t stats[5]);
/* Streaming probe on the current device: per repetition `bytes` read (and,
 * unless read_only, `bytes` written) with 16-B-per-lane nontemporal accesses;
 * returns GB/s of bytes moved -- the achievable HBM rate beside the 8 TB/s
 * peak.                                                     */
int pls_bench_copy(int64_t bytes, int32_t reps, int32_t read_only, double *gbs);

#ifdef __cplusplus
}
#endif
#endif /* PLS_H */
