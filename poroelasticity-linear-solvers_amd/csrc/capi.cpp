// capi.cpp -- the handle (what a pls_handle points to: the system, the block
// preconditioner, the outer solver) and the extern "C" entry points declared
// in include/pls.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <numeric>

#include "../../include/pls.h"
#include "runtime.hpp"
#include "amg_host.hpp"
#include "anderson.hpp"
#include "bccols.hpp"
#include "blockpc.hpp"
#include "dist.hpp"
#include "synthetic.hpp"

namespace pls {

static thread_local std::string g_last_error;

// ================================================================ handle ===
// pls.pc_type with '_' read as ' ' (values with spaces are passed with '_' or as the literal tail)
static std::string checked_pc_type(const Options &o) {
    std::string pt = o.str("pls.pc_type", "diagonal");
    std::replace(pt.begin(), pt.end(), '_', ' ');
    static const char *ok[] = {"undrained", "undrained 3-way", "diagonal", "diagonal 3-way", "diagonal 3-way-II", "lu"};
    for (auto s : ok)
        if (pt == s) return pt;
    throw Error("pc type must be one of lu, undrained, diagonal, diagonal 3-way, diagonal 3-way-II.");
}

struct Handle {
    Ctx ctx;  // first: destroyed last, after every buffer, solver and stream that used it
    Options opt;
    Timers timers;
    int64_t n = 0, ns = 0, nf = 0, np = 0;
    bool three_way = false, setup_done = false, solver_ready = false, keep = true;
    Dist dist;                          // row slabs (size 1: everything local)
    bool distributed = false;
    std::unique_ptr<SynthDev> synth_rows;  // synthetic handles: row map for the rhs
    DBuf<int32_t> synth_offs;
    std::string pc_type, solver_type, inner_ksp, inner_pc;
    std::vector<int64_t> perm;   // internal -> caller
    std::vector<int32_t> fp_is_f, fp_is_p;  // 2-way: f / p positions inside the sorted fp set (IndexSet.py:10-26)
    DBuf<int64_t> dperm;
    DevCSR A, P, Pd;
    bool have_Pd = false;
    BlockPC bpc;
    std::unique_ptr<KSP> outer;
    AAR aar;
    DBuf<double> vout;  // host vectors on their way in and out
    // result
    pls_result res{};
    std::vector<double> history;
    std::unique_ptr<MatOp> Aop;
    Coupling coupling;           // the PC's coupling product reused by the outer A z (runtime.hpp)
    bool coupling_stale = true;  // decide again before the next solve (setup, solver creation, matrix update)

    void parse_params() {
        pc_type = checked_pc_type(opt);
        three_way = (pc_type == "diagonal 3-way" || pc_type == "undrained 3-way");
        solver_type = opt.str("pls.solver_type", "gmres");
        inner_ksp = opt.str("pls.inner_ksp_type", "gmres");
        inner_pc = opt.str("pls.inner_pc_type", "hypre");
        timers.enabled = opt.flag("pls.timers", true);
        ctx.sell_d16 = opt.flag("pls.sell_d16", true);
        ctx.d16_wide_lpr = (int)opt.integer("pls.d16_wide_lpr", 8);
        if (ctx.d16_wide_lpr != 1 && ctx.d16_wide_lpr != 2 && ctx.d16_wide_lpr != 4 && ctx.d16_wide_lpr != 8 &&
            ctx.d16_wide_lpr != 16 && ctx.d16_wide_lpr != 32 && ctx.d16_wide_lpr != 64)
            throw Error("pls.d16_wide_lpr must be a power of two <= 64");
        ctx.d16_unroll = (int)opt.integer("pls.d16_unroll", 4);
        ctx.d16_xcd = (int)opt.integer("pls.d16_xcd", 0);  // workgroup -> slice order (tuning)
        ctx.d16_share = (int)opt.integer("pls.d16_share", -1);  // shared delta streams: -1 auto, 0 never, 1 always
        if (ctx.d16_share < -1 || ctx.d16_share > 1) throw Error("pls.d16_share must be -1, 0 or 1");
        ctx.d16_share_min_bytes = opt.integer("pls.d16_share_min_bytes", 268435456);
        ctx.reuse_wide = (int)opt.integer("pls.reuse_wide", -1);  // coupling reuse on multi-lane rows: -1 auto, 0 off
        if (ctx.reuse_wide != -1 && ctx.reuse_wide != 0) throw Error("pls.reuse_wide must be -1 (auto) or 0");
        ctx.d16_unroll_single = (int)opt.integer("pls.d16_unroll_single", 8);  // the fp32-value kernel's depth
        if (ctx.d16_unroll_single != 1 && ctx.d16_unroll_single != 2 && ctx.d16_unroll_single != 4 &&
            ctx.d16_unroll_single != 8)
            throw Error("pls.d16_unroll_single must be 1, 2, 4 or 8");
        ctx.halo_overlap = opt.flag("pls.halo_overlap", true);
        ctx.d16_segs = (int)opt.integer("pls.d16_segs", D16_SEG);  // 8: force the halo layout (tests)
        if (ctx.d16_segs != D16_SEG && ctx.d16_segs != D16_SEG_MAX) throw Error("pls.d16_segs must be 4 or 8");
        ctx.d16_sigma = (int)opt.integer("pls.d16_sigma", 1024);
        if (ctx.d16_sigma < 0 || ctx.d16_sigma % 64) throw Error("pls.d16_sigma must be a multiple of 64 (0: off)");
        ctx.d16_sigma_pad = opt.num("pls.d16_sigma_pad", 0.15);
        ctx.d16_sorted_lpr = (int)opt.integer("pls.d16_sorted_lpr", 2);
        ctx.spmv_b3 = opt.flag("pls.spmv_b3", false);
        ctx.spmv_rcm = (int)opt.integer("pls.spmv_rcm", -1);
        ctx.sweep_chain = (int)opt.integer("pls.sweep_chain", -1);
        ctx.sweep_window = (int)opt.integer("pls.sweep_window", -1);
        ctx.ilu_factor_dep = (int)opt.integer("pls.ilu_factor_dep", 1);
        ctx.ilu_view = (int)opt.integer("pls.ilu_view", 0);
        // test knobs of the ILU(0) factorization: staged-entry cap, persistent grid cap
        ctx.ilu0_stage_cap = (int)opt.integer("pls.ilu0_stage", -1);
        ctx.ilu_dep_grid = (int)opt.integer("pls.ilu_dep_grid", 0);
        ctx.window_depth = (int)opt.integer("pls.window_depth", 2);
        if (ctx.window_depth != 2 && ctx.window_depth != 3) throw Error("pls.window_depth must be 2 or 3");
        ctx.window_ring = (int)opt.integer("pls.window_ring", -1);
        ctx.window_mixed = (int)opt.integer("pls.window_mixed", -1);
        ctx.window_kpw = (int)opt.integer("pls.window_kpw", 0);
        ctx.sweep_swin = (int)opt.integer("pls.sweep_swin", 0);
        ctx.amg_csr_below = opt.num("pls.amg_csr_below", 16.0);
        if (opt.flag("pls.debug_bounds", false) || opt.integer("pls.debug_partial_cap", 0) > 0)
            ctx.set_debug(opt.flag("pls.debug_bounds", false), opt.integer("pls.debug_partial_cap", 0),
                          opt.flag("pls.debug_no_grow", false), opt.flag("pls.debug_unguarded", false));
        if (ctx.d16_sorted_lpr != 1 && ctx.d16_sorted_lpr != 2 && ctx.d16_sorted_lpr != 4 && ctx.d16_sorted_lpr != 8 &&
            ctx.d16_sorted_lpr != 16)
            throw Error("pls.d16_sorted_lpr must be 1, 2, 4, 8 or 16");
    }
};

// A handle from an options string (and a communicator, for sharded systems).  pls.pc_type is
// validated before anything touches the device.
static std::unique_ptr<Handle> open_handle(const char *options, Comm *comm = nullptr) {
    {
        Options pre;
        pre.parse(options);
        checked_pc_type(pre);
    }
    auto H = std::make_unique<Handle>();
    H->opt.parse(options);
    H->parse_params();
    H->timers.st = H->ctx.st;
    if (comm) H->ctx.comm = comm;
    return H;
}

// What every creator ends with, perm and the sizes set: the permutation and the BC positions on
// the device, pls.keep_matrices (default `keep`).
static pls_handle *finish_handle(std::unique_ptr<Handle> H, const std::vector<int32_t> &bcs, bool keep) {
    H->dperm.alloc(std::max<int64_t>(H->n, 1));
    HIPCHK(hipMemcpy(H->dperm.p, H->perm.data(), sizeof(int64_t) * H->n, hipMemcpyHostToDevice));
    H->bpc.set_bcs(bcs, H->np);
    H->keep = H->opt.flag("pls.keep_matrices", keep);
    return reinterpret_cast<pls_handle *>(H.release());
}

// ------------------------------------------------------------ setup path ---
// rows permuted and re-sorted into the internal field order; rows on host
// threads (the footing N=128 system's three 68.8M-entry matrices took ~8 s of
// pls_create on one thread)
static void permute_host(const pls_csr *M, const std::vector<int64_t> &perm, const std::vector<int64_t> &inv,
                         hvec<int64_t> &rp, hvec<int32_t> &ci, hvec<double> &v) {
    const int64_t n = (int64_t)perm.size();
    rp.assign(n + 1, 0);
    for (int64_t i = 0; i < n; ++i) rp[i + 1] = rp[i] + (M->row_ptr[perm[i] + 1] - M->row_ptr[perm[i]]);
    ci.resize(rp[n]);
    v.resize(rp[n]);
    std::atomic<bool> bad{false};
    amgh::parallel_rows(n, amgh::setup_threads(), [&](int, int64_t i0, int64_t i1) {
        std::vector<std::pair<int32_t, double>> row;
        for (int64_t i = i0; i < i1; ++i) {
            const int64_t o = perm[i];
            row.clear();
            for (int64_t k = M->row_ptr[o]; k < M->row_ptr[o + 1]; ++k) {
                const int32_t cc = M->col[k];
                if (cc < 0 || cc >= n) {
                    bad = true;
                    row.emplace_back(0, 0.0);
                    continue;
                }
                row.emplace_back((int32_t)inv[cc], M->val[k]);
            }
            std::sort(row.begin(), row.end(), [](auto &a, auto &b) { return a.first < b.first; });
            for (size_t t = 0; t < row.size(); ++t) {
                ci[rp[i] + t] = row[t].first;
                v[rp[i] + t] = row[t].second;
            }
        }
    });
    if (bad) throw Error("column index out of range");
}

static void upload_permuted(const pls_csr *M, Handle &H, const std::vector<int64_t> &inv, DevCSR &out) {
    if (M->nrows != H.n || M->ncols != H.n) throw Error("matrix must be n x n with n = ns + nf + np");
    hvec<int64_t> rp;
    hvec<int32_t> ci;
    hvec<double> v;
    permute_host(M, H.perm, inv, rp, ci, v);
    upload_csr(out, H.n, H.n, rp.data(), ci.data(), v.data(), H.ctx);
}

static void do_setup(Handle &H) {
    if (H.setup_done) return;
    H.coupling.eligible = false;  // the blocks change under it: decide_coupling runs before the next solve
    H.coupling_stale = true;
    H.bpc.coupling = &H.coupling;
    H.bpc.setup({H.P, H.Pd, H.have_Pd, H.dist, H.distributed, H.three_way, H.ns, H.nf, H.np, H.fp_is_f, H.fp_is_p,
                 H.inner_ksp, H.inner_pc, H.opt, H.timers, H.ctx});
    H.vout.alloc(std::max<int64_t>(H.n, 1));
    if (!H.keep) {
        H.P = DevCSR();
        H.Pd = DevCSR();
    }
    H.ctx.sync();
    H.setup_done = true;
}

// lib/Solver.py:64-103 create_solver (after the PC exists, as in Poromechanics.py:62-67)
static void do_setup_solver(Handle &H) {
    if (H.solver_ready) return;
    Ctx &c = H.ctx;
    const Options &o = H.opt;
    const int64_t n = H.n;
    H.solver_type = o.str("pls.solver_type", "gmres");
    const double atol = o.num("pls.solver_atol", 1e-8), rtol = o.num("pls.solver_rtol", 1e-6);
    const int64_t maxiter = o.integer("pls.solver_maxiter", 500);
    H.A.tag = 1;
    build_sell(H.A, c);
    H.Aop = std::make_unique<MatOp>(&H.A);
    H.Aop->timers = &H.timers;
    H.Aop->coupling = &H.coupling;
    H.coupling_stale = true;
    if (H.solver_type == "aar") {
        // AAR keeps its own start (x0 = None in the reference): the outer KSP's guess options have no meaning
        for (const char *key : {"global_ksp_initial_guess_nonzero", "global_ksp_guess_type",
                                "global_ksp_guess_fischer_model", "global_ksp_guess_fischer_tol"})
            if (o.has(key))
                throw Error(std::string(key) +
                            " is not available with pls.solver_type aar (AAR starts from its own x0)");
        H.aar.configure(o, n, atol, rtol, maxiter);
    } else {
        const int64_t restart = (H.solver_type == "gmres") ? maxiter : 30;
        H.outer = make_ksp("global_", o, &H.A, nullptr, H.solver_type, "python", c, rtol, atol, 1e20, maxiter, restart,
                           &H.bpc);
        H.outer->owned_op.reset();
        H.outer->A = H.Aop.get();
        if (H.outer->operator_single) H.Aop->enable_low(c, "global_pls_gmres_operator single");
        H.outer->monitor = H.outer->monitor || o.flag("pls.solver_monitor", false);
        const std::string gpc = o.str("global_pc_type", "python");
        if (gpc != "python") throw Error("global_pc_type must stay 'python' (the block preconditioner)");
    }
    c.sync();
    H.solver_ready = true;
}

// Coupling reuse, decided when the preconditioner and the solver exist and again after every
// matrix update: one rank, the 2-way PC without mixer, right-preconditioned gmres / fgmres,
// plain D16 layouts, and the PC's coupling block bitwise A's (build_coupling).
// pls.reuse_coupling: -1 where eligible (default), 0 never, 1 an error where not eligible.
static void decide_coupling(Handle &H) {
    Coupling &R = H.coupling;
    const int64_t mode = H.opt.integer("pls.reuse_coupling", -1);
    if (mode < -1 || mode > 1) throw Error("pls.reuse_coupling must be -1 (auto), 0 or 1");
    R.eligible = false;
    R.fresh_for = nullptr;
    const KSP *k = H.outer.get();
    std::string why;
    if (mode == 0) why = "pls.reuse_coupling 0";
    else if (H.distributed) why = "more than one rank";
    else if (H.three_way) why = "3-way preconditioner";
    else if (!k || (k->type != "gmres" && k->type != "fgmres") || !k->right)
        why = "the outer solver is not right-preconditioned gmres or fgmres";
    else if (!H.bpc.coupling_block()) why = "the preconditioner mixes its output (inner accel order > 0)";
    else if (!build_coupling(H.A, H.ns, *H.bpc.coupling_block(), R, H.ctx)) why = R.why;
    if (!R.eligible) {
        R.reduced = DevSELL();
        R.qw.release();
        R.wide_rows = 0;
        R.why = why;
        if (mode == 1) throw Error("pls.reuse_coupling 1: the coupling product cannot be reused: " + why);
    }
    // compressed-operator GMRES: the fp32 streams of the (new) A and of its reduced layout
    if (H.Aop && H.Aop->low) {
        H.Aop->enable_low(H.ctx, "global_pls_gmres_operator single");
        if (R.eligible) build_low(R.reduced, H.ctx, "global_pls_gmres_operator single (reduced outer operator)");
    }
    H.coupling_stale = false;
}

static void ensure_ready(Handle &H) {
    do_setup(H);
    do_setup_solver(H);
    if (H.coupling_stale) decide_coupling(H);
}

static void solve_device(Handle &H, const double *b, double *x) {
    ensure_ready(H);
    Ctx &c = H.ctx;
    H.bpc.pc_applies = 0;
    H.timers.begin(T_SOLVER);
    if (H.solver_type == "aar") {
        H.aar.solve(*H.Aop, H.bpc, b, x, c, H.timers, H.history, H.res);
    } else {
        H.outer->solve(b, x, c);
        H.res.its = H.outer->its;
        H.res.reason = H.outer->reason;
        H.res.rnorm = H.outer->rnorm;
        H.history = H.outer->history;
    }
    H.timers.end(T_SOLVER);
    c.sync();
    H.timers.flush();
    H.res.pc_applies = H.bpc.pc_applies;
    H.res.history_len = (int32_t)H.history.size();
}

}  // namespace pls

// ======================================================== extern "C" ABI ===
using namespace pls;

#define PLS_TRY(...)                                            \
    try {                                                       \
        __VA_ARGS__;                                            \
        return 0;                                               \
    } catch (const std::exception &e) {                         \
        g_last_error = e.what();                                \
        return 1;                                               \
    } catch (...) {                                             \
        g_last_error = "unknown error";                         \
        return 1;                                               \
    }

extern "C" {

int pls_abi_version(void) { return PLS_ABI_VERSION; }
const char *pls_last_error(void) { return g_last_error.c_str(); }

int pls_device_count(int *count) {
    PLS_TRY({
        int c = 0;
        hipError_t e = hipGetDeviceCount(&c);
        if (e != hipSuccess) c = 0;
        *count = c;
    })
}
int pls_set_device(int device) { PLS_TRY(HIPCHK(hipSetDevice(device))) }

static void check_is(const int32_t *is, int64_t m, int64_t n, std::vector<char> &seen, const char *name) {
    for (int64_t i = 0; i < m; ++i) {
        if (is[i] < 0 || is[i] >= n) throw Error(std::string(name) + ": index out of range");
        if (i && is[i] <= is[i - 1]) throw Error(std::string(name) + ": must be sorted ascending and unique");
        if (seen[is[i]]) throw Error(std::string(name) + ": overlaps another field");
        seen[is[i]] = 1;
    }
}

int pls_create(const pls_csr *A, const pls_csr *P, const pls_csr *Pdiff, const int32_t *is_s, int64_t ns,
               const int32_t *is_f, int64_t nf, const int32_t *is_p, int64_t np, const int32_t *bcs_sub_p, int64_t nbc,
               const char *options, pls_handle **out) {
    PLS_TRY({
        if (!A || !P || !out) throw Error("pls_create: A, P and out are required");
        auto H = open_handle(options);
        H->ns = ns; H->nf = nf; H->np = np; H->n = ns + nf + np;
        const int64_t n = H->n;
        std::vector<char> seen(n, 0);
        check_is(is_s, ns, n, seen, "is_s");
        check_is(is_f, nf, n, seen, "is_f");
        check_is(is_p, np, n, seen, "is_p");
        // internal order: 2-way [is_s | is_fp = sorted(f U p)], 3-way [is_s | is_f | is_p]
        H->perm.assign(is_s, is_s + ns);
        if (H->three_way) {
            H->perm.insert(H->perm.end(), is_f, is_f + nf);
            H->perm.insert(H->perm.end(), is_p, is_p + np);
        } else {
            std::vector<int64_t> fp(is_f, is_f + nf);
            fp.insert(fp.end(), is_p, is_p + np);
            std::sort(fp.begin(), fp.end());
            H->perm.insert(H->perm.end(), fp.begin(), fp.end());
            std::vector<char> isf(n, 0);
            for (int64_t i = 0; i < nf; ++i) isf[is_f[i]] = 1;
            for (size_t t = 0; t < fp.size(); ++t) (isf[fp[t]] ? H->fp_is_f : H->fp_is_p).push_back((int32_t)t);
        }
        std::vector<int64_t> inv(n);
        for (int64_t i = 0; i < n; ++i) inv[H->perm[i]] = i;
        upload_permuted(A, *H, inv, H->A);
        upload_permuted(P, *H, inv, H->P);
        if (Pdiff) {
            upload_permuted(Pdiff, *H, inv, H->Pd);
            H->have_Pd = true;
        }
        *out = finish_handle(std::move(H), std::vector<int32_t>(bcs_sub_p, bcs_sub_p + nbc), true);
    })
}

// Synthetic system generated directly in HBM.  With a communicator of size G
// every rank generates only its row slabs (global columns), then the
// matrices become distributed (make_dist): the same global system, sharded.
static pls_handle *create_synthetic(const pls_synth_spec *spec, const char *options, Comm *comm) {
    auto H = open_handle(options, comm);
    Comm *cm = H->ctx.comm;
    SynthHost S;
    S.init(*spec);
    H->dist.init(S.n, cm->rank, cm->size);
    H->distributed = cm->size > 1;
    const Dist &D = H->dist;
    H->ns = D.len[0]; H->nf = D.len[1]; H->np = D.len[2];
    H->n = D.nloc;
    SynthSystem sys = generate_synthetic(S, D, H->three_way, H->ctx);
    H->A = std::move(sys.A);
    H->P = std::move(sys.P);
    H->Pd = std::move(sys.Pd);
    H->have_Pd = H->three_way;
    H->synth_offs = std::move(sys.offs);
    H->synth_rows = std::move(sys.rows);
    if (H->distributed) make_dist(H->A, D, 0, 2, cm, H->ctx);
    H->perm.resize(H->n);
    std::iota(H->perm.begin(), H->perm.end(), 0);
    const bool keep = H->A.nnz < 50000000;
    return finish_handle(std::move(H), sys.bcs, keep);
}

int pls_create_synthetic(const pls_synth_spec *spec, const char *options, pls_handle **out) {
    PLS_TRY(*out = create_synthetic(spec, options, nullptr))
}

int pls_create_synthetic_dist(const pls_synth_spec *spec, const char *options, pls_comm *comm, pls_handle **out) {
    PLS_TRY({
        if (!comm) throw Error("pls_create_synthetic_dist: communicator required");
        *out = create_synthetic(spec, options, reinterpret_cast<Comm *>(comm));
    })
}

// This rank's share of a caller-assembled system (dist.cpp: shard_rows); collective over `comm`.
int pls_create_dist(const pls_csr *A, const pls_csr *P, const pls_csr *Pdiff, int64_t row_start, const int32_t *is_s,
                    int64_t ns, const int32_t *is_f, int64_t nf, const int32_t *is_p, int64_t np,
                    const int32_t *bcs_sub_p, int64_t nbc, const char *options, pls_comm *comm, pls_handle **out) {
    PLS_TRY({
        if (!comm || !out) throw Error("pls_create_dist: communicator and out are required");
        if (!A || !P) throw Error("pls_create_dist: A and P are required");
        Comm *cm = reinterpret_cast<Comm *>(comm);
        auto H = open_handle(options, cm);
        ShardedRows sh = shard_rows(A, P, Pdiff, row_start, is_s, ns, is_f, nf, is_p, np, H->three_way, cm, H->ctx);
        H->dist = std::move(sh.dist);
        H->perm = std::move(sh.perm);
        H->fp_is_f = std::move(sh.fp_is_f);
        H->fp_is_p = std::move(sh.fp_is_p);
        H->A = std::move(sh.A);
        H->P = std::move(sh.P);
        H->Pd = std::move(sh.Pd);
        H->have_Pd = sh.have_Pd;
        H->ns = ns; H->nf = nf; H->np = np; H->n = ns + nf + np;
        H->distributed = cm->size > 1;
        if (H->distributed) make_dist(H->A, H->dist, 0, 2, cm, H->ctx);
        // bcs_sub_pressure: positions inside this rank's p sub-vector (what
        // Poromechanics.py:48-55 computes from the rank's own dofs)
        *out = finish_handle(std::move(H), std::vector<int32_t>(bcs_sub_p, bcs_sub_p + nbc), true);
    })
}

int pls_rccl_unique_id(char out[128]) { PLS_TRY(rccl_unique_id(out)) }
int pls_comm_create_rccl(const char id[128], int rank, int size, pls_comm **out) {
    PLS_TRY(*out = reinterpret_cast<pls_comm *>(static_cast<Comm *>(rccl_init(id, rank, size))))
}
int pls_comm_create_callback(int rank, int size, pls_allgather_fn fn, void *user, pls_comm **out) {
    PLS_TRY({
        if (!fn || rank < 0 || rank >= size) throw Error("pls_comm_create_callback: bad arguments");
        auto *cb = new CommCallback();
        cb->rank = rank;
        cb->size = size;
        cb->fn = fn;
        cb->user = user;
        *out = reinterpret_cast<pls_comm *>(static_cast<Comm *>(cb));
    })
}
int pls_comm_destroy(pls_comm *comm) { PLS_TRY(delete reinterpret_cast<Comm *>(comm)) }

int pls_setup(pls_handle *h) { PLS_TRY(do_setup(*reinterpret_cast<Handle *>(h))) }
int pls_destroy(pls_handle *h) { PLS_TRY(delete reinterpret_cast<Handle *>(h)) }
int pls_set_option(pls_handle *hh, const char *key, const char *value) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        std::string k(key ? key : "");
        while (!k.empty() && k[0] == '-') k.erase(0, 1);
        if (k.empty()) throw Error("pls_set_option: empty key");
        const bool solver_key = k.rfind("pls.solver", 0) == 0 || k.rfind("pls.aar", 0) == 0 || k.rfind("global_", 0) == 0;
        if (solver_key && H.solver_ready) throw Error("option " + k + " set after the solver was created");
        if (!solver_key && H.setup_done) throw Error("option " + k + " set after the preconditioner was set up");
        H.opt.kv[k] = value ? value : "";
        if (k == "pls.timers") H.timers.enabled = H.opt.flag(k, true);
    })
}
int pls_create_solver(pls_handle *hh) {
    PLS_TRY({
        ensure_ready(*reinterpret_cast<Handle *>(hh));
    })
}

int pls_get_sizes(pls_handle *hh, int64_t *n, int64_t *ns, int64_t *nf, int64_t *np, int64_t *nnz_A) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        if (n) *n = H.n;
        if (ns) *ns = H.ns;
        if (nf) *nf = H.nf;
        if (np) *np = H.np;
        if (nnz_A) *nnz_A = H.A.nnz;
    })
}

static void to_internal(Handle &H, const double *x_host, double *d_internal) {
    HIPCHK(hipMemcpyAsync(H.vout.p, x_host, sizeof(double) * H.n, hipMemcpyHostToDevice, H.ctx.st));
    launch_gather(H.n, H.dperm.p, H.vout.p, d_internal, H.ctx.st);
}
static void from_internal(Handle &H, const double *d_internal, double *y_host) {
    launch_scatter(H.n, H.dperm.p, d_internal, H.vout.p, H.ctx.st);
    HIPCHK(hipMemcpyAsync(y_host, H.vout.p, sizeof(double) * H.n, hipMemcpyDeviceToHost, H.ctx.st));
    H.ctx.sync();
}

int pls_pc_apply(pls_handle *hh, const double *x, double *y) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        do_setup(H);
        DBuf<double> xi(H.n), yi(H.n);
        to_internal(H, x, xi.p);
        H.bpc.apply(xi.p, yi.p, H.ctx);
        from_internal(H, yi.p, y);
        H.timers.flush();
    })
}

int pls_matmult(pls_handle *hh, const double *x, double *y) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        DBuf<double> xi(H.n), yi(H.n);
        if (!H.vout.p) H.vout.alloc(H.n);
        to_internal(H, x, xi.p);
        build_sell(H.A, H.ctx);
        spmv(H.A, xi.p, yi.p, H.ctx);
        from_internal(H, yi.p, y);
    })
}

// the outer operator's layout with its fp32 value stream (built on demand; the refusals of build_low)
static DevSELL &low_layout(Handle &H, const char *who) {
    build_sell(H.A, H.ctx);
    if (!H.A.sell) throw Error(std::string(who) + ": the operator has no rows");
    build_low(*H.A.sell, H.ctx, who);
    return *H.A.sell;
}
int pls_matmult_single(pls_handle *hh, const double *x, double *y) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        DBuf<double> xi(H.n), yi(H.n);
        if (!H.vout.p) H.vout.alloc(H.n);
        to_internal(H, x, xi.p);
        low_layout(H, "pls_matmult_single");
        spmv(H.A, xi.p, yi.p, H.ctx, 1.0, 0.0, nullptr, true);
        from_internal(H, yi.p, y);
    })
}

int pls_solve(pls_handle *hh, const double *b, double *x, pls_result *res) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        do_setup(H);
        DBuf<double> bi(H.n), xi(H.n);
        to_internal(H, b, bi.p);
        ensure_ready(H);
        if (H.outer && H.outer->guess_nonzero && !H.outer->guess_fischer) to_internal(H, x, xi.p);  // x is read only then
        solve_device(H, bi.p, xi.p);
        from_internal(H, xi.p, x);
        if (res) *res = H.res;
    })
}

int pls_solve_device(pls_handle *hh, const double *d_b, double *d_x, pls_result *res) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        solve_device(H, d_b, d_x);
        if (res) *res = H.res;
    })
}
int pls_pc_apply_device(pls_handle *hh, const double *d_x, double *d_y) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        do_setup(H);
        H.bpc.apply(d_x, d_y, H.ctx);
        H.ctx.sync();
        H.timers.flush();
    })
}
int pls_matmult_device(pls_handle *hh, const double *d_x, double *d_y) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        build_sell(H.A, H.ctx);
        // pls.reuse_coupling_probe (tests): the outer operator's product as GMRES forms it after
        // a PC application -- reduced when d_x is what pls_pc_apply_device returned last
        if (H.Aop && H.opt.flag("pls.reuse_coupling_probe", false)) H.Aop->apply_after(H.bpc, d_x, d_y, H.ctx);
        else spmv(H.A, d_x, d_y, H.ctx);
        H.ctx.sync();
    })
}
int pls_matmult_single_device(pls_handle *hh, const double *d_x, double *d_y) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        low_layout(H, "pls_matmult_single_device");
        // pls.reuse_coupling_probe (tests): as pls_matmult_device, through the low reduced launch
        if (H.Aop && H.Aop->low && H.opt.flag("pls.reuse_coupling_probe", false))
            H.Aop->apply_after_low(H.bpc, d_x, d_y, H.ctx);
        else spmv(H.A, d_x, d_y, H.ctx, 1.0, 0.0, nullptr, true);
        H.ctx.sync();
    })
}
int pls_synthetic_rhs_device(pls_handle *hh, uint64_t seed, double *d_b) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        if (!H.synth_rows) throw Error("pls_synthetic_rhs_device: not a synthetic handle");
        launch_synth_rhs(*H.synth_rows, seed, d_b, H.ctx.st);
        H.ctx.sync();
    })
}
int pls_device_alloc(int64_t bytes, void **d_ptr) { PLS_TRY(HIPCHK(hipMalloc(d_ptr, (size_t)bytes))) }
int pls_device_free(void *d_ptr) { PLS_TRY(HIPCHK(hipFree(d_ptr))) }
int pls_memcpy_h2d(void *d_dst, const void *h_src, int64_t bytes) {
    PLS_TRY(HIPCHK(hipMemcpy(d_dst, h_src, (size_t)bytes, hipMemcpyHostToDevice)))
}
int pls_memcpy_d2h(void *h_dst, const void *d_src, int64_t bytes) {
    PLS_TRY(HIPCHK(hipMemcpy(h_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost)))
}

int pls_get_result(pls_handle *hh, pls_result *res) {
    PLS_TRY({ *res = reinterpret_cast<Handle *>(hh)->res; })
}
int pls_get_history(pls_handle *hh, double *hist, int32_t cap) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        const int32_t m = std::min<int32_t>(cap, (int32_t)H.history.size());
        std::copy(H.history.begin(), H.history.begin() + m, hist);
    })
}
int pls_get_timings(pls_handle *hh, pls_timings *t) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        H.timers.flush();
        t->pc_total = H.timers.acc[T_PC_TOTAL];
        t->pc_solid = H.timers.acc[T_PC_SOLID];
        t->pc_fluid = H.timers.acc[T_PC_FLUID];
        t->pc_press = H.three_way ? H.timers.acc[T_PC_PRESS] : H.timers.acc[T_PC_FLUID];
        t->pc_alloc = H.timers.acc[T_PC_ALLOC];
        t->solver_total = H.timers.acc[T_SOLVER];
        t->spmv_total = H.timers.acc[T_SPMV];
        t->spmv_calls = H.timers.spmv_calls;
    })
}
// the KSP with this options prefix (the outer solver, the blocks', the fp fieldsplit's); `who` names the caller
static const KSP *find_ksp(Handle &H, const char *prefix, const void *out, const std::string &who) {
    if (!prefix || !out) throw Error(who + ": null argument");
    const std::string want(prefix);
    const KSP *found = nullptr;
    std::vector<const KSP *> all = H.bpc.ksps();
    all.push_back(H.outer.get());
    for (const KSP *k : all)
        if (k && k->prefix == want) found = k;
    if (!found) throw Error(who + ": no inner solver with prefix '" + want + "'");
    return found;
}
int pls_get_ksp_stats(pls_handle *hh, const char *prefix, int64_t *stats) {
    PLS_TRY({
        const KSP *found = find_ksp(*reinterpret_cast<Handle *>(hh), prefix, stats, "pls_get_ksp_stats");
        stats[0] = found->stat_solves;
        stats[1] = found->stat_its;
        stats[2] = found->stat_max;
        stats[3] = found->stat_div;
        stats[4] = found->stat_last_neg;
    })
}
int pls_get_gmres_orthog_stats(pls_handle *hh, const char *prefix, int64_t *stats) {
    PLS_TRY({
        const KSP *found = find_ksp(*reinterpret_cast<Handle *>(hh), prefix, stats, "pls_get_gmres_orthog_stats");
        if (found->type != "gmres" && found->type != "fgmres")
            throw Error("pls_get_gmres_orthog_stats: the solver with prefix '" + found->prefix + "' is of type " +
                        found->type + ", not gmres or fgmres");
        stats[0] = found->stat_orth_steps;
        stats[1] = found->stat_orth_second;
        stats[2] = found->orthog;
    })
}
int pls_get_ksp_guess_stats(pls_handle *hh, const char *prefix, int64_t stats[6], double *last_reduction) {
    PLS_TRY({
        const KSP *found = find_ksp(*reinterpret_cast<Handle *>(hh), prefix, stats, "pls_get_ksp_guess_stats");
        stats[0] = found->guess_fischer ? 1 : 0;
        stats[1] = found->guess_fischer ? found->guess_m : 0;
        stats[2] = found->guess_fischer ? found->guess_size : 0;
        stats[3] = found->stat_guess_formed;
        stats[4] = found->stat_guess_skipped;
        stats[5] = found->stat_guess_resets;
        if (last_reduction) *last_reduction = found->guess_last_reduction;
    })
}
int pls_get_ksp_guess_info(pls_handle *hh, const char *prefix, int64_t *reads_x, double *seconds) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        if (!prefix || !reads_x || !seconds) throw Error("pls_get_ksp_guess_info: null argument");
        ensure_ready(H);  // (the options are read when the solver is created)
        *reads_x = 0;
        *seconds = std::nan("");
        if (std::string(prefix) == "global_" && !H.outer) return 0;  // AAR: no outer KSP, x is output only
        const KSP *found = find_ksp(H, prefix, seconds, "pls_get_ksp_guess_info");
        *reads_x = found->guess_nonzero && !found->guess_fischer ? 1 : 0;
        if (found->guess_timing) *seconds = found->guess_seconds;
    })
}
int pls_get_gmres_basis_stats(pls_handle *hh, const char *prefix, int64_t *stats) {
    PLS_TRY({
        const KSP *found = find_ksp(*reinterpret_cast<Handle *>(hh), prefix, stats, "pls_get_gmres_basis_stats");
        if (found->type != "gmres" && found->type != "fgmres")
            throw Error("pls_get_gmres_basis_stats: the solver with prefix '" + found->prefix + "' is of type " +
                        found->type + ", not gmres or fgmres");
        stats[0] = found->basis_single ? 1 : 0;
        stats[1] = found->basis_bytes();
        stats[2] = found->stat_cb_forced;
        stats[3] = found->stat_cb_confirm;
        stats[4] = found->stat_cb_failed;
    })
}
int pls_get_gmres_operator_stats(pls_handle *hh, const char *prefix, int64_t *stats) {
    PLS_TRY({
        const KSP *found = find_ksp(*reinterpret_cast<Handle *>(hh), prefix, stats, "pls_get_gmres_operator_stats");
        if (found->type != "gmres" && found->type != "fgmres")
            throw Error("pls_get_gmres_operator_stats: the solver with prefix '" + found->prefix + "' is of type " +
                        found->type + ", not gmres or fgmres");
        const MatOp *op = dynamic_cast<const MatOp *>(found->A);
        stats[0] = found->operator_single ? 1 : 0;
        stats[1] = found->operator_single && op ? op->low_bytes() : 0;
        stats[2] = found->stat_co_low;
        stats[3] = found->stat_co_double;
    })
}
int pls_get_reuse_rows(pls_handle *hh, uint8_t *mask) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        if (!mask) throw Error("pls_get_reuse_rows: null argument");
        const Coupling &R = H.coupling;
        const bool on = R.eligible && (int64_t)R.reuse.size() == H.n;
        for (int64_t i = 0; i < H.n; ++i) mask[H.perm[i]] = on ? R.reuse[i] : 0;
    })
}
int pls_get_chebyshev_bounds(pls_handle *hh, const char *prefix, double *out) {
    PLS_TRY({
        const KSP *found = find_ksp(*reinterpret_cast<Handle *>(hh), prefix, out, "pls_get_chebyshev_bounds");
        if (found->type != "chebyshev")
            throw Error("pls_get_chebyshev_bounds: the solver with prefix '" + found->prefix + "' is of type " +
                        found->type + ", not chebyshev");
        if (!found->stat_solves || !found->cheb_ready)
            throw Error("pls_get_chebyshev_bounds: the solver with prefix '" + found->prefix +
                        "' has not run a solve yet");
        out[0] = found->cheb_emin;
        out[1] = found->cheb_emax;
        out[2] = found->cheb_raw[0];
        out[3] = found->cheb_raw[1];
    })
}
int pls_get_ilu_fill(pls_handle *hh, const char *prefix, int64_t *stats) {
    PLS_TRY({
        const KSP *found = find_ksp(*reinterpret_cast<Handle *>(hh), prefix, stats, "pls_get_ilu_fill");
        const PCILU *ilu = found->pc ? dynamic_cast<const PCILU *>(found->pc->unwrapped()) : nullptr;
        if (!ilu || ilu->exact || ilu->sgs)
            throw Error("pls_get_ilu_fill: the PC with prefix '" + found->prefix + "' is of type " +
                        (found->pc ? found->pc->type : std::string("none")) + ", not ilu or bjacobi with ilu blocks");
        stats[0] = ilu->levels;
        stats[1] = ilu->nnz_block;
        stats[2] = ilu->F.nnz;
        stats[3] = ilu->F.max_row;
    })
}
static const PCASM *find_asm(Handle &H, const char *prefix, const void *out, const std::string &who) {
    const KSP *found = find_ksp(H, prefix, out, who);
    const PCASM *a = dynamic_cast<const PCASM *>(found->pc);
    if (!a)
        throw Error(who + ": the PC with prefix '" + found->prefix + "' is of type " +
                    (found->pc ? found->pc->type : std::string("none")) + ", not asm");
    return a;
}
int pls_get_asm_stats(pls_handle *hh, const char *prefix, int64_t *stats) {
    PLS_TRY({
        const PCASM *a = find_asm(*reinterpret_cast<Handle *>(hh), prefix, stats, "pls_get_asm_stats");
        stats[0] = a->nblocks;
        stats[1] = a->overlap;
        stats[2] = (int64_t)a->atype;
        stats[3] = a->ne;
        stats[4] = a->largest;
        stats[5] = a->fused ? 1 : 0;
    })
}
int pls_get_asm_rows(pls_handle *hh, const char *prefix, int64_t *ptr, int32_t *rows) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        const PCASM *a = find_asm(H, prefix, ptr, "pls_get_asm_rows");
        std::copy(a->ptr_h.begin(), a->ptr_h.end(), ptr);
        if (rows && a->ne) {
            H.ctx.sync();
            HIPCHK(hipMemcpy(rows, a->gidx.p, sizeof(int32_t) * a->ne, hipMemcpyDeviceToHost));
        }
    })
}
int pls_get_boomeramg_relax(pls_handle *hh, const char *prefix, int64_t stats[6], double *lambda, int32_t cap) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        do_setup(H);
        const KSP *found = find_ksp(H, prefix, stats, "pls_get_boomeramg_relax");
        if (lambda == nullptr && cap > 0) throw Error("pls_get_boomeramg_relax: null argument");
        const bool ok = found->pc && (boomeramg_relax_info(found->pc, stats, lambda, cap) ||
                                      boomeramg_relax_info(found->pc->unwrapped(), stats, lambda, cap));
        if (!ok)
            throw Error("pls_get_boomeramg_relax: the PC with prefix '" + found->prefix + "' is of type " +
                        (found->pc ? found->pc->type : std::string("none")) + ", not the BoomerAMG stand-in of hypre");
    })
}
int pls_relax_step(pls_handle *hh, const double *m, const double *b, const double *x, double *d, double a, double g,
                   int32_t fused, double *x_new, int32_t *was_fused) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        if (!m || !b || !x || !x_new || !was_fused) throw Error("pls_relax_step: null argument");
        if (H.A.halo) throw Error("pls_relax_step: one rank only");
        const int64_t n = H.n;
        DBuf<double> mi(n), bi(n), xi(n), di(n), yi(n), ri(n);
        if (!H.vout.p) H.vout.alloc(n);
        to_internal(H, m, mi.p);
        to_internal(H, b, bi.p);
        to_internal(H, x, xi.p);
        if (d) to_internal(H, d, di.p);
        build_sell(H.A, H.ctx);
        const int flags = d ? (RELAX_READ_D | RELAX_WRITE_D) : 0;
        const DevSELL *S = H.A.sell.get();
        *was_fused = fused && S && S->d16 && !S->nperm && !S->b3_nslices;
        if (*was_fused) {
            launch_d16_relax(n, S->nslices, S->streams(), S->val.p, xi.p, yi.p, bi.p, mi.p, d ? di.p : nullptr, a, g,
                             flags, H.ctx.d16_unroll, H.ctx.d16_xcd, H.ctx.st, S->nrows_mapped ? S->rowmap.p : nullptr);
        } else {
            spmv(H.A, xi.p, ri.p, H.ctx, -1.0, 1.0, bi.p);
            launch_relax_step(n, ri.p, xi.p, yi.p, mi.p, d ? di.p : nullptr, a, g, flags, H.ctx.st);
        }
        HIPCHK(hipGetLastError());
        if (d) from_internal(H, di.p, d);
        from_internal(H, yi.p, x_new);
    })
}
int pls_get_bc_columns_stats(pls_handle *hh, const char *prefix, int64_t stats[5]) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        if (!prefix || !stats) throw Error("pls_get_bc_columns_stats: null argument");
        ensure_ready(H);  // (the split is made when the inner solvers are)
        const BcColumns *bc = find_ksp(H, prefix, stats, "pls_get_bc_columns_stats")->bc.get();
        stats[0] = bc ? bc->mode : 0;
        stats[1] = bc ? bc->nbc : 0;
        stats[2] = bc ? bc->nmoved : 0;
        stats[3] = bc ? bc->nrc : 0;
        stats[4] = bc ? bc->bytes() : 0;
    })
}
int pls_get_bc_columns_matrix(pls_handle *hh, const char *prefix, int32_t *bc_rows, int64_t *c_rp, int32_t *c_ci,
                              double *c_val) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        if (!prefix) throw Error("pls_get_bc_columns_matrix: null argument");
        ensure_ready(H);
        const KSP *found = find_ksp(H, prefix, prefix, "pls_get_bc_columns_matrix");
        const BcColumns *bc = found->bc.get();
        H.ctx.sync();
        if (bc_rows && bc && bc->nbc)
            HIPCHK(hipMemcpy(bc_rows, bc->bc_rows.p, sizeof(int32_t) * bc->nbc, hipMemcpyDeviceToHost));
        if (c_rp) {
            // the compact rows spread over all rows of the block
            const int64_t n = found->n, nrc = bc ? bc->nrc : 0;
            std::vector<int32_t> rows(nrc);
            std::vector<int64_t> rp(nrc + 1, 0);
            if (nrc) {
                HIPCHK(hipMemcpy(rows.data(), bc->crow.p, sizeof(int32_t) * nrc, hipMemcpyDeviceToHost));
                HIPCHK(hipMemcpy(rp.data(), bc->crp.p, sizeof(int64_t) * (nrc + 1), hipMemcpyDeviceToHost));
            }
            int64_t k = 0;
            for (int64_t i = 0; i <= n; ++i) {
                while (k < nrc && rows[k] < i) ++k;
                c_rp[i] = rp[k];
            }
        }
        if (bc && bc->nmoved) {
            if (c_ci) HIPCHK(hipMemcpy(c_ci, bc->cci.p, sizeof(int32_t) * bc->nmoved, hipMemcpyDeviceToHost));
            if (c_val) HIPCHK(hipMemcpy(c_val, bc->cval.p, sizeof(double) * bc->nmoved, hipMemcpyDeviceToHost));
        }
    })
}
int pls_hessenberg_eigenvalues(int m,const double *H, int ldh, double *re, double *im) {
    return hessenberg_eigenvalues(m, H, ldh, re, im);
}
int pls_reset_timings(pls_handle *hh) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        H.timers.reset();
        H.coupling.n_reduced = H.coupling.n_full = 0;
    })
}
int pls_get_reuse_stats(pls_handle *hh, int64_t *stats) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        if (!stats) throw Error("pls_get_reuse_stats: null argument");
        stats[0] = H.coupling.n_reduced;
        stats[1] = H.coupling.n_full;
        stats[2] = H.coupling.eligible ? 1 : 0;
    })
}
int pls_get_reuse_wide(pls_handle *hh, int64_t *stats) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        if (!stats) throw Error("pls_get_reuse_wide: null argument");
        const Coupling &R = H.coupling;
        stats[0] = R.eligible ? R.wide_rows : 0;
        stats[1] = R.eligible && R.wide_rows ? R.wlpr : 0;
        stats[2] = R.eligible ? R.reuse_rows : 0;
        stats[3] = R.eligible ? R.reduced.bytes() : 0;
    })
}

int pls_export_matrix(pls_handle *hh, int which, int64_t *nrows, int64_t *nnz, int64_t *row_ptr, int32_t *col,
                      double *val) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        const DevCSR &M = which == 0 ? H.A : which == 1 ? H.P : H.Pd;
        if (!M.rp.p) throw Error("matrix not available (freed after setup, or not generated)");
        *nrows = M.nrows;
        *nnz = M.nnz;
        if (col) {
            HIPCHK(hipMemcpy(row_ptr, M.rp.p, sizeof(int64_t) * (M.nrows + 1), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(col, M.ci.p, sizeof(int32_t) * M.nnz, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(val, M.val.p, sizeof(double) * M.nnz, hipMemcpyDeviceToHost));
        }
    })
}
int pls_get_permutation(pls_handle *hh, int64_t *perm) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        std::copy(H.perm.begin(), H.perm.end(), perm);
    })
}

int pls_bench_spmv(pls_handle *hh, const double *d_x, double *d_y, int32_t reps, double *sec_per_launch) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        H.A.tag = 1;
        build_sell(H.A, H.ctx);
        hipEvent_t a, b;
        HIPCHK(hipEventCreate(&a));
        HIPCHK(hipEventCreate(&b));
        HIPCHK(hipEventRecord(a, H.ctx.st));
        for (int r = 0; r < reps; ++r) spmv(H.A, d_x, d_y, H.ctx);
        HIPCHK(hipEventRecord(b, H.ctx.st));
        HIPCHK(hipEventSynchronize(b));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, a, b));
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
        *sec_per_launch = (double)ms * 1e-3 / std::max(1, reps);
    })
}

int pls_bench_spmv_single(pls_handle *hh, const double *d_x, double *d_y, int32_t reps, double *sec_per_launch) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        H.A.tag = 1;
        low_layout(H, "pls_bench_spmv_single");
        hipEvent_t a, b;
        HIPCHK(hipEventCreate(&a));
        HIPCHK(hipEventCreate(&b));
        HIPCHK(hipEventRecord(a, H.ctx.st));
        for (int r = 0; r < reps; ++r) spmv(H.A, d_x, d_y, H.ctx, 1.0, 0.0, nullptr, true);
        HIPCHK(hipEventRecord(b, H.ctx.st));
        HIPCHK(hipEventSynchronize(b));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, a, b));
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
        *sec_per_launch = (double)ms * 1e-3 / std::max(1, reps);
    })
}

// Host-only query of the classical-AMG setup (no device): level `level` of
// the hierarchy built from A with the options' prefix_pc_hypre_boomeramg_*
// values.  Outputs n, nc, P's nnz (the coarsest operator when level ==
// nlevels - 1); cf (n int8: 1 C, -1 F) and P's CSR arrays are written when
// non-NULL (call once for the sizes, then with buffers).
int pls_boomeramg_host_level(const pls_csr *A, const char *options, const char *prefix, int64_t level,
                             int64_t *nlevels, int64_t *n, int64_t *nc, int64_t *p_nnz, int8_t *cf, int64_t *p_rp,
                             int32_t *p_ci, double *p_v) {
    PLS_TRY({
        if (!A || A->nrows != A->ncols) throw Error("pls_boomeramg_host_level: square A required");
        Options o;
        o.parse(options);
        HostCSR H;
        H.nrows = H.ncols = A->nrows;
        H.rp.assign(A->row_ptr, A->row_ptr + A->nrows + 1);
        H.ci.assign(A->col, A->col + H.rp.back());
        H.v.assign(A->val, A->val + H.rp.back());
        std::vector<int8_t> cfv;
        HostCSR P;
        boomeramg_host_level(H, o, prefix ? prefix : "", level, *nlevels, *n, *nc, cfv, P);
        *p_nnz = (int64_t)P.ci.size();
        if (cf && !cfv.empty()) std::copy(cfv.begin(), cfv.end(), cf);
        if (p_rp && P.nrows > 0) std::copy(P.rp.begin(), P.rp.end(), p_rp);
        if (p_ci) std::copy(P.ci.begin(), P.ci.end(), p_ci);
        if (p_v) std::copy(P.v.begin(), P.v.end(), p_v);
    })
}

int pls_sparse_lu_analyze(const pls_csr *A, const char *options, double *stats, int64_t nstats, int32_t *perm,
                          int32_t *front_of, int32_t *parent) {
    PLS_TRY({
        if (!A || A->nrows != A->ncols) throw Error("pls_sparse_lu_analyze: square A required");
        if (A->nrows < 0 || !A->row_ptr || (A->nrows > 0 && !A->col))
            throw Error("pls_sparse_lu_analyze: negative size or null arrays");
        // the pattern is indexed directly by the symbolic analysis: validate it first
        if (A->row_ptr[0] != 0) throw Error("pls_sparse_lu_analyze: row_ptr[0] must be 0");
        for (int64_t i = 0; i < A->nrows; ++i)
            if (A->row_ptr[i + 1] < A->row_ptr[i]) throw Error("pls_sparse_lu_analyze: row_ptr must be nondecreasing");
        for (int64_t k = 0; k < A->row_ptr[A->nrows]; ++k)
            if (A->col[k] < 0 || A->col[k] >= A->ncols) throw Error("pls_sparse_lu_analyze: column index out of range");
        Options o;
        o.parse(options);
        HostCSR H;
        H.nrows = H.ncols = A->nrows;
        H.rp.assign(A->row_ptr, A->row_ptr + A->nrows + 1);
        H.ci.assign(A->col, A->col + H.rp.back());
        if (A->val) H.v.assign(A->val, A->val + H.rp.back());
        sparse_lu_analyze(H, o, stats, nstats, perm, front_of, parent);
    })
}

// Standalone AndersonAcceleration (lib/AndersonAcceleration.py:8-78) on its
// own stream and a single-rank communicator; the same mixer the block PC runs
// for "inner accel order" > 0.
struct AndersonObj {
    Ctx ctx;
    AndersonMixer mix;
};
int pls_anderson_create(int32_t order, int64_t n, pls_anderson **out) {
    PLS_TRY({
        if (!out) throw Error("pls_anderson_create: out is NULL");
        if (order < 0 || order > 15) throw Error("pls_anderson_create: order must be in 0..15");
        if (n < 0) throw Error("pls_anderson_create: negative length");
        auto *a = new AndersonObj();
        a->mix.init(order, n);
        *out = reinterpret_cast<pls_anderson *>(a);
    })
}
int pls_anderson_next(pls_anderson *aa, double *d_gk) {
    PLS_TRY({
        if (!aa) throw Error("pls_anderson_next: NULL object");
        AndersonObj &a = *reinterpret_cast<AndersonObj *>(aa);
        if (a.mix.n > 0 && !d_gk) throw Error("pls_anderson_next: NULL vector");
        // order 0: mk = 0 every call, x_k = g_k (AndersonAcceleration.py:69-70)
        if (a.mix.order > 0) a.mix.next(d_gk, a.ctx);
        a.ctx.sync();
    })
}
int pls_anderson_destroy(pls_anderson *a) { PLS_TRY(delete reinterpret_cast<AndersonObj *>(a)) }

// Latency of the solve's global sums (one batched all-reduce per
// CGS step, one per norm): reps x (global_sum_dev of `count` doubles + the
// stream sync the Krylov loop does to read them on the host), host clock.
int pls_bench_global_sum(pls_handle *hh, int32_t count, int32_t reps, double *sec_per_call) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        Ctx &c = H.ctx;
        if (count < 1 || count > 4096) throw Error("pls_bench_global_sum: count must be in 1..4096");
        DBuf<double> v(count);
        HIPCHK(hipMemsetAsync(v.p, 0, sizeof(double) * count, c.st));
        c.comm->global_sum_dev(v.p, count, c.st);  // warm (scratch allocation, first collective)
        c.sync();
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < reps; ++r) {
            c.comm->global_sum_dev(v.p, count, c.st);
            c.sync();
        }
        const auto t1 = std::chrono::steady_clock::now();
        *sec_per_call = std::chrono::duration<double>(t1 - t0).count() / std::max(1, reps);
    })
}

// New values (or patterns) of A, P, P_diff for the next solves, in the
// caller's ordering as for pls_create.  The block preconditioner is set up
// again before the next solve (PETSc re-runs PCSetUp when the operator state
// changes, as after the reference's bc.apply in every time step,
// lib/Poromechanics.py:70-86); the outer solver and AAR / inner Anderson
// histories persist, as the reference's objects do.
int pls_update_matrices(pls_handle *hh, const pls_csr *A, const pls_csr *P, const pls_csr *Pdiff) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        if (H.synth_rows) throw Error("pls_update_matrices: synthetic handles generate their matrices");
        if (H.distributed) throw Error("pls_update_matrices: not available for distributed handles");
        if (!P && !H.keep && H.setup_done)
            throw Error("pls_update_matrices: P was released after setup (pls.keep_matrices 0); pass P");
        const int64_t n = H.n;
        std::vector<int64_t> inv(n);
        for (int64_t i = 0; i < n; ++i) inv[H.perm[i]] = i;
        if (A) {
            H.coupling.eligible = false;  // (its reduced layout is of the old A)
            H.coupling_stale = true;
            upload_permuted(A, H, inv, H.A);
            H.A.sell.reset();
            H.A.tag = 1;
            if (H.solver_ready) build_sell(H.A, H.ctx);
            if (H.outer) H.outer->guess_reset();  // B = A X no longer holds (PETSc's operator-state check)
        }
        if (P) upload_permuted(P, H, inv, H.P);
        if (Pdiff) {
            upload_permuted(Pdiff, H, inv, H.Pd);
            H.have_Pd = true;
        }
        H.setup_done = false;
        // (the inner solvers are built again by the setup; the outer one persists)
        if (H.outer && !H.outer->cheb_explicit) H.outer->cheb_ready = false;
    })
}

int pls_bench_copy(int64_t bytes, int32_t reps, int32_t read_only, double *gbs) {
    PLS_TRY({
        const int64_t n = std::max<int64_t>(bytes / 8, 2) & ~(int64_t)1;
        DBuf<double> a(n), b(n);
        hipStream_t st;
        HIPCHK(hipStreamCreate(&st));
        HIPCHK(hipMemsetAsync(a.p, 0, sizeof(double) * n, st));
        launch_copy_probe(n, a.p, b.p, read_only ? 1 : 0, st);
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        HIPCHK(hipEventRecord(e0, st));
        for (int r = 0; r < std::max(1, reps); ++r) launch_copy_probe(n, a.p, b.p, read_only ? 1 : 0, st);
        HIPCHK(hipEventRecord(e1, st));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        *gbs = (read_only ? 1.0 : 2.0) * 8.0 * (double)n * std::max(1, reps) / (ms * 1e-3) / 1e9;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        (void)hipStreamDestroy(st);
    })
}

int pls_spmv_layout(pls_handle *hh, int32_t *d16, int64_t *matrix_bytes) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        build_sell(H.A, H.ctx);
        if (d16) *d16 = H.A.sell && H.A.sell->d16 ? 1 : 0;
        if (matrix_bytes) *matrix_bytes = H.A.sell ? H.A.sell->bytes() : 0;
    })
}

int pls_spmv_layout_single(pls_handle *hh, int32_t *d16, int64_t *matrix_bytes) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        build_sell(H.A, H.ctx);
        const bool ok = H.A.sell && H.A.sell->d16 && !H.A.sell->b3_nslices;
        if (d16) *d16 = ok ? 1 : 0;
        if (matrix_bytes) *matrix_bytes = ok ? H.A.sell->bytes_low() : 0;
    })
}

int pls_get_d16_share(pls_handle *hh, int32_t which, int64_t *stats) {
    PLS_TRY({
        Handle &H = *reinterpret_cast<Handle *>(hh);
        if (!stats) throw Error("pls_get_d16_share: null argument");
        if (which != 0 && which != 1) throw Error("pls_get_d16_share: which must be 0 (A) or 1 (the reduced outer layout)");
        if (which == 0) build_sell(H.A, H.ctx);
        const DevSELL *S = which == 0 ? H.A.sell.get() : H.coupling.eligible ? &H.coupling.reduced : nullptr;
        const bool d16 = S && S->d16;
        stats[0] = d16 && S->cls.p ? 1 : 0;
        stats[1] = d16 ? S->nslices : 0;
        stats[2] = d16 ? S->shared_slices : 0;
        stats[3] = d16 ? S->dstored : 0;
        stats[4] = H.ctx.d16_share_built;
    })
}

}  // extern "C"
