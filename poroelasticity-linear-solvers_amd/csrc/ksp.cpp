// ksp.cpp -- the PETSc-semantics Krylov solvers of libpls.so (declared in
// runtime.hpp): GMRES / FGMRES, CG, BiCGStab, Richardson, Chebyshev, PREONLY and
// KSPConvergedDefault.
//
// The algorithms follow PETSc as the reference configures it (reference
// lib/Solver.py:91-102 for the outer solver, lib/Preconditioner.py:94-118 for
// the inner ones): GMRES with classical Gram-Schmidt, Givens rotations,
// happy-breakdown test and BuildSoln (gmres.c, fgmres.c); CG (cg.c); BiCGStab
// (bcgs.c); Richardson (rich.c) and Chebyshev (cheby.c) without inner products
// when the norm type is none; KSPConvergedDefault (iterativ.c).  GMRES's
// scalar recurrences run on the host in double precision, as the CPU oracle
// evaluates them (Richardson and Chebyshev have none beyond a norm); CG's and
// BiCGStab's run on the device unless something needs each iteration on the
// host (KSP::device_loop_allowed).
#include "runtime.hpp"
#include "bccols.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace pls {

static_assert((int)CG_NS == (int)BC_NS, "CG and BiCGStab share the device state buffers");

void KSP::resolve_side_norm(const std::string &side, const std::string &nt) {
    // KSPSetUpNorms_Private for the types implemented here
    if (type == "preonly") {
        right = false;
        norm = "none";
        return;
    }
    if (type == "gmres" || type == "bcgs") {
        // left with the preconditioned norm or right with the unpreconditioned one; left by
        // default, and KSPGMRES goes right when only the unpreconditioned norm is asked for
        const bool gmres = type == "gmres";
        std::string s = side;
        if (s.empty()) s = (gmres && nt == "unpreconditioned") ? "right" : "left";
        const std::string nn = nt.empty() ? (s == "right" ? "unpreconditioned" : "preconditioned") : nt;
        const bool ok = (s == "left" && (nn == "preconditioned" || nn == "none")) ||
                        (s == "right" && (nn == "unpreconditioned" || nn == "none"));
        if (!ok)
            throw Error(std::string(gmres ? "KSPGMRES" : "KSPBCGS") + " (" + prefix + ") does not support norm " + nn +
                        " with pc side " + s);
        right = (s == "right");
        norm = nn;
        return;
    }
    if (type == "fgmres") {
        // KSPFGMRES: right preconditioning only, the true residual norm (or none)
        const std::string s = side.empty() ? "right" : side, nn = nt.empty() ? "unpreconditioned" : nt;
        if (s != "right" || (nn != "unpreconditioned" && nn != "none"))
            throw Error("KSPFGMRES (" + prefix + ") does not support norm " + nn + " with pc side " + s +
                        " (right preconditioning with norm unpreconditioned or none only)");
        right = true;
        norm = nn;
        return;
    }
    if (type == "cg") {
        if (!side.empty() && side != "left") throw Error("KSPCG (" + prefix + ") supports only left preconditioning");
        right = false;
        norm = nt.empty() ? "preconditioned" : nt;
        if (norm != "preconditioned" && norm != "unpreconditioned" && norm != "none")
            throw Error("KSPCG (" + prefix + "): unsupported norm type " + norm);
        return;
    }
    if (type == "richardson" || type == "chebyshev") {
        const std::string who = type == "chebyshev" ? "KSPCHEBYSHEV" : "KSPRICHARDSON";
        if (!side.empty() && side != "left")
            throw Error(who + " (" + prefix + ") supports only left preconditioning, not pc side " + side);
        right = false;
        norm = nt.empty() ? "preconditioned" : nt;
        if (norm != "preconditioned" && norm != "unpreconditioned" && norm != "none")
            throw Error(who + " (" + prefix + "): unsupported norm type " + norm);
        return;
    }
    throw Error("KSP type '" + type + "' (prefix " + prefix +
                ") is not available (supported: gmres, fgmres, cg, bcgs, preonly, richardson, chebyshev)");
}

// May this solve (CG or BiCGStab) run its recurrence on the device?  Not when
// something needs each iteration on the host, and only over a PC without a KSP
// of its own: the iterations enqueued past the end would count as inner solves
// and feed them frozen (or, after a divergence, NaN) vectors.
bool KSP::device_loop_allowed() const {
    return (type == "cg" ? cg_device : bcgs_device) && !monitor && time_limit <= 0 && maxit > 0 && maxit <= 10000000 &&
           !pc->holds_ksp();
}

void KSP::ensure_work(Ctx &c) {
    if (type == "gmres" || type == "fgmres") {
        // CGS dots of up to restart + 1 columns: one partial per (column, block)
        // (the context's default room, 136 columns at the largest grid, overflowed
        // past ~450 iterations of a 1.3M-row solve)
        c.ensure_partial(n, restart + 2);
        if (allocated_single != (int)basis_single) {  // the basis mode changed: nothing allocated fits
            allocated_single = (int)basis_single;
            allocated_k = -1;
            V.release();
            Vf.release();
            cbw.release();
            cbv.release();
        }
        if (basis_single && allocated_k != restart) {
            ldv = (n + 127) & ~(int64_t)127;  // 512-B aligned columns of floats; Z, fp64, has the same stride
            vf_canary = c.debug_bounds;
            Vf.alloc((size_t)(restart + 1) * ldv + (vf_canary ? Ctx::CANARY : 0));
            if (vf_canary)
                HIPCHK(hipMemsetAsync(Vf.p + (size_t)(restart + 1) * ldv, 0xA5, sizeof(float) * Ctx::CANARY, c.st));
            cbw.alloc(std::max<int64_t>(n, 1));
            cbv.alloc(std::max<int64_t>(n, 1));
            if (type == "fgmres") Z.alloc((size_t)restart * ldv);
            else t1.alloc(n);
            t2.alloc(n);
            dh.alloc(2 * restart + 4);
            allocated_k = restart;
        }
        if (allocated_k != restart) {
            ldv = (n + 63) & ~(int64_t)63;  // 512-B aligned columns (16-B loads), V and Z alike
            V.alloc((size_t)(restart + 1) * ldv);
            if (type == "fgmres") Z.alloc((size_t)restart * ldv);
            else t1.alloc(n);
            t2.alloc(n);
            dh.alloc(2 * restart + 4);  // two CGS passes of restart + 1 scalars each
            allocated_k = restart;
        }
        if (orthog == MGS && !mgs_part.p) {
            mgs_part.alloc(reduce_blocks(n));
            mgs_ticket.alloc(1);
        }
        return;
    }
    if (type == "richardson" || type == "chebyshev") {
        if (allocated_k != -2) {
            t1.alloc(n);  // r
            t2.alloc(n);  // z
            if (type == "chebyshev") t3.alloc(n);  // the iterate that is not in x
            allocated_k = -2;
        }
        return;
    }
    const bool bcgs = type == "bcgs";
    if (bcgs) c.ensure_partial(n, 2);
    if (allocated_k != 0) {
        for (DBuf<double> *v : {&t1, &t2, &t3, &t4}) v->alloc(n);  // CG: r z p w; BiCGStab: r rp p v ...
        if (bcgs) {
            for (DBuf<double> *v : {&t5, &t6, &t7}) v->alloc(n);  // ... s t, one scratch
            bcticket.alloc(4);
        }
        // the device state (solve_bcgs keeps its coefficients there too)
        cgS.alloc(CG_NS);
        cgI.alloc(CG_NI);
        allocated_k = 0;
    }
    if (device_loop_allowed() && cghist.n < (size_t)(maxit + 2)) cghist.alloc(maxit + 2);
}

int KSP::converged(int it, double r) {
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    if (it == 0) {
        rnorm0 = guess_rnorm0 > 0.0 ? guess_rnorm0 : r;  // (a guessed solve: ||b|| or ||B b||, solve_guessed)
        ttol = std::max(rtol * rnorm0, atol);
        if (time_limit > 0) t_start = now();
    }
    if (std::isnan(r) || std::isinf(r)) return DIVERGED_NANORINF;
    if (r <= ttol) return r < atol ? CONVERGED_ATOL : CONVERGED_RTOL;
    if (r >= dtol * rnorm0) return DIVERGED_DTOL;
    if (time_limit > 0 && it > 0 && now() - t_start > time_limit) return DIVERGED_TIME_LIMIT;
    return CONVERGED_ITERATING;
}

// Iteration `it` ended with residual norm r: history, monitor line, rnorm and
// (unless the norm type says there is nothing to test) the convergence test.
int KSP::record(int it, double r, bool test) {
    history.push_back(r);
    if (monitor) {
        printf("  %3d KSP Residual norm %.12e\n", it, r);
        fflush(stdout);
    }
    rnorm = r;
    return test ? converged(it, r) : CONVERGED_ITERATING;
}

void KSP::solve(const double *b, double *x, Ctx &c) {
    // pls_bc_columns lift: b' = b - C b first; the guess, the norms and the test below all see b'
    if (bc && bc->lifting()) b = bc->lift(b, c);
    history.clear();
    if (guess_nonzero || guess_fischer) solve_guessed(b, x, c);
    else run(b, x, c);
    stat_its += its;
    stat_max = std::max<int64_t>(stat_max, its);
    ++stat_solves;
    stat_div += reason < 0 ? 1 : 0;
    if (reason < 0) stat_last_neg = reason;
    c.check_bounds();
    if (vf_canary) check_basis_bounds(c);
    if (guess_canary) check_guess_bounds(c);
}

void KSP::run(const double *b, double *x, Ctx &c) {
    if (type == "preonly") {
        pc->apply(b, x, c);
        its = 1;
        reason = CONVERGED_ITS;
    } else {
        ensure_work(c);
        if (type == "gmres" || type == "fgmres") solve_gmres(b, x, c);
        else if (type == "richardson") solve_richardson(b, x, c);
        else if (type == "chebyshev") solve_chebyshev(b, x, c);
        else if (type == "cg") device_loop_allowed() ? solve_cg_dev(b, x, c) : solve_cg(b, x, c);
        else device_loop_allowed() ? solve_bcgs_dev(b, x, c) : solve_bcgs(b, x, c);  // bcgs: no other type is left
    }
}

// ------------------------------------------------------- the initial guess --
// KSPSolve with a guess: x0 = FormGuess(b) when a guess object exists, else the
// incoming x; r0 = b - A x0; the type's own zero-guess solve of A d = r0 (run: no solver loop knows of
// the guess, and restarts evaluate r0 - A d, which is b - A x to rounding); x = x0 + d; the space's update.
// KSPConvergedDefault with a nonzero guess measures rtol and dtol against ||b|| (right preconditioning,
// norm unpreconditioned) or ||B b|| (the preconditioned norm: one more PC application) instead of the first
// residual; where that norm is 0 the first residual stays.  The norms of b and r0 come back in one read-back.
namespace {
bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
constexpr double GUESS_REFORM = 1e-2;  // ||y'|| / ||y|| below which B's new column is formed again as A x'
}  // namespace

void KSP::ensure_guess(Ctx &c) {
    c.ensure_partial(n, guess_size + 2);
    const int64_t nn = std::max<int64_t>(n, 1);
    if (!gx0.p) {
        for (DBuf<double> *v : {&gx0, &gr0, &gy}) v->alloc(nn);
        gd.alloc(2 * GUESS_MAX + 16);  // alpha, two norms, the second pass's beta; three norms of a solve's start
    }
    if (guess_timing && !guess_ev[0])
        for (hipEvent_t &e : guess_ev) HIPCHK(hipEventCreate(&e));
    if (guess_fischer && !gX.p) {
        guess_ldv = (nn + 63) & ~(int64_t)63;  // 512-B aligned columns, the Krylov basis's stride
        guess_canary = c.debug_bounds;
        const size_t count = (size_t)guess_size * guess_ldv, guard = guess_canary ? Ctx::CANARY : 0;
        try {
            gX.alloc(count + guard);
            gB.alloc(count + guard);
        } catch (const Error &e) {
            gX.release();
            gB.release();
            (void)hipGetLastError();
            throw Error("ksp_guess_type fischer (" + prefix + "): the projection space of 2 x " +
                        std::to_string(guess_size) + " columns (" + std::to_string(2 * count * sizeof(double)) +
                        " bytes) could not be allocated: " + e.what());
        }
        if (guess_canary)
            for (DBuf<double> *v : {&gX, &gB})
                HIPCHK(hipMemsetAsync(v->p + count, 0xA5, sizeof(double) * Ctx::CANARY, c.st));
        guess_m = 0;
    }
}

// pls.debug_bounds: the guard doubles behind the two column stores, as check_basis_bounds checks the fp32 basis's
void KSP::check_guess_bounds(Ctx &c) {
    if (!gX.p) return;
    std::vector<unsigned char> g(sizeof(double) * Ctx::CANARY);
    for (DBuf<double> *v : {&gX, &gB}) {
        HIPCHK(hipMemcpyAsync(g.data(), v->p + (v->n - Ctx::CANARY), g.size(), hipMemcpyDeviceToHost, c.st));
        c.sync();
        for (size_t i = 0; i < g.size(); ++i)
            if (g[i] != 0xA5)
                throw Error("pls.debug_bounds: the canary behind the Fischer guess's columns (" + prefix +
                            ") was overwritten at byte +" + std::to_string(i));
    }
}

void KSP::guess_reset() {
    if (!guess_fischer) return;
    guess_m = 0;
    ++stat_guess_resets;
}

// FormGuess(b): alpha = B^T b (k_mdot, the global sum in rank order), x0 = sum_i alpha_i X_i with i
// ascending (k_lincomb).  Nothing is read back.
void KSP::guess_form(const double *b, double *x0, Ctx &c) {
    const int m = (int)guess_m;
    if (m == 0) {
        launch_set(n, 0.0, x0, c.st);
        return;
    }
    if (!aligned16(b)) {  // (a block's rows inside a longer vector: k_mdot loads 16 bytes)
        launch_copy(n, b, gy.p, c.st);
        b = gy.p;
    }
    launch_mdot(n, m, gB.p, guess_ldv, b, c.partials(n, m), gd.p, c.st);
    c.comm->global_sum_dev(gd.p, m, c.st);
    launch_lincomb(n, m, gX.p, guess_ldv, gd.p, x0, c.st);
}

// Update(b, x) of Fischer's model 2: y = A x, alpha = B^T y, x' = x - X alpha, y' = y - B alpha, and the
// pair (x', y') / ||y'|| appended when ||y'|| > tol ||y||.  A full space is emptied first.  The projection
// runs twice (beta = B^T y', x' -= X beta, y' -= B beta, in place in the new slot): one pass leaves B^T y' at
// eps ||y|| / ||y'||, and consecutive solutions of a time loop differ by 1e-3 .. 1e-6, so the columns lost
// their orthogonality within one fill of the space.  A solve that made no iteration returned the guess
// itself, a combination of the stored columns, for which ||y'|| is 0 in exact arithmetic and rounding
// noise when computed (1e-13 ||y||, above the default tol): it is counted as skipped without computing it,
// unless the space is full and about to be emptied.  Where ||y'|| < GUESS_REFORM ||y|| the new column of B is
// formed again as a product, so that B = A X holds to rounding for nearly dependent solutions too (a third
// product with A, for those updates only).  One read-back of the m + 2 scalars (one more when the space is
// emptied -- ||y|| first, which tells whether x is finite -- and when the column is formed again).
void KSP::guess_update(const double *x, Ctx &c) {
    if (its == 0 && guess_m > 0 && guess_m < guess_size) {
        ++stat_guess_skipped;
        return;
    }
    if (!aligned16(x)) {
        launch_copy(n, x, gx0.p, c.st);
        x = gx0.p;
    }
    double *y = gy.p, *d = gd.p;
    A->apply(x, y, c);
    if (basis_single) ++stat_co_double;  // (the guess products stay fp64)
    auto read_back = [&](int count) {
        double *hs = c.host_scalars(count);
        HIPCHK(hipMemcpyAsync(hs, d, sizeof(double) * count, hipMemcpyDeviceToHost, c.st));
        c.sync();
        return hs;
    };
    if (guess_m == guess_size) {
        launch_dot(n, y, y, c.partials(n, 1), d, c.st);
        c.comm->global_sum_dev(d, 1, c.st);
        if (!std::isfinite(read_back(1)[0])) return;  // x holds NaN or Inf: the space stays
        guess_m = 0;
        ++stat_guess_resets;
    }
    const int m = (int)guess_m;
    double *yo = gB.p + (int64_t)m * guess_ldv, *beta = d + m + 2;
    launch_mdot(n, m, gB.p, guess_ldv, y, c.partials(n, m), d, c.st);
    launch_dot(n, y, y, c.partials(n, 1), d + m, c.st);
    c.comm->global_sum_dev(d, m + 1, c.st);
    launch_guess_update(n, m, gX.p, gB.p, guess_ldv, d, x, y, c.partials(n, 1), d + m + 1, c.st);
    if (m > 0) {
        launch_mdot(n, m, gB.p, guess_ldv, yo, c.partials(n, m), beta, c.st);
        c.comm->global_sum_dev(beta, m, c.st);
        launch_guess_update(n, m, gX.p, gB.p, guess_ldv, beta, nullptr, nullptr, c.partials(n, 1), d + m + 1, c.st);
    }
    c.comm->global_sum_dev(d + m + 1, 1, c.st);
    const double *hs = read_back(m + 2);
    if (!std::isfinite(hs[m]) || !std::isfinite(hs[m + 1])) return;
    const double nu0 = std::sqrt(hs[m]), nu = std::sqrt(hs[m + 1]);
    if (nu > guess_tol * nu0 && nu > 0.0) {
        double *xo = gX.p + (int64_t)m * guess_ldv;
        launch_scale2(n, 1.0 / nu, xo, yo, c.st);
        if (nu < GUESS_REFORM * nu0) {
            // y' carries the rounding of y = A x, eps nu0, which is eps nu0 / nu of the normalised column
            // (7e-11 at nu = 1e-6 nu0): B's column is formed again as the product A x', projected once more
            // (the new column is orthogonal to the others to eps nu0 / nu only) and normalised again
            A->apply(xo, yo, c);
            if (basis_single) ++stat_co_double;  // (the guess products stay fp64)
            launch_mdot(n, m, gB.p, guess_ldv, yo, c.partials(n, m), beta, c.st);
            c.comm->global_sum_dev(beta, m, c.st);
            launch_guess_update(n, m, gX.p, gB.p, guess_ldv, beta, nullptr, nullptr, c.partials(n, 1), d + m + 1,
                                c.st);
            c.comm->global_sum_dev(d + m + 1, 1, c.st);
            const double nu2 = std::sqrt(read_back(m + 2)[m + 1]);
            if (!(nu2 > 0.0) || !std::isfinite(nu2)) return;  // (the slot is not counted: nothing was appended)
            launch_scale2(n, 1.0 / nu2, xo, yo, c.st);
        }
        ++guess_m;
    } else {
        ++stat_guess_skipped;
    }
}

void KSP::solve_guessed(const double *b, double *x, Ctx &c) {
    ensure_work(c);
    ensure_guess(c);
    double *x0 = gx0.p, *r0 = gr0.p, *d = gd.p + 2 * GUESS_MAX + 4;
    if (guess_timing) HIPCHK(hipEventRecord(guess_ev[0], c.st));
    if (guess_fischer) {
        guess_form(b, x0, c);
        ++stat_guess_formed;
    } else {
        launch_copy(n, x, x0, c.st);
    }
    A->residual(x0, b, r0, c);
    if (basis_single) ++stat_co_double;  // (the guess products stay fp64)
    const bool pnorm = norm == "preconditioned";
    launch_dot(n, b, b, c.partials(n, 1), d, c.st);
    launch_dot(n, r0, r0, c.partials(n, 1), d + 1, c.st);
    if (pnorm) {
        pc->apply(b, gy.p, c);
        launch_dot(n, gy.p, gy.p, c.partials(n, 1), d + 2, c.st);
    }
    c.comm->global_sum_dev(d, pnorm ? 3 : 2, c.st);
    if (guess_timing) HIPCHK(hipEventRecord(guess_ev[1], c.st));
    double *hs = c.host_scalars(3);
    HIPCHK(hipMemcpyAsync(hs, d, sizeof(double) * (pnorm ? 3 : 2), hipMemcpyDeviceToHost, c.st));
    c.sync();
    const double bn = std::sqrt(hs[0]), rn = std::sqrt(hs[1]);
    guess_last_reduction = rn / bn;
    guess_rnorm0 = norm == "none" ? 0.0 : pnorm ? std::sqrt(hs[2]) : bn;
    if (!(guess_rnorm0 > 0.0)) guess_rnorm0 = 0.0;  // (0, or NaN: the first residual's norm stays)
    struct Restore {
        double &v;
        ~Restore() { v = 0.0; }
    } restore{guess_rnorm0};
    run(r0, x, c);
    if (guess_timing) HIPCHK(hipEventRecord(guess_ev[2], c.st));
    launch_axpby(n, 1.0, x0, 1.0, x, c.st);  // x = x0 + d
    if (guess_fischer) guess_update(x, c);
    if (guess_timing) {  // everything the guess adds to the zero-guess solve: before it and after it
        float a = 0.f, u = 0.f;
        HIPCHK(hipEventRecord(guess_ev[3], c.st));
        HIPCHK(hipEventSynchronize(guess_ev[3]));
        HIPCHK(hipEventElapsedTime(&a, guess_ev[0], guess_ev[1]));
        HIPCHK(hipEventElapsedTime(&u, guess_ev[2], guess_ev[3]));
        guess_seconds = ((double)a + (double)u) * 1e-3;
    }
}

// pls.debug_bounds: the guard bytes behind the fp32 basis, as Ctx::check_bounds checks those behind the partials
void KSP::check_basis_bounds(Ctx &c) {
    if (!Vf.p || Vf.n < (size_t)Ctx::CANARY) return;
    std::vector<unsigned char> g(sizeof(float) * Ctx::CANARY);
    HIPCHK(hipMemcpyAsync(g.data(), Vf.p + (Vf.n - Ctx::CANARY), g.size(), hipMemcpyDeviceToHost, c.st));
    c.sync();
    for (size_t i = 0; i < g.size(); ++i)
        if (g[i] != 0xA5)
            throw Error("pls.debug_bounds: the canary behind the fp32 Krylov basis (" + prefix +
                        ") was overwritten at byte +" + std::to_string(i));
}

KSP::KSP() = default;

KSP::~KSP() {
    for (hipEvent_t e : guess_ev)
        if (e) (void)hipEventDestroy(e);
    if (stats && stat_solves)
        fprintf(stderr, "[ksp %s%s] %lld solves, %lld its (mean %.1f, max %lld)\n", prefix.c_str(), type.c_str(),
                (long long)stat_solves, (long long)stat_its, (double)stat_its / (double)stat_solves, (long long)stat_max);
}

// ---------------------------------------------------------- GMRES, FGMRES --
// KSPGMRES (left or right) and KSPFGMRES in one cycle.  FGMRES keeps the
// preconditioned vectors (Z_k = M^-1 V_k, written by the PC straight into
// column k of Z), so the PC may change from one application to the next: the
// solution is x += Z y -- no PC application in BuildSoln -- and the Givens
// estimate is the true residual norm (right preconditioning only,
// resolve_side_norm).  PETSc's FGMRES happy-breakdown bound differs from
// GMRES's only below the 1e-30 cap applied here.
//
// Compressed-basis GMRES (<prefix>pls_gmres_basis single; Aliaga, Anzt et al., "Compressed basis
// GMRES") is the same cycle over a basis stored in fp32.  Every basis vector is rounded once,
// v = fl32(w / ||w||), and the operator and the PC are applied to the promoted rounded vector
// (cbv), so the Arnoldi relation holds for the basis that is stored; w (cbw), every sum and the
// Hessenberg matrix stay fp64.  One cycle cannot reduce the residual by much more than fp32's
// unit roundoff, and its Givens estimate drifts from the true residual by then, hence two rules
// for that basis (norm type not none):
//   (a) the cycle ends once the estimate is <= basis_drop x the residual the cycle began with;
//   (b) a positive reason from the estimate ends the cycle, not the solve: x is built, the next
//       cycle start computes and records the true residual at the same its, and that value
//       decides -- at its == max_it too, where a failed check is DIVERGED_ITS.
// A forced or confirming cycle start appends one history entry, as any restart does.  With norm
// type none the fp32 basis records and tests nothing: max_it steps, CONVERGED_ITS.
void KSP::solve_gmres(const double *b, double *x, Ctx &c) {
    const bool flexible = type == "fgmres";
    const bool cb = basis_single;               // the fp32 basis: rules (a) and (b), the products counted
    const bool tested = !cb || norm != "none";  // (the double basis records and tests whatever the norm type)
    const bool hess_kept = keep_hess && !cb;
    // compressed operator: the Arnoldi products through the fp32 copy of A, a cycle being one step
    // of iterative refinement that the fp64 residual of the cycle start corrects
    const bool low = cb && operator_single;
    if (low && !A->has_low())
        throw Error(prefix + "pls_gmres_operator single: the operator of this solver is not a stored matrix");
    // where the vector that becomes column k lives before it is normalised, and which vector the
    // operator and the PC read for column k: the column of V itself, or cbw and cbv
    auto wcol = [&](int64_t k) { return cb ? cbw.p : V.p + k * ldv; };
    auto vcol = [&](int64_t k) { return cb ? cbv.p : V.p + k * ldv; };
    // column k = w / nrm: in place, or rounded into Vf and promoted into cbv
    auto normalise = [&](int64_t k, double nrm, double *w) {
        if (cb) launch_scale_round(n, 1.0 / nrm, w, Vf.p + k * ldv, cbv.p, c.st);
        else launch_scale(n, 1.0 / nrm, w, c.st);
    };
    const int64_t mk = restart;
    const double haptol = 1e-30;
    std::vector<double> HH((mk + 1) * (mk + 1), 0.0), cc(mk + 1, 0.0), ss(mk + 1, 0.0), grs(mk + 2, 0.0),
        nrs(mk + 1, 0.0), hcol(mk + 1, 0.0);
    auto H = [&](int64_t i, int64_t j) -> double & { return HH[(size_t)i * (mk + 1) + j]; };
    double *t1p = t1.p, *t2p = t2.p;  // (no t1 for fgmres: right, with the PC's output in Z)
    if (hess_kept) hess.assign((size_t)(mk + 1) * (mk + 1), 0.0);
    launch_set(n, 0.0, x, c.st);
    if (orthog == MGS && !cb) HIPCHK(hipMemsetAsync(mgs_ticket.p, 0, sizeof(unsigned), c.st));
    its = 0;
    reason = 0;
    bool first = true, confirming = false;
    while (true) {
        double *w0 = wcol(0);
        if (first) {
            launch_copy(n, b, right ? w0 : t1p, c.st);
        } else {
            A->apply(x, t2p, c);
            if (cb) ++stat_co_double;
            launch_waxpby(n, 1.0, b, -1.0, t2p, right ? w0 : t1p, c.st);
        }
        if (!right) pc->apply(t1p, w0, c);
        double res = c.norm2(n, w0);
        if (tested) reason = record(its, res);
        if (confirming) {
            ++stat_cb_confirm;
            if (!reason) ++stat_cb_failed;
        }
        confirming = false;
        if (res == 0.0) {
            reason = CONVERGED_ATOL;
            break;
        }
        if (cb) {
            if (reason) break;
            if (its >= maxit) {  // (a confirmation that failed at max_it, or max_it 0)
                reason = tested ? DIVERGED_ITS : CONVERGED_ITS;
                break;
            }
        }
        const double res0c = res;
        normalise(0, res, w0);
        std::fill(HH.begin(), HH.end(), 0.0);
        grs.assign(mk + 2, 0.0);
        grs[0] = res;
        int64_t loc_it = 0;
        int creason = reason;  // the cycle's reason, from its estimates (double basis: the cycle start's too)
        bool forced = false;
        while (!creason && !forced && loc_it < mk && its < maxit) {
            double *vk = vcol(loc_it), *w = wcol(loc_it + 1);
            if (right) {
                double *zk = flexible ? Z.p + loc_it * ldv : t1p;
                pc->apply(vk, zk, c);
                // (may continue a product the PC has just formed with zk)
                if (low) A->apply_after_low(*pc, zk, w, c);
                else A->apply_after(*pc, zk, w, c);
            } else {
                if (low) A->apply_low(vk, t1p, c);
                else A->apply(vk, t1p, c);
                pc->apply(t1p, w, c);
            }
            if (cb) ++(low ? stat_co_low : stat_co_double);
            const int k = (int)(loc_it + 1);
            const double tt = std::sqrt(cb ? gmres_orthogonalise(k, Vf.p, w, hcol.data(), c)
                                           : gmres_orthogonalise(k, V.p, w, hcol.data(), c));
            for (int j = 0; j < k; ++j) H(j, loc_it) = hcol[j];
            H(loc_it + 1, loc_it) = tt;
            if (hess_kept && first) {
                for (int j = 0; j < k; ++j) hess[(size_t)j + (size_t)loc_it * (mk + 1)] = hcol[j];
                hess[(size_t)k + (size_t)loc_it * (mk + 1)] = tt;
            }
            double hapbnd = std::fabs(tt / grs[loc_it]);
            if (hapbnd > haptol) hapbnd = haptol;
            const bool hapend = tt < hapbnd;
            if (!hapend) normalise(loc_it + 1, tt, w);
            // KSPGMRESUpdateHessenberg
            const int64_t it = loc_it;
            for (int64_t j = 0; j < it; ++j) {
                const double t0 = H(j, it);
                H(j, it) = cc[j] * t0 + ss[j] * H(j + 1, it);
                H(j + 1, it) = cc[j] * H(j + 1, it) - ss[j] * t0;
            }
            if (!hapend) {
                const double t0 = std::sqrt(H(it, it) * H(it, it) + H(it + 1, it) * H(it + 1, it));
                if (t0 == 0.0) {
                    creason = DIVERGED_NULL;
                    break;
                }
                cc[it] = H(it, it) / t0;
                ss[it] = H(it + 1, it) / t0;
                grs[it + 1] = -(ss[it] * grs[it]);
                grs[it] = cc[it] * grs[it];
                H(it, it) = cc[it] * H(it, it) + ss[it] * H(it + 1, it);
                res = std::fabs(grs[it + 1]);
            } else {
                res = 0.0;
            }
            loc_it++;
            its++;
            if (tested) creason = record(its, res);
            if (hapend && !creason) {
                creason = DIVERGED_BREAKDOWN;
                break;
            }
            // rule (a), where the cycle would otherwise go on
            forced = cb && tested && !creason && basis_drop > 0.0 && res <= basis_drop * res0c && loc_it < mk &&
                     its < maxit;
        }
        // KSPGMRESBuildSoln: x += M^-1 V y (right), V y (left), Z y (fgmres; Z is fp64)
        const int64_t it = loc_it - 1;
        if (it >= 0) {
            if (H(it, it) == 0.0) {
                creason = DIVERGED_BREAKDOWN;
            } else {
                nrs[it] = grs[it] / H(it, it);
                for (int64_t k = it - 1; k >= 0; --k) {
                    double t0 = grs[k];
                    for (int64_t j = k + 1; j <= it; ++j) t0 = t0 - H(k, j) * nrs[j];
                    nrs[k] = t0 / H(k, k);
                }
                HIPCHK(hipMemcpyAsync(dh.p, nrs.data(), sizeof(double) * (it + 1), hipMemcpyHostToDevice, c.st));
                if (cb && !flexible) launch_lincomb(n, (int)(it + 1), Vf.p, ldv, dh.p, t2p, c.st);
                else launch_lincomb(n, (int)(it + 1), flexible ? Z.p : V.p, ldv, dh.p, t2p, c.st);
                if (right && !flexible) {
                    pc->apply(t2p, t1p, c);
                    launch_axpby(n, 1.0, t1p, 1.0, x, c.st);
                } else {
                    launch_axpby(n, 1.0, t2p, 1.0, x, c.st);
                }
                c.sync();  // nrs host buffer reuse
            }
        }
        first = false;
        if (creason < 0 || (creason && !cb)) {
            reason = creason;
            break;
        }
        if (creason > 0) {  // rule (b)
            confirming = true;
            continue;
        }
        if (its >= maxit) {
            reason = tested ? DIVERGED_ITS : CONVERGED_ITS;
            break;
        }
        if (forced) ++stat_cb_forced;
    }
}

// The orthogonalisation of one Arnoldi step (PETSc's gborthog.c rules) against the k columns of
// the basis B -- V, or Vf read as floats and promoted:
//   CGS            h = V^T w, w -= V h in one multi-vector kernel each (refine_never);
//                  refine_always runs the pair again on the updated w and adds the second
//                  pass's l_j to h_j here, in double; refine_ifneeded does so exactly when
//                  ||w|| after the first pass is smaller than sqrt(sum_j h_j^2) (j ascending)
//   MGS            for j ascending: h_j = (w, v_j), w -= h_j v_j -- k dependent reductions,
//                  so k + 1 launches of one step kernel (the update by h_{j-1} fused into the
//                  launch that sums (w, v_j); the last one sums (w, w)), each reading its
//                  coefficient from dh, where the launch before it left it.  k_final and the
//                  global sum sit between the steps; with pls.gmres_mgs_fused, on one rank and
//                  over the double basis, the last block to arrive finishes each sum in its
//                  launch instead (not the default: 4 % slower at 10M rows, a tie at 2,669;
//                  DESIGN.md section 15).  The same order of summation either way: bitwise the
//                  same on one rank.
// The k + 1 scalars come to the host in one read-back per pass.
template <class T>
double KSP::gmres_orthogonalise(int k, const T *B, double *w, double *h, Ctx &c) {
    double *hs = c.host_scalars(k + 1);
    auto read_back = [&](const double *d) {
        HIPCHK(hipMemcpyAsync(hs, d, sizeof(double) * (k + 1), hipMemcpyDeviceToHost, c.st));
        c.sync();
    };
    ++stat_orth_steps;
    if (orthog == MGS) {
        const bool fuse = mgs_fused && c.comm->size == 1 && !basis_single;
        for (int j = 0; j <= k; ++j) {
            launch_mgs_step(n, j > 0 ? B + (int64_t)(j - 1) * ldv : nullptr, j > 0 ? dh.p + (j - 1) : nullptr,
                            j < k ? B + (int64_t)j * ldv : nullptr, w, mgs_part.p, dh.p + j,
                            fuse ? mgs_ticket.p : nullptr, c.st);
            if (!fuse) {
                launch_final(n, 1, mgs_part.p, dh.p + j, c.st);
                c.comm->global_sum_dev(dh.p + j, 1, c.st);
            }
        }
        read_back(dh.p);
        std::copy(hs, hs + k, h);
        return hs[k];
    }
    auto cgs_pass = [&](double *d) {
        launch_mdot(n, k, B, ldv, w, c.partials(n, k), d, c.st);
        c.comm->global_sum_dev(d, k, c.st);
        launch_maxpy_norm(n, k, B, ldv, d, w, c.partials(n, 1), d + k, c.st);
        c.comm->global_sum_dev(d + k, 1, c.st);
        read_back(d);
    };
    cgs_pass(dh.p);
    std::copy(hs, hs + k, h);
    bool again = orthog == CGS_ALWAYS;
    if (orthog == CGS_IFNEEDED) {
        double hh = 0.0;
        for (int j = 0; j < k; ++j) hh += h[j] * h[j];
        again = std::sqrt(hs[k]) < std::sqrt(hh);
    }
    if (again) {
        ++stat_orth_second;
        cgs_pass(dh.p + k + 1);
        for (int j = 0; j < k; ++j) h[j] += hs[j];
    }
    return hs[k];
}

// ----------------------------------------------- the device-resident loops --
// What solve_cg_dev and solve_bcgs_dev share.  The scalar recurrence runs in a
// one-thread state kernel; iterations are enqueued in batches -- 1 per
// read-back for the first 32, growing to 8 -- with one read-back of (done, its,
// reason, hcount) per batch instead of several scalar read-backs per iteration.
// Iterations enqueued after the solve ended run their products and PC applies
// on frozen vectors (the vector updates and every state phase check the done
// flag): x, the iteration count, the reason and the history are the host
// driver's, bit for bit.
CgParams KSP::cg_params() const {
    return CgParams{rtol, atol, dtol, maxit, norm != "none" ? 1 : 0, CONVERGED_RTOL, CONVERGED_ATOL, DIVERGED_DTOL,
                    DIVERGED_NANORINF, DIVERGED_ITS, DIVERGED_INDEFINITE_PC, DIVERGED_INDEFINITE_MAT};
}

// the state a solve starts from: the scalars s0, zero integers and (BiCGStab's device loop) zero tickets
void KSP::reset_state(const std::vector<double> &s0, bool tickets, Ctx &c) {
    const std::vector<int64_t> i0(CG_NI, 0);
    HIPCHK(hipMemcpyAsync(cgS.p, s0.data(), sizeof(double) * CG_NS, hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemcpyAsync(cgI.p, i0.data(), sizeof(int64_t) * CG_NI, hipMemcpyHostToDevice, c.st));
    if (tickets) HIPCHK(hipMemsetAsync(bcticket.p, 0, sizeof(unsigned) * 4, c.st));
    c.sync();  // (the host vectors go out of scope only after the copies)
}

template <class Enqueue>
void KSP::device_loop(Ctx &c, Enqueue enqueue) {
    double *hb = c.host_scalars(CG_NI);
    int64_t i = 0;
    while (i < maxit) {
        // (at most 8 per batch: iterations enqueued past the end are wasted work --
        // batches of 32 cost more than the read-backs they saved, swelling N=80)
        const int64_t B = std::min<int64_t>(std::clamp<int64_t>(i / 16, 1, 8), maxit - i);
        for (int64_t k = 0; k < B; ++k, ++i) enqueue(i);
        HIPCHK(hipMemcpyAsync(hb, cgI.p, sizeof(int64_t) * CG_NI, hipMemcpyDeviceToHost, c.st));
        c.sync();
        int64_t d = 0;
        std::memcpy(&d, hb + CG_DONE, sizeof(d));
        if (d) break;
    }
    int64_t st[CG_NI];
    std::memcpy(st, hb, sizeof(st));
    its = (int)st[CG_ITS];
    reason = (int)st[CG_REASON];
    if (st[CG_HCOUNT] > 0) {
        std::vector<double> hh(st[CG_HCOUNT]);
        HIPCHK(hipMemcpyAsync(hh.data(), cghist.p, sizeof(double) * hh.size(), hipMemcpyDeviceToHost, c.st));
        c.sync();
        history.insert(history.end(), hh.begin(), hh.end());
        rnorm = hh.back();
    }
}

// ----------------------------------------------------------------------- CG --
// KSPSolve_CG, zero initial guess.  Work vectors: r t1, z t2, p t3, w t4.  Two
// drivers over the same operations: solve_cg keeps the scalars on the host,
// solve_cg_dev runs the recurrence on the device (k_cg_state, device_loop).

// what the two drivers share: the start (false: ended at iteration 0), up to beta = (z, r)
bool KSP::cg_begin(const double *b, double *x, Ctx &c, double &beta) {
    double *r = t1.p, *z = t2.p;
    launch_set(n, 0.0, x, c.st);
    launch_copy(n, b, r, c.st);
    double dp = 0.0;
    if (norm == "preconditioned") {
        pc->apply(r, z, c);
        dp = c.norm2(n, z);
    } else if (norm == "unpreconditioned") {
        dp = c.norm2(n, r);
    }
    its = 0;
    reason = record(0, dp, norm != "none");
    if (reason) return false;
    if (norm != "preconditioned") pc->apply(r, z, c);
    beta = c.dot(n, z, r);
    return true;
}

void KSP::solve_cg(const double *b, double *x, Ctx &c) {
    double *r = t1.p, *z = t2.p, *p = t3.p, *w = t4.p;
    double beta = 0.0, betaold = 0.0, dpi = 0.0, dpiold = 0.0, dp = 0.0;
    if (!cg_begin(b, x, c, beta)) return;
    int64_t i = 0;
    while (true) {
        its = (int)(i + 1);
        if (beta == 0.0) {
            reason = CONVERGED_ATOL;
            break;
        }
        // cg.c: (z, r) changing sign means an indefinite PC (e.g. ILU(0) of an
        // undrained solid block with negative pivots): stop with that reason
        // instead of iterating to max_it
        if (i > 0 && beta * betaold < 0.0) {
            reason = DIVERGED_INDEFINITE_PC;
            break;
        }
        if (i == 0) launch_copy(n, z, p, c.st);
        else launch_axpby(n, 1.0, z, beta / betaold, p, c.st);
        dpiold = dpi;
        A->apply(p, w, c);
        dpi = c.dot(n, p, w);
        betaold = beta;
        auto sgn = [](double v) { return (v > 0) - (v < 0); };
        if (dpi == 0.0 || (i > 0 && sgn(dpi) * sgn(dpiold) < 0)) {
            reason = DIVERGED_INDEFINITE_MAT;
            break;
        }
        const double a = beta / dpi;
        launch_axpby(n, a, p, 1.0, x, c.st);
        launch_axpby(n, -a, w, 1.0, r, c.st);
        if (norm == "preconditioned") {
            pc->apply(r, z, c);
            dp = c.norm2(n, z);
        } else if (norm == "unpreconditioned") {
            dp = c.norm2(n, r);
        } else {
            dp = 0.0;
        }
        reason = record((int)(i + 1), dp, norm != "none");
        if (reason) break;
        if (norm != "preconditioned") pc->apply(r, z, c);
        beta = c.dot(n, z, r);
        i++;
        if (i >= maxit) break;
    }
    if (i >= maxit && !reason) reason = DIVERGED_ITS;
}

void KSP::solve_cg_dev(const double *b, double *x, Ctx &c) {
    double *r = t1.p, *z = t2.p, *p = t3.p, *w = t4.p;
    double beta0 = 0.0;
    if (!cg_begin(b, x, c, beta0)) return;
    std::vector<double> s0(CG_NS, 0.0);
    s0[CG_BETA] = beta0;
    s0[CG_ONE] = 1.0;
    s0[CG_RNORM0] = rnorm0;
    s0[CG_TTOL] = ttol;
    reset_state(s0, false, c);
    const CgParams prm = cg_params();
    double *S = cgS.p, *hist = cghist.p;
    int64_t *I = cgI.p;
    const int64_t *done = I + CG_DONE;
    auto sum_into = [&](const double *u, const double *v, double *slot) {
        launch_dot(n, u, v, c.partials(n, 1), slot, c.st);
        c.comm->global_sum_dev(slot, 1, c.st);
    };
    device_loop(c, [&](int64_t i) {
        launch_cg_state(CG_TOP, i, S, I, hist, prm, c.st);
        if (i == 0) launch_copy(n, z, p, c.st);
        else launch_axpby_dev(n, S + CG_ONE, z, S + CG_BB, p, done, c.st);  // p = z + (beta / betaold) p
        A->apply(p, w, c);
        sum_into(p, w, S + CG_SLOT);
        launch_cg_state(CG_MID, i, S, I, hist, prm, c.st);
        launch_axpby_dev(n, S + CG_A, p, S + CG_ONE, x, done, c.st);     // x += a p
        launch_axpby_dev(n, S + CG_NEGA, w, S + CG_ONE, r, done, c.st);  // r -= a w
        if (norm == "preconditioned") {
            pc->apply(r, z, c);
            sum_into(z, z, S + CG_SLOT);
        } else if (norm == "unpreconditioned") {
            sum_into(r, r, S + CG_SLOT);
        }
        launch_cg_state(CG_POST, i, S, I, hist, prm, c.st);
        if (norm != "preconditioned") pc->apply(r, z, c);
        sum_into(z, r, S + CG_SLOT2);
        launch_cg_state(CG_END, i, S, I, hist, prm, c.st);
    });
}

// ------------------------------------------------------------- BiCGStab --
// KSPSolve_BCGS, zero initial guess.  K = M^-1 A (left, the preconditioned
// residual's norm) or A M^-1 (right, the true residual's norm; x = M^-1 x at
// the end).  Work vectors: r t1, rp t2, p t3, v t4, s t5, t t6, scratch t7.
// Two drivers over the same vector kernels (coefficients read from the device
// state S): solve_bcgs keeps the scalars on the host, solve_bcgs_dev runs the
// recurrence on the device (device_loop); x, the iteration count, the reason
// and the history are the same, bit for bit.
namespace {
constexpr int BC_PENDING = 1 << 20;  // (t, t) == 0: decided on the host (bcgs_end)
}

bool KSP::bcgs_begin(const double *b, double *x, Ctx &c, double &rho0) {
    double *r = t1.p, *rp = t2.p, *p = t3.p, *v = t4.p;
    launch_set(n, 0.0, x, c.st);
    if (right) launch_copy(n, b, r, c.st);
    else pc->apply(b, r, c);
    const double dp = (norm != "none") ? c.norm2(n, r) : 0.0;
    its = 0;
    reason = record(0, dp, norm != "none");
    if (reason) return false;
    launch_copy(n, r, rp, c.st);
    launch_set(n, 0.0, p, c.st);
    launch_set(n, 0.0, v, c.st);
    rho0 = c.dot(n, r, rp);
    return true;
}

void KSP::bcgs_end(double *x, Ctx &c) {
    double *p = t3.p, *s = t5.p, *tmp = t7.p;
    if (reason == BC_PENDING) {
        // t = K s vanished: converged when s did too (x += alpha p), else a breakdown
        if (c.dot(n, s, s) != 0.0) {
            reason = DIVERGED_BREAKDOWN;
        } else {
            launch_axpby_dev(n, cgS.p + BC_ALPHA, p, cgS.p + BC_ONE, x, nullptr, c.st);
            its++;
            history.push_back(0.0);
            rnorm = 0.0;
            reason = CONVERGED_RTOL;
        }
    }
    if (right) {
        pc->apply(x, tmp, c);
        launch_copy(n, tmp, x, c.st);
    }
}

// out = K in, through the scratch vector
void KSP::bcgs_K(const double *in, double *out, Ctx &c) {
    double *tmp = t7.p;
    if (right) {
        pc->apply(in, tmp, c);
        A->apply(tmp, out, c);
    } else {
        A->apply(in, tmp, c);
        pc->apply(tmp, out, c);
    }
}

void KSP::solve_bcgs(const double *b, double *x, Ctx &c) {
    double *r = t1.p, *rp = t2.p, *p = t3.p, *v = t4.p, *s = t5.p, *t = t6.p;
    double rho = 0.0;
    if (!bcgs_begin(b, x, c, rho)) return;
    double *S = cgS.p;
    int64_t *I = cgI.p;
    const int64_t *never = I + CG_DONE;  // stays 0: the host ends this loop
    double *hs = c.host_scalars(8);      // [0, 2): sums read back, [4, 6): coefficients on their way up
    std::vector<double> s0(BC_NS, 0.0);
    s0[BC_ONE] = 1.0;
    reset_state(s0, false, c);
    auto put2 = [&](int slot, double a0, double a1) {  // (the previous upload ran before the last read-back)
        hs[4] = a0;
        hs[5] = a1;
        HIPCHK(hipMemcpyAsync(S + slot, hs + 4, sizeof(double) * 2, hipMemcpyHostToDevice, c.st));
    };
    auto sums = [&](int rows) {
        launch_final(n, rows, c.partials(n, rows), S + BC_SLOT0, c.st);
        c.comm->global_sum_dev(S + BC_SLOT0, rows, c.st);
        HIPCHK(hipMemcpyAsync(hs, S + BC_SLOT0, sizeof(double) * rows, hipMemcpyDeviceToHost, c.st));
        c.sync();
    };
    const BcgsFuse nofuse{nullptr, 0, 0, S, I, nullptr, BcgsParams{}};
    double rhoold = 1.0, alpha = 1.0, omegaold = 1.0;
    int64_t i = 0;
    while (true) {
        const double beta = (rho / rhoold) * (alpha / omegaold);
        put2(BC_BETA, beta, omegaold * beta);
        launch_bcgs_p(n, r, v, p, S, never, c.st);
        bcgs_K(p, v, c);
        launch_bcgs_dot(n, v, rp, c.partials(n, 1), nofuse, never, c.st);
        sums(1);
        double d1 = hs[0];
        if (d1 == 0.0) {
            reason = DIVERGED_BREAKDOWN;
            break;
        }
        alpha = rho / d1;
        put2(BC_ALPHA, alpha, -alpha);
        launch_waxpby_dev(n, S + BC_ONE, r, S + BC_NEGALPHA, v, s, never, c.st);  // s = r - alpha v
        bcgs_K(s, t, c);
        launch_dot2(n, s, t, c.partials(n, 2), nofuse, never, c.st);
        sums(2);
        d1 = hs[0];
        const double d2 = hs[1];
        if (d2 == 0.0) {
            reason = BC_PENDING;
            break;
        }
        const double omega = d1 / d2;
        put2(BC_OMEGA, omega, -omega);
        launch_bcgs_update(n, p, s, t, rp, x, r, c.partials(n, 2), nofuse, never, c.st);
        sums(2);
        const double dp = (norm != "none") ? std::sqrt(hs[0]) : 0.0;
        const double rho_this = rho;
        rhoold = rho;
        omegaold = omega;
        rho = hs[1];  // (r, rp): the next iteration's rho
        its = (int)(i + 1);
        reason = record((int)(i + 1), dp, norm != "none");
        if (reason) break;
        if (rho_this == 0.0) {
            reason = DIVERGED_BREAKDOWN;
            break;
        }
        i++;
        if (i >= maxit) {
            reason = DIVERGED_ITS;
            break;
        }
    }
    bcgs_end(x, c);
}

void KSP::solve_bcgs_dev(const double *b, double *x, Ctx &c) {
    double *r = t1.p, *rp = t2.p, *p = t3.p, *v = t4.p, *s = t5.p, *t = t6.p;
    double rho0 = 0.0;
    if (!bcgs_begin(b, x, c, rho0)) return;
    double *S = cgS.p, *hist = cghist.p;
    int64_t *I = cgI.p;
    const int64_t *done = I + CG_DONE;
    // one launch per sum only where no global sum has to sit between the final sum and the state
    const bool fuse = bcgs_fused && c.comm->size == 1;
    std::vector<double> s0(BC_NS, 0.0);
    const double beta = (rho0 / 1.0) * (1.0 / 1.0);
    s0[BC_RHO] = rho0;
    s0[BC_RHOOLD] = s0[BC_ALPHA] = s0[BC_OMEGA] = s0[BC_OMEGAOLD] = s0[BC_ONE] = 1.0;
    s0[BC_BETA] = beta;
    s0[BC_C1] = 1.0 * beta;
    s0[BC_RNORM0] = rnorm0;
    s0[BC_TTOL] = ttol;
    reset_state(s0, true, c);
    const BcgsParams prm{cg_params(), DIVERGED_BREAKDOWN, BC_PENDING};
    auto how = [&](int phase, int64_t i, int tk) {
        return BcgsFuse{fuse ? bcticket.p + tk : nullptr, phase, i, S, I, hist, prm};
    };
    auto after = [&](int rows, int phase, int64_t i) {
        if (fuse) return;
        launch_final(n, rows, c.partials(n, rows), S + BC_SLOT0, c.st);
        c.comm->global_sum_dev(S + BC_SLOT0, rows, c.st);
        launch_bcgs_state(phase, i, S, I, hist, prm, c.st);
    };
    device_loop(c, [&](int64_t i) {
        launch_bcgs_p(n, r, v, p, S, done, c.st);
        bcgs_K(p, v, c);
        launch_bcgs_dot(n, v, rp, c.partials(n, 1), how(BC_MID1, i, 0), done, c.st);
        after(1, BC_MID1, i);
        launch_waxpby_dev(n, S + BC_ONE, r, S + BC_NEGALPHA, v, s, done, c.st);  // s = r - alpha v
        bcgs_K(s, t, c);
        launch_dot2(n, s, t, c.partials(n, 2), how(BC_MID2, i, 1), done, c.st);
        after(2, BC_MID2, i);
        launch_bcgs_update(n, p, s, t, rp, x, r, c.partials(n, 2), how(BC_POST, i, 2), done, c.st);
        after(2, BC_POST, i);
    });
    bcgs_end(x, c);
}

// --------------------------------------------------- Richardson, Chebyshev --
// KSPSolve_Richardson (no self-scaling) and KSPSolve_Chebyshev (first kind),
// left preconditioning, zero initial guess.  Neither takes an inner product:
// with norm type none the whole solve is enqueued without a read-back or a
// synchronisation and applies the same linear operator every time, so it is a
// legal preconditioner for plain GMRES.  With a norm the host loop reads one
// scalar back per iteration, as GMRES does.  Work vectors: r t1, z t2 and
// (Chebyshev) the iterate that is not in x, t3.  Every vector update is one
// launch of k_poly_update; over PCJacobi (and no preconditioned norm to form
// z = B r for) the PC's product happens in that launch too: two launches per
// iteration, the residual product and the update.
const double *KSP::poly_dinv() const {
    if (!poly_fuse_jacobi || norm == "preconditioned") return nullptr;
    const PCJacobi *j = dynamic_cast<const PCJacobi *>(pc);
    return j ? j->dinv.p : nullptr;
}

// rn(r): ||B r|| (z = B r is left in z) or ||r||
double KSP::poly_norm(const double *r, double *z, Ctx &c) {
    if (norm == "preconditioned") {
        pc->apply(r, z, c);
        return c.norm2(n, z);
    }
    return c.norm2(n, r);
}

void KSP::poly_step(double a, const double *pm1, double b, const double *pk, double cz, const double *r, double *z,
                    bool z_done, double *out, Ctx &c) {
    if (const double *dinv = poly_dinv()) {
        launch_poly_update(n, a, pm1, b, pk, cz, dinv, r, out, c.st);
        return;
    }
    if (!z_done) pc->apply(r, z, c);
    launch_poly_update(n, a, pm1, b, pk, cz, nullptr, z, out, c.st);
}

void KSP::solve_richardson(const double *b, double *x, Ctx &c) {
    const bool normed = norm != "none", pnorm = norm == "preconditioned";
    double *rw = t1.p, *z = t2.p;
    const double *r = b;
    its = 0;
    reason = 0;
    rnorm = 0.0;
    for (int64_t i = 0; i < maxit; ++i) {
        if (normed) {
            reason = record((int)i, poly_norm(r, z, c));
            if (reason) break;
        }
        // x = 0 is never written: the first update omits the x term
        poly_step(0.0, nullptr, 1.0, i > 0 ? x : nullptr, rich_scale, r, z, pnorm, x, c);
        its++;
        if (i + 1 < maxit || normed) {
            A->residual(x, b, rw, c);
            r = rw;
        }
    }
    if (its == 0) launch_set(n, 0.0, x, c.st);
    if (reason) return;
    if (!normed) {
        reason = CONVERGED_ITS;
        return;
    }
    reason = record((int)std::max<int64_t>(maxit, 0), poly_norm(r, z, c));
    if (!reason) reason = DIVERGED_ITS;
}

void KSP::solve_chebyshev(const double *b, double *x, Ctx &c) {
    if (!cheb_ready) chebyshev_estimate(c);
    const bool normed = norm != "none", pnorm = norm == "preconditioned";
    const double scale = 2.0 / (cheb_emax + cheb_emin), alpha = 1.0 - scale * cheb_emin, mu = 1.0 / alpha,
                 omegaprod = 2.0 / alpha;
    double c_km1 = 1.0, c_k = mu;
    double *rw = t1.p, *z = t2.p;
    its = 0;
    reason = 0;
    rnorm = 0.0;
    if (normed) reason = record(0, poly_norm(b, z, c));
    if (!reason && maxit <= 0) reason = DIVERGED_ITS;
    if (reason) {
        launch_set(n, 0.0, x, c.st);
        return;
    }
    // two buffers take the iterates in turn (p_k+1 overwrites p_k-1); the one that update
    // maxit - 1, the last, writes is x, so a solve that runs to max_it ends without a copy
    auto buf = [&](int64_t j) { return (maxit - 1 - j) % 2 == 0 ? x : t3.p; };
    const double *pkm1 = nullptr;
    double *pk = buf(0);
    poly_step(0.0, nullptr, 0.0, nullptr, scale, b, z, pnorm, pk, c);
    its = 1;
    int64_t i = 1;
    for (; i < maxit; ++i) {
        its++;
        const double c_kp1 = 2.0 * mu * c_k - c_km1, omega = omegaprod * c_k / c_kp1;
        A->residual(pk, b, rw, c);
        if (normed) {
            reason = record((int)i, poly_norm(rw, z, c));
            if (reason) break;
        }
        double *out = buf(i);  // (i == 1: p_k-1 = 0, its term omitted)
        poly_step(1.0 - omega, pkm1, omega, pk, omega * scale, rw, z, pnorm, out, c);
        pkm1 = pk;
        pk = out;
        c_km1 = c_k;
        c_k = c_kp1;
    }
    if (!reason) {
        if (!normed) {
            reason = CONVERGED_ITS;
        } else {
            A->residual(pk, b, rw, c);
            reason = record((int)i, poly_norm(rw, z, c));
            if (!reason) reason = DIVERGED_ITS;
        }
    }
    if (pk != x) launch_copy(n, pk, x, c.st);
}

// PETSc's default bounds: cheb_steps Arnoldi steps of the left-preconditioned operator B A
// through the GMRES cycle of a child KSP (CGS, no refinement, no tolerance), the extreme real
// parts of the Hessenberg matrix's eigenvalues, transformed by ksp_chebyshev_esteig a,b,c,d.
// The right-hand side is a fixed function of the block-global row index (PETSc's is random):
// v_g = ((g + 1) * 2654435761 mod 2^32) / 2^32 - 0.5, the same vector on every rank count.
void KSP::chebyshev_estimate(Ctx &c) {
    const std::string who = "KSPCHEBYSHEV (" + prefix + "): ";
    const std::string ask = "; give " + prefix + "ksp_chebyshev_eigenvalues emin,emax";
    const MatOp *mo = dynamic_cast<const MatOp *>(A);
    if (!mo)
        throw Error(who + "the eigenvalue estimate needs the block-global row indices of an assembled operator, this one is matrix-free" + ask);
    const DevCSR &M = *mo->M;
    const Halo *halo = M.halo.get();
    if (halo && (halo->nlocal != n || (int64_t)halo->l2g.size() < n))
        throw Error(who + "the eigenvalue estimate needs the block-global row indices, this distributed operator has none" + ask);
    std::vector<double> v(n);
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t g = (uint64_t)(halo ? halo->l2g[i] : i);
        v[i] = (double)(((g + 1) * 2654435761ull) & 0xffffffffull) / 4294967296.0 - 0.5;
    }
    DBuf<double> rhs(std::max<int64_t>(n, 1)), sol(std::max<int64_t>(n, 1));
    launch_set(n, 1.0, rhs.p, c.st);
    const int64_t nglob = (int64_t)std::llround(c.dot(n, rhs.p, rhs.p));  // rows of the whole block
    if (n) HIPCHK(hipMemcpyAsync(rhs.p, v.data(), sizeof(double) * n, hipMemcpyHostToDevice, c.st));
    c.sync();
    const int64_t steps = std::min<int64_t>(cheb_steps, nglob);
    if (steps < 1) throw Error(who + "empty operator");
    if (!cheb_est) {
        cheb_est = std::make_unique<KSP>();
        KSP &k = *cheb_est;
        k.prefix = prefix + "esteig_";
        k.type = "gmres";
        k.right = false;
        k.norm = "preconditioned";
        k.orthog = CGS_NEVER;
        k.rtol = k.atol = 0.0;
        k.dtol = INFINITY;
        k.keep_hess = true;
        k.A = A;
        k.pc = pc;
        k.n = n;
    }
    KSP &k = *cheb_est;
    k.maxit = k.restart = steps;
    k.solve(rhs.p, sol.p, c);
    c.sync();
    const int m = k.its;
    double re[64], im[64];
    if (m < 1) throw Error(who + "the eigenvalue estimate made no Arnoldi step" + ask);
    if (hessenberg_eigenvalues(m, k.hess.data(), (int)(steps + 1), re, im))
        throw Error(who + "the Hessenberg eigenvalue iteration of the estimate did not converge" + ask);
    const double lo = *std::min_element(re, re + m), hi = *std::max_element(re, re + m);
    const double emin = cheb_tr[0] * lo + cheb_tr[1] * hi, emax = cheb_tr[2] * lo + cheb_tr[3] * hi;
    if (!(emin > 0.0 && emin < emax))
        throw Error(who + "estimated bounds " + std::to_string(emin) + ", " + std::to_string(emax) +
                    " are not 0 < emin < emax" + ask);
    cheb_raw[0] = lo;
    cheb_raw[1] = hi;
    cheb_emin = emin;
    cheb_emax = emax;
    cheb_ready = true;
}

namespace {
std::vector<double> comma_list(const std::string &text, const std::string &key) {
    std::vector<double> v;
    size_t a = 0;
    while (a <= text.size()) {
        const size_t b = std::min(text.find(',', a), text.size());
        try {
            size_t used = 0;
            const std::string tok = text.substr(a, b - a);
            v.push_back(std::stod(tok, &used));
            if (used != tok.size()) throw 0;
        } catch (...) {
            throw Error("option " + key + ": not a comma-separated list of numbers: " + text);
        }
        a = b + 1;
    }
    return v;
}
}  // namespace

std::unique_ptr<KSP> make_ksp(const std::string &prefix, const Options &o, const DevCSR *Amat, const DevCSR *Pmat,
                              const std::string &default_ksp, const std::string &default_pc, Ctx &c, double rtol,
                              double atol, double dtol, int64_t maxit, int64_t restart, PC *external_pc) {
    auto k = std::make_unique<KSP>();
    k->prefix = prefix;
    k->type = o.str(prefix + "ksp_type", default_ksp);
    k->rtol = o.num(prefix + "ksp_rtol", rtol);
    k->atol = o.num(prefix + "ksp_atol", atol);
    k->dtol = o.num(prefix + "ksp_divtol", dtol);
    k->maxit = o.integer(prefix + "ksp_max_it", maxit);
    k->restart = o.integer(prefix + "ksp_gmres_restart", restart);
    k->monitor = o.has(prefix + "ksp_monitor");
    k->stats = o.flag("pls.ksp_stats", false);
    k->cg_device = o.flag("pls.cg_device", true);
    if (prefix == "global_") k->time_limit = o.num("pls.solver_time_limit", 0.0);
    k->bcgs_device = o.flag("pls.bcgs_device", true);
    k->bcgs_fused = o.flag("pls.bcgs_fused_reduce", true);
    if (k->type == "gmres" || k->type == "fgmres") {
        // KSPSetFromOptions_GMRES reads the classical flag first, so the modified one wins when both
        // are given; the refinement type is CGS's alone (other types ignore all three options)
        const std::string key = prefix + "ksp_gmres_cgs_refinement_type", rt = o.str(key, "refine_never");
        if (rt == "refine_never") k->orthog = KSP::CGS_NEVER;
        else if (rt == "refine_ifneeded") k->orthog = KSP::CGS_IFNEEDED;
        else if (rt == "refine_always") k->orthog = KSP::CGS_ALWAYS;
        else throw Error(key + ": unknown value '" + rt + "' (refine_never, refine_ifneeded, refine_always)");
        if (o.flag(prefix + "ksp_gmres_modifiedgramschmidt", false)) k->orthog = KSP::MGS;
        k->mgs_fused = o.flag("pls.gmres_mgs_fused", false);
        // the precision the Krylov basis is stored in (other types ignore both options)
        const std::string bkey = prefix + "pls_gmres_basis", basis = o.str(bkey, "double");
        if (basis != "double" && basis != "single")
            throw Error(bkey + ": unknown value '" + basis + "' (double, single)");
        k->basis_single = basis == "single";
        const std::string dkey = prefix + "pls_gmres_basis_drop";
        k->basis_drop = o.num(dkey, 1e-6);
        if (!(k->basis_drop >= 0.0 && k->basis_drop < 1.0))
            throw Error(dkey + ": " + o.str(dkey, "") + " is outside 0 <= d < 1 (0 switches the rule off)");
        if (k->basis_single && k->orthog == KSP::MGS && k->mgs_fused)
            throw Error(bkey + " single is not available together with pls.gmres_mgs_fused 1 (" + prefix +
                        "ksp_gmres_modifiedgramschmidt): the fp32 step kernel has no single-launch sums");
        // the precision of the operator inside the Arnoldi step (the fp32 basis' cycle only)
        const std::string okey = prefix + "pls_gmres_operator", oper = o.str(okey, "double");
        if (oper != "double" && oper != "single")
            throw Error(okey + ": unknown value '" + oper + "' (double, single)");
        if (oper == "single" && !k->basis_single)
            throw Error(okey + " single requires " + bkey + " single: the low-precision operator runs inside the " +
                        "compressed-basis cycle, whose true residuals correct it");
        k->operator_single = oper == "single";
    }
    k->resolve_side_norm(o.str(prefix + "ksp_pc_side", ""), o.str(prefix + "ksp_norm_type", ""));
    {
        // the initial guess: ksp_initial_guess_nonzero (the outer KSP only) and KSPGuess
        const std::string nzkey = prefix + "ksp_initial_guess_nonzero", gkey = prefix + "ksp_guess_type";
        const std::string mkey = prefix + "ksp_guess_fischer_model", tkey = prefix + "ksp_guess_fischer_tol";
        if (o.flag(nzkey, false)) {
            if (prefix != "global_")
                throw Error(nzkey + ": a nonzero initial guess is available for the outer solver (global_) only, " +
                            "not for prefix '" + prefix + "': the block preconditioner's inner x vectors are scratch");
            if (k->type == "preonly")
                throw Error(nzkey + ": KSPPREONLY cannot start from a nonzero initial guess");
            k->guess_nonzero = true;
        }
        const std::string gt = o.str(gkey, "none");
        if (gt != "none" && gt != "fischer")
            throw Error(gkey + ": unknown value '" + gt + "' (available: none, fischer)");
        if (gt == "fischer") {
            if (k->type == "preonly")
                throw Error(gkey + " fischer is not available with ksp_type preonly (" + prefix + ")");
            k->guess_fischer = true;
            int64_t model = 2, size = 10;
            if (o.has(mkey)) {
                const std::vector<double> v = comma_list(o.str(mkey, ""), mkey);
                if (v.size() != 2 || v[0] != std::floor(v[0]) || v[1] != std::floor(v[1]))
                    throw Error(mkey + " takes <model>,<size> (one token of two integers)");
                model = (int64_t)v[0];
                size = (int64_t)v[1];
            }
            if (model != 2)
                throw Error(mkey + ": model " + std::to_string(model) + " is not available; only model 2 " +
                            "(least squares, valid for a nonsymmetric operator) is built");
            if (size < 1 || size > GUESS_MAX)
                throw Error(mkey + ": size " + std::to_string(size) + " is outside 1 <= size <= " +
                            std::to_string(GUESS_MAX));
            k->guess_size = size;
            k->guess_tol = o.num(tkey, 32.0 * 2.220446049250313e-16);
        }
        k->guess_timing = o.flag("pls.ksp_guess_timing", false);
        k->guess_last_reduction = std::nan("");
    }
    k->poly_fuse_jacobi = o.flag("pls.poly_fuse_jacobi", true);
    if (k->type == "richardson") {
        if (o.has(prefix + "ksp_richardson_self_scale"))
            throw Error("KSPRICHARDSON (" + prefix + "): ksp_richardson_self_scale is not available");
        k->rich_scale = o.num(prefix + "ksp_richardson_scale", 1.0);
    }
    if (k->type == "chebyshev") {
        const std::string who = "KSPCHEBYSHEV (" + prefix + "): ";
        if (o.has(prefix + "ksp_chebyshev_eigenvalues")) {
            const std::string key = prefix + "ksp_chebyshev_eigenvalues";
            const std::vector<double> v = comma_list(o.str(key, ""), key);
            if (v.size() != 2) throw Error(who + key + " takes emin,emax (one token)");
            if (!(v[0] > 0.0 && v[0] < v[1]))
                throw Error(who + key + " needs 0 < emin < emax, got " + o.str(key, ""));
            k->cheb_explicit = k->cheb_ready = true;
            k->cheb_emin = v[0];
            k->cheb_emax = v[1];
            k->cheb_raw[0] = k->cheb_raw[1] = std::nan("");
        }
        const std::string tkey = prefix + "ksp_chebyshev_esteig";
        if (o.has(tkey)) {
            const std::vector<double> v = comma_list(o.str(tkey, ""), tkey);
            if (v.size() != 4) throw Error(who + tkey + " takes a,b,c,d (one token)");
            std::copy(v.begin(), v.end(), k->cheb_tr);
        }
        k->cheb_steps = o.integer(prefix + "ksp_chebyshev_esteig_steps", 10);
        if (k->cheb_steps < 1 || k->cheb_steps > 64)
            throw Error(who + prefix + "ksp_chebyshev_esteig_steps must be between 1 and 64");
    }
    {
        // the Dirichlet columns of a bc.apply block (bccols.hpp): with lift or drop the operator, the PC and
        // the SpMV layout below are all built from the KSP's own K'
        const std::string key = prefix + "pls_bc_columns", how = o.str(key, "keep");
        if (how != "keep" && how != "lift" && how != "drop")
            throw Error(key + ": unknown value '" + how + "' (keep, lift, drop)");
        if (how != "keep") {
            if (external_pc)
                throw Error(key + " " + how + ": this solver was handed its preconditioner (the fp_ solver over a " +
                            "fieldsplit, the outer solver over the block preconditioner); set the option on the " +
                            "solvers inside it (fp_fieldsplit_0_, fp_fieldsplit_1_, s_, ...)");
            if (!Amat)
                throw Error(key + " " + how + ": the operator of this solver is not a stored matrix (the Schur " +
                            "complement of a fieldsplit)");
            if (Amat != Pmat)
                throw Error(key + " " + how + ": the operator and the preconditioner matrix of this solver differ");
            if (Amat->halo)
                throw Error(key + " " + how + ": the block is sharded over " +
                            std::to_string(c.comm ? c.comm->size : 1) +
                            " ranks, and a constrained column may be owned by another rank");
            k->bc = std::make_unique<BcColumns>();
            k->bc->build(*Amat, how == "lift" ? BcColumns::LIFT : BcColumns::DROP, key, c);
            if (k->bc->has_copy()) Amat = Pmat = &k->bc->Kp;
        }
    }
    if (Amat) {
        auto op = std::make_unique<MatOp>(Amat);
        if (k->operator_single) op->enable_low(c, prefix + "pls_gmres_operator single");
        k->owned_op = std::move(op);
        k->A = k->owned_op.get();
        k->n = Amat->nrows;
    } else if (k->operator_single) {
        throw Error(prefix + "pls_gmres_operator single: the operator of this solver is not a stored matrix");
    }
    if (external_pc) {
        k->pc = external_pc;
    } else {
        k->owned_pc = make_pc(o.str(prefix + "pc_type", default_pc), *Pmat, o, prefix, c);
        k->pc = k->owned_pc.get();
    }
    return k;
}

}  // namespace pls
