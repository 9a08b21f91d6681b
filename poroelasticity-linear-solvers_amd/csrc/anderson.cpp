// anderson.cpp -- Anderson acceleration (anderson.hpp): AndersonLS, RingVecs,
// the update kernel, AndersonMixer and AAR.
#include "anderson.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace pls {

// Least squares min ||f + F a|| for the Anderson steps.  The reference
// (lib/AAR.py:102-105, lib/AndersonAcceleration.py:62-65) gathers F and f to
// rank 0 and runs numpy's Householder QR, then solve(R, -Q^T f).  Here a
// Householder TSQR of the panel [F | f] on the device (k_tsqr: 512-row
// chunks, then the stacked R's, a fixed tree), one m x m R per rank; across
// ranks the R's are all-gathered (m^2 doubles each) and the stack is factored
// on the host in rank order.  The last column of R~ = [[R, z], [0, rho]]
// holds z = Q^T f in R's own sign convention, so a = R^-1 (-z) -- the same
// quantity numpy computes, by a Householder QR, so it stays backward stable up
// to cond(F) ~ 1/eps (no Gram matrix squares the condition number).  Only an
// exactly singular R fails, as numpy.linalg.solve raises LinAlgError.
static void householder_qr_host(std::vector<double> &A, int rows, int m) {  // column-major rows x m, in place
    for (int j = 0; j < m && j < rows; ++j) {
        double sigma = 0.0;
        for (int r = j + 1; r < rows; ++r) sigma += A[(size_t)j * rows + r] * A[(size_t)j * rows + r];
        const double alpha = A[(size_t)j * rows + j];
        if (sigma == 0.0) continue;
        const double nrm = std::sqrt(alpha * alpha + sigma);
        const double beta = alpha >= 0.0 ? -nrm : nrm, tau = (beta - alpha) / beta, scal = 1.0 / (alpha - beta);
        for (int k = j + 1; k < m; ++k) {
            double s = 0.0;
            for (int r = j + 1; r < rows; ++r) s += A[(size_t)j * rows + r] * A[(size_t)k * rows + r];
            const double w = A[(size_t)k * rows + j] + scal * s;
            A[(size_t)k * rows + j] -= tau * w;
            for (int r = j + 1; r < rows; ++r) A[(size_t)k * rows + r] -= tau * w * (A[(size_t)j * rows + r] * scal);
        }
        A[(size_t)j * rows + j] = beta;
    }
}

std::vector<double> AndersonLS::solve(const std::vector<const double *> &cols, const double *f, int64_t n, Ctx &c) {
    const int L = (int)cols.size();
    if (L < 1) return {};
    if (L + 1 > 16) throw Error("Anderson order > 15 not supported");
    const int m = L + 1;
    const int64_t C = tsqr_rows_per_block();
    // the TSQR tree: level 0 reads [F | f]; level l > 0 reads level l-1's stacked R's
    std::vector<int64_t> rows{std::max<int64_t>(n, 1)};
    while ((rows.back() + C - 1) / C > 1) rows.push_back(((rows.back() + C - 1) / C) * m);
    const int nlev = (int)rows.size();
    const size_t cap = (size_t)((rows[0] + C - 1) / C) * m * m;
    if (lvl[0].n < cap) { lvl[0].alloc(cap); lvl[1].alloc(cap); }
    if (dptr.n < (size_t)nlev * 16) dptr.alloc((size_t)nlev * 16);
    const int G = c.comm->size;
    if (Rdev.n < (size_t)(G + 1) * m * m) Rdev.alloc((size_t)(G + 1) * m * m);
    std::vector<const double *> hp((size_t)nlev * 16, nullptr);
    for (int k = 0; k < L; ++k) hp[k] = cols[k];
    hp[L] = f;
    for (int l = 1; l < nlev; ++l)
        for (int k = 0; k < m; ++k) hp[(size_t)l * 16 + k] = lvl[(l - 1) & 1].p + (size_t)k * rows[l];
    HIPCHK(hipMemcpyAsync((void *)dptr.p, hp.data(), sizeof(double *) * hp.size(), hipMemcpyHostToDevice, c.st));
    if (n == 0) HIPCHK(hipMemsetAsync(Rdev.p, 0, sizeof(double) * m * m, c.st));  // a rank without rows
    for (int l = 0; l < nlev && n > 0; ++l) {
        const bool last = l == nlev - 1;
        double *out = last ? Rdev.p : lvl[l & 1].p;
        const int64_t ldo = last ? m : ((rows[l] + C - 1) / C) * m;
        launch_tsqr(rows[l], m, dptr.p + (size_t)l * 16, out, ldo, c.st);
    }
    std::vector<double> R((size_t)m * m);
    if (G > 1) {
        double *gat = Rdev.p + (size_t)m * m;
        c.comm->allgather_dev(Rdev.p, m * m, gat, c.st);
        std::vector<double> S((size_t)G * m * m);
        HIPCHK(hipMemcpyAsync(S.data(), gat, sizeof(double) * S.size(), hipMemcpyDeviceToHost, c.st));
        c.sync();
        // stack the ranks' R's in rank order: (G m) x m column-major, then QR
        const int rows_s = G * m;
        std::vector<double> A((size_t)rows_s * m);
        for (int g = 0; g < G; ++g)
            for (int k = 0; k < m; ++k)
                for (int i = 0; i < m; ++i) A[(size_t)k * rows_s + g * m + i] = S[(size_t)g * m * m + (size_t)k * m + i];
        householder_qr_host(A, rows_s, m);
        for (int k = 0; k < m; ++k)
            for (int i = 0; i < m; ++i) R[(size_t)k * m + i] = i <= k ? A[(size_t)k * rows_s + i] : 0.0;
    } else {
        HIPCHK(hipMemcpyAsync(R.data(), Rdev.p, sizeof(double) * R.size(), hipMemcpyDeviceToHost, c.st));
        c.sync();
    }
    // R~ column-major: R(i, k) = R[k m + i]; z = R~(0:L, L)
    std::vector<double> a(L, 0.0);
    for (int i = L - 1; i >= 0; --i) {
        const double d = R[(size_t)i * m + i];
        if (d == 0.0) throw Error("Anderson least squares: singular R (numpy.linalg.solve raises LinAlgError)");
        double s = -R[(size_t)L * m + i];
        for (int k = i + 1; k < L; ++k) s -= R[(size_t)k * m + i] * a[k];
        a[i] = s / d;
    }
    return a;
}

void RingVecs::init(int capacity, int64_t n_) {
    cap = capacity;
    n = n_;
    store.alloc((size_t)std::max(cap, 1) * std::max<int64_t>(n, 1));
    live.clear();
    free_.clear();
    for (int i = cap - 1; i >= 0; --i) free_.push_back(i);
}

void RingVecs::append(const double *v, int keep, Ctx &c) {
    if (free_.empty()) { free_.push_back(live.front()); live.pop_front(); }
    int s = free_.back();
    free_.pop_back();
    launch_copy(n, v, slot(s), c.st);
    live.push_back(s);
    while ((int)live.size() > keep) { free_.push_back(live.front()); live.pop_front(); }
}

__global__ void k_anderson_update(int64_t n, int mk, const double *const *X, const double *const *F,
                                  const double *alpha, double beta, const double *f, double *y) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        // the oracle's operation order, no contraction (AAR.py:109-111)
        double v = __dadd_rn(y[e], __dmul_rn(beta, f[e]));
        for (int i = 0; i < mk; ++i) v = __dadd_rn(v, __dmul_rn(alpha[i], __dadd_rn(X[i][e], __dmul_rn(beta, F[i][e]))));
        y[e] = v;
    }
}

void AndersonUpdate::alloc() {
    pX.alloc(16);
    pF.alloc(16);
    dalpha.alloc(16);
}

void AndersonUpdate::run(int64_t mk, const RingVecs &X, const RingVecs &F, const std::vector<double> &alpha,
                         double beta, const double *f, double *y, Ctx &c) {
    std::vector<const double *> hx, hf;
    for (int64_t i = 0; i < mk; ++i) { hx.push_back(X.at((int)i)); hf.push_back(F.at((int)i)); }
    if (mk > 0) {
        HIPCHK(hipMemcpyAsync((void *)pX.p, hx.data(), sizeof(double *) * mk, hipMemcpyHostToDevice, c.st));
        HIPCHK(hipMemcpyAsync((void *)pF.p, hf.data(), sizeof(double *) * mk, hipMemcpyHostToDevice, c.st));
        HIPCHK(hipMemcpyAsync(dalpha.p, alpha.data(), sizeof(double) * mk, hipMemcpyHostToDevice, c.st));
    }
    k_anderson_update<<<2048, 256, 0, c.st>>>(X.n, (int)mk, pX.p, pF.p, dalpha.p, beta, f, y);
    c.sync();
}

void AndersonMixer::init(int order_, int64_t n_) {
    order = order_;
    n = n_;
    if (order <= 0) return;
    xk.alloc(n); fk.alloc(n); dxk.alloc(n); dfk.alloc(n);
    F.init(order + 1, n);
    X.init(order + 1, n);
    upd.alloc();
}

void AndersonMixer::next(double *gk, Ctx &c) {
    if (k == 0) {
        launch_set(n, 0.0, xk.p, c.st);
        launch_set(n, 0.0, fk.p, c.st);
    }
    launch_copy(n, fk.p, dfk.p, c.st);
    launch_copy(n, xk.p, dxk.p, c.st);
    launch_waxpby(n, 1.0, gk, -1.0, xk.p, fk.p, c.st);  // fk = gk - xk
    const int64_t mk = std::min<int64_t>(k, order);
    if (mk > 0) {
        launch_waxpby(n, 1.0, fk.p, -1.0, dfk.p, dfk.p, c.st);  // dfk = fk - dfk
        if (c.norm2(n, dfk.p) < 1e-12) {
            k -= 1;
            launch_copy(n, gk, xk.p, c.st);
        } else {
            F.append(dfk.p, order, c);
            std::vector<const double *> cols;
            for (int i = 0; i < F.size(); ++i) cols.push_back(F.at(i));
            std::vector<double> alpha = ls.solve(cols, fk.p, n, c);
            if ((int64_t)X.size() < mk || (int64_t)F.size() < mk)
                throw Error("AndersonAcceleration: history shorter than mk (reference raises IndexError)");
            upd.run(mk, X, F, alpha, 1.0, fk.p, xk.p, c);
        }
    } else {
        launch_copy(n, gk, xk.p, c.st);
    }
    launch_waxpby(n, 1.0, xk.p, -1.0, dxk.p, dxk.p, c.st);  // dxk = xk - dxk
    X.append(dxk.p, order, c);
    k += 1;
    launch_copy(n, xk.p, gk, c.st);
}

void AAR::configure(const Options &o, int64_t n_, double atol_, double rtol_, int64_t maxiter_) {
    n = n_;
    order = (int)o.integer("pls.aar_order", 10);
    p = (int)o.integer("pls.aar_p", 5);
    omega = o.num("pls.aar_omega", 1.0);
    beta = o.num("pls.aar_beta", 1.0);
    atol = atol_;
    rtol = rtol_;
    maxiter = maxiter_;
    monitor = o.flag("pls.solver_monitor", false);
    if (order > 15) throw Error("AAR order > 15 not supported");
    F.init(order + 1, n);
    X.init(order + 1, n);
    xk.alloc(n); fk.alloc(n); dxk.alloc(n); dfk.alloc(n); tmp.alloc(n);
    upd.alloc();
}

// lib/AAR.py:46-128 (single process: the rank-0 gathers are the identity).
void AAR::solve(Op &A, PC &M, const double *b, double *x, Ctx &c, Timers &timers, std::vector<double> &history,
                pls_result &res) {
    // x0 = 0; fk = b - A x0 = b
    launch_set(n, 0.0, xk.p, c.st);
    launch_copy(n, b, fk.p, c.st);
    const double error0 = c.norm2(n, fk.p);
    double err_abs = error0, err_rel = 1.0;
    int64_t it = 0;
    history.assign(1, error0);
    while (err_abs > atol && err_rel > rtol && it < maxiter) {
        launch_copy(n, fk.p, dfk.p, c.st);
        launch_copy(n, xk.p, dxk.p, c.st);
        // update_residual: temp = b - A xk ; fk = PC(temp)
        A.apply(xk.p, tmp.p, c);
        launch_waxpby(n, 1.0, b, -1.0, tmp.p, tmp.p, c.st);
        M.apply(tmp.p, fk.p, c);
        launch_waxpby(n, 1.0, fk.p, -1.0, dfk.p, dfk.p, c.st);  // dfk = fk - dfk
        F.append(dfk.p, order, c);
        const double fnorm = c.norm2(n, fk.p);
        const char *kind = "R";
        if (fnorm < 1e-14) {
            // no update (AAR.py:91-92)
        } else if (it == 0 || order == 0 || ((it + 1) % p) != 0) {
            launch_axpby(n, omega, fk.p, 1.0, xk.p, c.st);
        } else {
            kind = "A";
            const int64_t mk = std::min<int64_t>(order, it);
            std::vector<const double *> cols;
            for (int i = 0; i < F.size(); ++i) cols.push_back(F.at(i));
            std::vector<double> alpha = ls.solve(cols, fk.p, n, c);
            if ((int64_t)X.size() < mk) throw Error("AAR: history shorter than mk");
            upd.run(mk, X, F, alpha, beta, fk.p, xk.p, c);
        }
        launch_waxpby(n, 1.0, xk.p, -1.0, dxk.p, dxk.p, c.st);  // dxk = xk - dxk
        X.append(dxk.p, order, c);
        err_abs = fnorm;
        err_rel = err_abs / error0;
        it += 1;
        history.push_back(err_abs);
        if (monitor) printf("---- Iteration [%s] %3lld\tabs=%1.2e\trel=%1.2e\n", kind, (long long)it, err_abs, err_rel);
        timers.flush();
    }
    launch_copy(n, xk.p, x, c.st);
    c.sync();
    res.its = (int)it;
    res.rnorm = err_abs;
    res.reason = (err_abs <= atol) ? 3 : (err_rel <= rtol) ? 2 : -3;
}

}  // namespace pls
