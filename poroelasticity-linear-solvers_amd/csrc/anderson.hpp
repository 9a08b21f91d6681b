// anderson.hpp -- Anderson acceleration: the least squares of its steps, the
// vector histories, the update, the mixer the block PC runs for "inner accel
// order" > 0 (and pls_anderson_*), and the AAR outer solver (anderson.cpp).
#pragma once
#include <deque>

#include "runtime.hpp"

namespace pls {

// Least squares min ||f + F a|| by a Householder TSQR of the panel [F | f].
struct AndersonLS {
    DBuf<const double *> dptr;  // column pointers of every TSQR level
    DBuf<double> lvl[2];        // ping-pong stacks of R's
    DBuf<double> Rdev;          // m x m, then G x m x m gathered
    std::vector<double> solve(const std::vector<const double *> &cols, const double *f, int64_t n, Ctx &c);
};

struct RingVecs {
    DBuf<double> store;
    int cap = 0;
    int64_t n = 0;
    std::deque<int> live;
    std::vector<int> free_;
    void init(int capacity, int64_t n_);
    double *slot(int s) const { return store.p + (int64_t)s * n; }
    // append a copy of v; pop the oldest when more than `keep` remain
    void append(const double *v, int keep, Ctx &c);
    int size() const { return (int)live.size(); }
    const double *at(int i) const { return slot(live[i]); }
};

// y = y + beta * f + sum_{i<mk} alpha_i (X_i + beta F_i)   (AAR.py:109-111): the first mk
// vectors of both histories and alpha staged on the device, one launch, one sync
struct AndersonUpdate {
    DBuf<const double *> pX, pF;
    DBuf<double> dalpha;
    void alloc();
    void run(int64_t mk, const RingVecs &X, const RingVecs &F, const std::vector<double> &alpha, double beta,
             const double *f, double *y, Ctx &c);
};

struct AndersonMixer {  // lib/AndersonAcceleration.py:19-78
    int order = 0;
    int64_t k = 0;
    int64_t n = 0;
    DBuf<double> xk, fk, dxk, dfk;
    RingVecs F, X;
    AndersonLS ls;
    AndersonUpdate upd;
    void init(int order_, int64_t n_);
    void next(double *gk, Ctx &c);
};

struct AAR {  // lib/AAR.py
    int order = 10, p = 5;
    double omega = 1.0, beta = 1.0, atol = 1e-8, rtol = 1e-6;
    int64_t maxiter = 500, n = 0;
    bool monitor = false;
    RingVecs F, X;
    AndersonLS ls;
    AndersonUpdate upd;
    DBuf<double> xk, fk, dxk, dfk, tmp;
    // pls.aar_order / aar_p / aar_omega / aar_beta, pls.solver_monitor; the histories and work vectors
    void configure(const Options &o, int64_t n_, double atol_, double rtol_, int64_t maxiter_);
    // x0 = 0; history[k] = ||M (b - A x_k)||; res: its, rnorm, reason
    void solve(Op &A, PC &M, const double *b, double *x, Ctx &c, Timers &timers, std::vector<double> &history,
               pls_result &res);
};

}  // namespace pls
