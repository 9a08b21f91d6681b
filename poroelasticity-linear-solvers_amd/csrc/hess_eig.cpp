// hess_eig.cpp -- eigenvalues of a small upper Hessenberg matrix, plain host
// code without HIP or LAPACK (declared in runtime.hpp and, for tests, exported
// as pls_hessenberg_eigenvalues): what Chebyshev's eigenvalue estimate
// (ksp.cpp, KSP::chebyshev_estimate) needs from its Arnoldi steps.  The file
// includes nothing of the library's, so a stand-alone program can compile it
// alone (tools/micro/hess_eig_check.cpp).
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstddef>
#include <vector>

namespace pls {

int hessenberg_eigenvalues(int m, const double *H, int ldh, double *re, double *im);

// Shifted QR on the complex copy of an upper Hessenberg matrix: deflate where a
// subdiagonal entry is negligible against its diagonal neighbours, shift by the
// eigenvalue of the active block's trailing 2 x 2 that is nearer its last
// diagonal entry (Wilkinson), an exceptional shift every tenth sweep; one sweep
// is A - mu I = Q R by Givens rotations, A = R Q + mu I, on the active block
// alone (eigenvalues only).  m <= 64: a sweep is O(m^2).
int hessenberg_eigenvalues(int m, const double *H, int ldh, double *re, double *im) {
    using cd = std::complex<double>;
    if (m < 1 || m > 64 || !H || !re || !im || ldh < m) return 2;
    std::vector<cd> a((size_t)m * m, cd(0.0, 0.0));
    auto A = [&](int i, int j) -> cd & { return a[(size_t)i + (size_t)j * m]; };
    double anorm = 0.0;
    for (int j = 0; j < m; ++j)
        for (int i = 0; i <= std::min(j + 1, m - 1); ++i) {
            A(i, j) = H[(size_t)i + (size_t)j * ldh];
            anorm = std::max(anorm, std::fabs(H[(size_t)i + (size_t)j * ldh]));
        }
    if (std::isnan(anorm) || std::isinf(anorm)) return 3;
    const double eps = 2.220446049250313e-16;
    std::vector<cd> gc(m), gs(m);
    int hi = m - 1, sweeps = 0;
    while (hi >= 0) {
        int l = hi;
        while (l > 0) {
            double s = std::abs(A(l - 1, l - 1)) + std::abs(A(l, l));
            if (s == 0.0) s = anorm;
            if (std::abs(A(l, l - 1)) <= eps * s) {
                A(l, l - 1) = 0.0;
                break;
            }
            --l;
        }
        if (l == hi) {
            re[hi] = A(hi, hi).real();
            im[hi] = A(hi, hi).imag();
            --hi;
            sweeps = 0;
            continue;
        }
        if (++sweeps > 300) return 1;
        cd mu;
        if (sweeps % 10 == 0) {
            mu = A(hi, hi) + cd(std::abs(A(hi, hi - 1)) + (hi - 1 > l ? std::abs(A(hi - 1, hi - 2)) : 0.0), 0.0);
        } else {
            const cd p = A(hi - 1, hi - 1), q = A(hi - 1, hi), r = A(hi, hi - 1), t = A(hi, hi);
            const cd half = 0.5 * (p - t), disc = std::sqrt(half * half + q * r);
            const cd m1 = 0.5 * (p + t) + disc, m2 = 0.5 * (p + t) - disc;
            mu = std::abs(m1 - t) <= std::abs(m2 - t) ? m1 : m2;
        }
        for (int k = l; k <= hi; ++k) A(k, k) -= mu;
        for (int k = l; k < hi; ++k) {  // rows k, k + 1 <- G_k (rows k, k + 1), columns k .. hi
            const double rr = std::hypot(std::abs(A(k, k)), std::abs(A(k + 1, k)));
            if (rr == 0.0) {
                gc[k] = 1.0;
                gs[k] = 0.0;
                continue;
            }
            const cd cc = A(k, k) / rr, ss = A(k + 1, k) / rr;
            gc[k] = cc;
            gs[k] = ss;
            for (int j = k; j <= hi; ++j) {
                const cd u = A(k, j), v = A(k + 1, j);
                A(k, j) = std::conj(cc) * u + std::conj(ss) * v;
                A(k + 1, j) = -ss * u + cc * v;
            }
            A(k + 1, k) = 0.0;
        }
        for (int k = l; k < hi; ++k) {  // columns k, k + 1 <- (columns k, k + 1) G_k^H, rows l .. k + 1
            const cd cc = gc[k], ss = gs[k];
            for (int i = l; i <= k + 1; ++i) {
                const cd u = A(i, k), v = A(i, k + 1);
                A(i, k) = u * cc + v * ss;
                A(i, k + 1) = -std::conj(ss) * u + std::conj(cc) * v;
            }
        }
        for (int k = l; k <= hi; ++k) A(k, k) += mu;
    }
    return 0;
}

}  // namespace pls
