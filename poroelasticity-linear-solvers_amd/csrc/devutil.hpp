// devutil.hpp -- device-side helpers that more than one kernel file uses (kernels.hip, ilu0.hip,
// sweep_lds.hip).  Included by .hip files only; a helper with one user lives in that user's
// file.  Everything here is static or inline: no device symbol crosses a translation unit (the
// library links without -fgpu-rdc).
//
// Contraction state: this header sets none and every file includes it first, so its helpers
// (row_dot is the one with floating-point arithmetic) compile under the compiler's default for
// device code, which fuses multiply-adds across statements.  A kernel file sets
// `#pragma clang fp contract` itself, after the include:
//   kernels.hip    the default up to the synthetic section (wave_reduce), contract(off) inside
//                  it, contract(on) everywhere after it
//   ilu0.hip       contract(on); contract(off) around the factorization (ilu0_row, k_ilu0_level,
//                  k_ilu0_dep), which rounds as the CPU restatement does
//   sweep_lds.hip  contract(on) throughout
// A pragma holds where a function is written, not where it is instantiated: code that moves to
// a file of its own has to take the state of its section along, or its rounding changes.
#pragma once

#include "kernels.hpp"

namespace pls {

static constexpr int TPB = 256;

static inline unsigned grid_for(int64_t work, int per_block) {
    int64_t g = (work + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// first position in the sorted a[s, e) with a value >= v (kernels.hip extraction, ilu0.hip k_find_diag)
__device__ __forceinline__ int64_t lower_bound_i32(const int32_t *a, int64_t s, int64_t e, int64_t v) {
    while (s < e) {
        const int64_t m = (s + e) >> 1;
        if ((int64_t)a[m] < v) s = m + 1; else e = m;
    }
    return s;
}

// (kernels.hip CSR SpMV, ilu0.hip level sweeps)
// Partial dot of a CSR row slice over LPR lanes, U entries per lane in flight:
// unconditional loads at a clamped index (s is valid inside the loop) and a
// masked value, so the loads of one pass issue back to back.
template <int LPR, int U, bool NT>
__device__ __forceinline__ double row_dot(int64_t s, int64_t e, int sub, const int32_t *__restrict__ ci,
                                          const double *__restrict__ val, const double *x) {
    double acc = 0.0;
    for (int64_t k0 = s; k0 < e; k0 += U * LPR) {
        int32_t c[U];
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t k = k0 + u * LPR + sub;
            const int64_t kk = k < e ? k : s;
            if (NT) {
                c[u] = __builtin_nontemporal_load(ci + kk);
                const double t = __builtin_nontemporal_load(val + kk);
                v[u] = k < e ? t : 0.0;
            } else {
                c[u] = ci[kk];
                const double t = val[kk];
                v[u] = k < e ? t : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc += v[u] * x[(uint32_t)c[u]];
    }
    return acc;
}

// Block of a row: explicit starts (binary search; nb + 1 entries) or PETSc's
// sizes (n / nb, the first n % nb blocks one longer).  b0 / len of the block.
__device__ __forceinline__ int64_t block_of(int64_t i, int64_t n, int64_t nb, const int64_t *bstart, int64_t &b0,
                                            int64_t &len) {
    if (bstart) {
        int64_t lo = 0, hi = nb;  // largest b with bstart[b] <= i
        while (hi - lo > 1) {
            const int64_t m = (lo + hi) >> 1;
            if (bstart[m] <= i) lo = m; else hi = m;
        }
        b0 = bstart[lo];
        len = bstart[lo + 1] - b0;
        return lo;
    }
    const int64_t q = n / nb, r = n % nb;
    const int64_t b = i < r * (q + 1) ? i / (q + 1) : r + (i - r * (q + 1)) / q;
    b0 = b * q + (b < r ? b : r);
    len = q + (b < r ? 1 : 0);
    return b;
}
__device__ __forceinline__ void block_range(int64_t b, int64_t n, int64_t nb, const int64_t *bstart, int64_t &b0,
                                            int64_t &len) {
    if (bstart) {
        b0 = bstart[b];
        len = bstart[b + 1] - b0;
        return;
    }
    const int64_t q = n / nb, r = n % nb;
    b0 = b * q + (b < r ? b : r);
    len = q + (b < r ? 1 : 0);
}

// Header entry of a lane's stream in the LDS and chain sweeps (the layout: sweep_lds.hip,
// "LDS sweep stream layout"): col = local row | (entries of this lane << SW_ROW_BITS).
static constexpr int SW_ROW_BITS = 18;
static constexpr int32_t SW_ROW_PAD = (1 << SW_ROW_BITS) - 1;  // local rows 0..262,142

__device__ __forceinline__ int64_t readlane64(int64_t v, int l) {
    const int32_t lo = __builtin_amdgcn_readlane((int32_t)(uint32_t)(uint64_t)v, l);
    const int32_t hi = __builtin_amdgcn_readlane((int32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// a double through a DPP lane permutation (no LDS round trip, unlike a shuffle)
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

}  // namespace pls
