// bccols.hip -- kernels of <prefix>pls_bc_columns (bccols.hpp; host code in bccols.cpp).
//
// Detection and split run once per setup: one wave per row, grid-stride, the row walked in
// chunks of 64 stored entries.  Everything whose order matters is placed by a prefix, never by an
// atomic: the lists of rows come from exclusive scans of per-row flags, and a row's moved entries
// keep their stored order through a ballot and a popcount of the lanes below.  So the lists, C and
// the zeroed copy are the same bits on every run.
//
// The lift, b' = b - C b, runs before every solve.  C holds a few entries (5 per row on the FE
// blocks, where a constrained dof couples to one element patch) on a few rows scattered over the
// block, so the mapping is one lane per row of b': the thread that owns b'_i copies b_i and, where
// bit i of the row mask is set, finds its row of C (the word's base count plus the popcount of the
// lower bits) and subtracts the row's sum, taken serially in stored order.  A wave per row of C
// would leave 59 of 64 lanes idle and reduce across lanes in another order; a second launch, or a
// second writer for the rows of C, would need the copy to be ordered against it.  Here every entry
// of b' has one writer, in one launch, without atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "bccols.hpp"

namespace pls {

namespace {
constexpr int TPB = 256;
constexpr int WPB = TPB / 64;
constexpr int64_t GRID_MAX = 2048;
unsigned grid_for(int64_t work, int per_block) {
    const int64_t g = (work + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : (g > GRID_MAX ? GRID_MAX : g));
}
}  // namespace

__global__ __launch_bounds__(TPB) void k_bc_flag(int64_t n, const int64_t *__restrict__ rp,
                                                 const int32_t *__restrict__ ci, const double *__restrict__ val,
                                                 uint8_t *__restrict__ flag8, int64_t *__restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * WPB;
    for (int64_t row = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6); row < n; row += nwaves) {
        const int64_t s = rp[row], e = rp[row + 1];
        bool ok = true, diag = false;
        for (int64_t k = s + lane; k < e; k += 64) {
            const double v = val[k];
            if (ci[k] == row) {
                diag = true;
                ok = ok && v == 1.0;
            } else {
                ok = ok && v == 0.0;
            }
        }
        const bool f = __all(ok) && __any(diag);
        if (lane == 0) {
            flag8[row] = f ? 1 : 0;
            flag[row] = f ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(TPB) void k_bc_compact(int64_t n, const int64_t *__restrict__ flag,
                                                    const int64_t *__restrict__ pos, int32_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * TPB;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += stride)
        if (flag[i]) out[pos[i]] = (int32_t)i;
}

// FILL false: cnt / has.  FILL true: C's entries from cptr[row] on, the copy's values zeroed.
template <bool FILL>
__global__ __launch_bounds__(TPB) void k_bc_split(int64_t n, const int64_t *__restrict__ rp,
                                                  const int32_t *__restrict__ ci, double *val,
                                                  const uint8_t *__restrict__ flag8, int64_t *__restrict__ cnt,
                                                  int64_t *__restrict__ has, const int64_t *__restrict__ cptr,
                                                  int32_t *__restrict__ cci, double *__restrict__ cval) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * WPB;
    for (int64_t row = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6); row < n; row += nwaves) {
        const int64_t s = rp[row], e = rp[row + 1];
        int64_t o = FILL ? cptr[row] : 0;
        for (int64_t k0 = s; k0 < e; k0 += 64) {  // (wave-uniform bounds: every lane reaches the ballot)
            const int64_t k = k0 + lane;
            const bool in = k < e;
            const int32_t j = in ? ci[k] : -1;
            const bool cons = in && j != row && j >= 0 && j < n && flag8[j] != 0;
            const double v = cons ? val[k] : 0.0;
            const bool moved = cons && v != 0.0;
            const unsigned long long m = __ballot(moved);
            if (FILL) {
                if (cons) val[k] = 0.0;
                if (moved) {
                    const int64_t p = o + __popcll(m & ((1ull << lane) - 1ull));
                    cci[p] = j;
                    cval[p] = v;
                }
            }
            o += __popcll(m);
        }
        if (!FILL && lane == 0) {
            cnt[row] = o;
            has[row] = o > 0 ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(TPB) void k_bc_rowptr(int64_t nrc, int64_t n, const int32_t *__restrict__ crow,
                                                   const int64_t *__restrict__ cptr, int64_t *__restrict__ crp) {
    const int64_t stride = (int64_t)gridDim.x * TPB;
    for (int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x; k <= nrc; k += stride)
        crp[k] = k < nrc ? cptr[crow[k]] : cptr[n];
}

__global__ __launch_bounds__(TPB) void k_bc_mask(int64_t n, int64_t nw, const int64_t *__restrict__ has,
                                                 const int64_t *__restrict__ hpos, uint32_t *__restrict__ mask,
                                                 int32_t *__restrict__ base) {
    const int64_t stride = (int64_t)gridDim.x * TPB;
    for (int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x; w < nw; w += stride) {
        const int64_t r0 = w << 5;
        uint32_t m = 0;
        for (int t = 0; t < 32 && r0 + t < n; ++t)
            if (has[r0 + t]) m |= 1u << t;
        mask[w] = m;
        base[w] = (int32_t)hpos[r0];
    }
}

__global__ __launch_bounds__(TPB) void k_bc_lift(int64_t n, const double *__restrict__ b,
                                                 const uint32_t *__restrict__ mask, const int32_t *__restrict__ base,
                                                 const int64_t *__restrict__ crp, const int32_t *__restrict__ cci,
                                                 const double *__restrict__ cval, double *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * TPB;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) {
        double v = b[i];
        const uint32_t m = mask[i >> 5];
        const int bit = (int)(i & 31);
        if ((m >> bit) & 1u) {
            const int64_t k = base[i >> 5] + __popc(m & ((1u << bit) - 1u));
            double sum = 0.0;
            for (int64_t e = crp[k]; e < crp[k + 1]; ++e) sum += cval[e] * b[cci[e]];
            v -= sum;
        }
        out[i] = v;
    }
}

// -------------------------------------------------------------- launchers --
void launch_bc_flag(int64_t n, const int64_t *rp, const int32_t *ci, const double *val, uint8_t *flag8,
                    int64_t *flag, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_bc_flag, dim3(grid_for(n, WPB)), dim3(TPB), 0, st, n, rp, ci, val, flag8, flag);
}
void launch_bc_compact(int64_t n, const int64_t *flag, const int64_t *pos, int32_t *out, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_bc_compact, dim3(grid_for(n, TPB)), dim3(TPB), 0, st, n, flag, pos, out);
}
void launch_bc_split_count(int64_t n, const int64_t *rp, const int32_t *ci, const double *val,
                           const uint8_t *flag8, int64_t *cnt, int64_t *has, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_bc_split<false>, dim3(grid_for(n, WPB)), dim3(TPB), 0, st, n, rp, ci,
                       const_cast<double *>(val), flag8, cnt, has, (const int64_t *)nullptr, (int32_t *)nullptr,
                       (double *)nullptr);
}
void launch_bc_split_fill(int64_t n, const int64_t *rp, const int32_t *ci, double *val, const uint8_t *flag8,
                          const int64_t *cptr, int32_t *cci, double *cval, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_bc_split<true>, dim3(grid_for(n, WPB)), dim3(TPB), 0, st, n, rp, ci, val, flag8,
                       (int64_t *)nullptr, (int64_t *)nullptr, cptr, cci, cval);
}
void launch_bc_rowptr(int64_t nrc, int64_t n, const int32_t *crow, const int64_t *cptr, int64_t *crp,
                      hipStream_t st) {
    hipLaunchKernelGGL(k_bc_rowptr, dim3(grid_for(nrc + 1, TPB)), dim3(TPB), 0, st, nrc, n, crow, cptr, crp);
}
void launch_bc_mask(int64_t n, const int64_t *has, const int64_t *hpos, uint32_t *mask, int32_t *base,
                    hipStream_t st) {
    if (n <= 0) return;
    const int64_t nw = (n + 31) / 32;
    hipLaunchKernelGGL(k_bc_mask, dim3(grid_for(nw, TPB)), dim3(TPB), 0, st, n, nw, has, hpos, mask, base);
}
void launch_bc_lift(int64_t n, const double *b, const uint32_t *mask, const int32_t *base, const int64_t *crp,
                    const int32_t *cci, const double *cval, double *out, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_bc_lift, dim3(grid_for(n, TPB)), dim3(TPB), 0, st, n, b, mask, base, crp, cci, cval, out);
}

}  // namespace pls
