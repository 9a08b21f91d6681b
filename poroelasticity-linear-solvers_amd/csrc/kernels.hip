// kernels.hip -- HIP kernels for gfx950 (MI355X / CDNA4) behind libpls.so.
//
// Everything on the solver path is HBM-bandwidth bound fp64 sparse / BLAS-1
// work (no MFMA).  Design rules applied (cdna_hip_programming.md):
//  * 64-lane wavefronts: CSR rows are mapped to groups of LPR lanes
//    (LPR in {8,16,32,64}) sized from the mean row length, reductions are
//    __shfl_xor trees inside the group;
//  * val / col streams use non-temporal loads (read once), the x gathers go
//    through L2 / the Infinity Cache (banded columns: hot window);
//  * reductions are deterministic: a fixed grid that depends only on n, one
//    partial per block, then a single-block final pass in fixed order, so a
//    solve is bitwise reproducible run to run.
// (ILU(0), the level tables and the level sweeps: ilu0.hip; the LDS sweeps: sweep_lds.hip.)
#include "devutil.hpp"

#include <hipcub/hipcub.hpp>

#include <type_traits>

namespace pls {

__device__ __forceinline__ double wave_reduce(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ============================================================ synthetic ====
// Bit-exact restatement of the synthetic spec; every float
// expression rounds as written (no FMA contraction) so the device matrices are
// identical to the CPU definition.
#pragma clang fp contract(off)

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t hash3(uint64_t s, uint64_t a, uint64_t b) {
    return mix64(mix64(mix64(s) ^ a) ^ b);
}
__device__ __forceinline__ double u01(uint64_t h) { return (double)(h >> 11) * 0x1.0p-53; }

#define SALT_VAL 0x5A1BE5ULL
#define SALT_DIAGA 0xD1A60AULL
#define SALT_DIAGP 0xD1A60BULL
#define SALT_BC 0x00BC00ULL
#define SALT_RHS 0x00B0B0ULL

__device__ __forceinline__ int blk_id(int a, int b) {
    // ss sf sp / sf ff fp / sp fp pp
    const int t = a * 3 + b;
    return (t == 0) ? 0 : (t == 1 || t == 3) ? 1 : (t == 2 || t == 6) ? 2 : (t == 4) ? 3 : (t == 5 || t == 7) ? 4 : 5;
}

__device__ __forceinline__ int field_of(const SynthDev &S, int64_t g) {
    return g < S.off[1] ? 0 : (g < S.off[2] ? 1 : 2);
}

// Visits the global columns of row i (local in field a) in ascending order.
template <typename F>
__device__ __forceinline__ void synth_visit(const SynthDev &S, int a, int64_t i, F &&f) {
    for (int b = 0; b < 3; ++b) {
        const int bid = blk_id(a, b);
        const int32_t *D = S.offs[bid];
        const int m = S.cnt[bid];
        const int64_t na = S.n[a], nb = S.n[b];
        if (a <= b) {
            const int64_t ctr = (a == b) ? i : (i * nb) / na;
            for (int k = 0; k < m; ++k) {
                const int64_t j = ctr + D[k];
                if (j >= 0 && j < nb) f(b, S.off[b] + j);
            }
        } else {
            for (int k = m - 1; k >= 0; --k) {
                const int64_t mm = i - D[k];
                if (mm < 0 || mm >= na) continue;
                const int64_t lo = (mm * nb + na - 1) / na;
                int64_t hi = ((mm + 1) * nb + na - 1) / na;
                if (hi > nb) hi = nb;
                for (int64_t j = lo; j < hi; ++j) f(b, S.off[b] + j);
            }
        }
    }
}

__device__ __forceinline__ int64_t synth_global_row(const SynthDev &S, int64_t l) {
    const int f = l < S.rloff[1] ? 0 : (l < S.rloff[2] ? 1 : 2);
    return S.off[f] + S.rlo[f] + (l - S.rloff[f]);
}

__global__ __launch_bounds__(TPB) void k_synth_count(SynthDev S, int64_t *row_len) {
    const int64_t n = S.nrows;
    const int64_t l = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (l > n) return;
    if (l == n) { row_len[n] = 0; return; }
    const int64_t g = synth_global_row(S, l);
    const int a = field_of(S, g);
    int64_t c = 0;
    synth_visit(S, a, g - S.off[a], [&](int, int64_t) { ++c; });
    row_len[l] = c;
}

__global__ __launch_bounds__(TPB) void k_synth_fill(SynthDev S, int variant, const int64_t *rp,
                                                    int32_t *col, double *val) {
    const int64_t l = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (l >= S.nrows) return;
    const int64_t g = synth_global_row(S, l);
    const int a = field_of(S, g);
    const int64_t i = g - S.off[a];
    const uint64_t sv = S.seed ^ SALT_VAL;
    const uint64_t sd = S.seed ^ (variant == 0 ? SALT_DIAGA : SALT_DIAGP);
    const bool bcrow = (variant == 2 && a == 2 &&
                        ((hash3(S.seed ^ SALT_BC, (uint64_t)i, 7ULL) & 15ULL) == 0ULL));
    int64_t pos = rp[l];
    int64_t dpos = -1;
    double sum = 0.0;
    synth_visit(S, a, i, [&](int b, int64_t gj) {
        col[pos] = (int32_t)gj;
        if (gj == g) {
            dpos = pos;
            val[pos] = 0.0;
        } else {
            const uint64_t lo = (uint64_t)(g < gj ? g : gj), hi = (uint64_t)(g < gj ? gj : g);
            const double u = u01(hash3(sv, lo, hi));
            const double v = (a == b) ? -u : -(0.1 * u);
            val[pos] = bcrow ? 0.0 : v;
            sum = sum + fabs(v);
        }
        ++pos;
    });
    if (dpos >= 0) {
        if (bcrow) {
            val[dpos] = 1.0;
        } else {
            const double u = u01(hash3(sd, (uint64_t)g, (uint64_t)g));
            const double sh = S.delta * (1.0 + u);
            val[dpos] = sum + sh;
        }
    }
}

__global__ __launch_bounds__(TPB) void k_synth_rhs(SynthDev S, uint64_t seed, double *b) {
    const int64_t l = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (l >= S.nrows) return;
    const int64_t i = synth_global_row(S, l);
    const double u = u01(hash3(seed ^ SALT_RHS, (uint64_t)i, 3ULL));
    b[l] = 2.0 * u - 1.0;
}

#pragma clang fp contract(on)

void launch_synth_count(const SynthDev &S, int64_t *row_len, hipStream_t st) {
    k_synth_count<<<grid_for(S.nrows + 1, TPB), TPB, 0, st>>>(S, row_len);
}
void launch_synth_fill(const SynthDev &S, int variant, const int64_t *row_ptr, int32_t *col,
                       double *val, hipStream_t st) {
    if (S.nrows > 0) k_synth_fill<<<grid_for(S.nrows, TPB), TPB, 0, st>>>(S, variant, row_ptr, col, val);
}
void launch_synth_rhs(const SynthDev &S, uint64_t seed, double *b, hipStream_t st) {
    if (S.nrows > 0) k_synth_rhs<<<grid_for(S.nrows, TPB), TPB, 0, st>>>(S, seed, b);
}

// ================================================================ scans ====
size_t exclusive_scan_tmp_bytes(int64_t n) {
    size_t bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const int64_t *)nullptr, (int64_t *)nullptr,
                                     (int)(n + 1));
    return bytes;
}
void exclusive_scan_i64(const int64_t *in, int64_t *out, int64_t n, void *tmp, size_t tmp_bytes,
                        hipStream_t st) {
    (void)hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, in, out, (int)(n + 1), st);
}

// ========================================================== extraction =====

__device__ __forceinline__ void window_of(const WindowSpec &w, int64_t lr, int64_t nloc, int64_t r0,
                                          int64_t &lo, int64_t &hi) {
    if (w.mode == 0) {
        lo = w.c0;
        hi = w.c1;
        return;
    }
    int64_t b0, len;
    block_of(lr, nloc, w.nblocks, w.bstart, b0, len);
    lo = r0 + b0;
    hi = r0 + b0 + len;
}

__global__ __launch_bounds__(TPB) void k_extract_count(const int64_t *rp, const int32_t *ci, int64_t r0,
                                                       int64_t r1, WindowSpec w, int64_t *len) {
    const int64_t nloc = r1 - r0;
    const int64_t lr = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (lr > nloc) return;
    if (lr == nloc) { len[nloc] = 0; return; }
    const int64_t r = r0 + lr;
    int64_t lo, hi;
    window_of(w, lr, nloc, r0, lo, hi);
    const int64_t a = lower_bound_i32(ci, rp[r], rp[r + 1], lo);
    const int64_t b = lower_bound_i32(ci, a, rp[r + 1], hi);
    len[lr] = b - a;
}

__global__ __launch_bounds__(TPB) void k_extract_fill(const int64_t *rp, const int32_t *ci, const double *val,
                                                      int64_t r0, int64_t r1, WindowSpec w, int64_t cshift,
                                                      const int64_t *orp, int32_t *oci, double *oval) {
    const int64_t nloc = r1 - r0;
    // one wave per row: contiguous copy
    const int64_t lr = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (lr >= nloc) return;
    const int64_t r = r0 + lr;
    int64_t lo, hi;
    window_of(w, lr, nloc, r0, lo, hi);
    const int64_t a = lower_bound_i32(ci, rp[r], rp[r + 1], lo);
    const int64_t dst = orp[lr];
    const int64_t cnt = orp[lr + 1] - dst;
    for (int64_t k = lane; k < cnt; k += 64) {
        oci[dst + k] = (int32_t)((int64_t)ci[a + k] - cshift);
        oval[dst + k] = val[a + k];
    }
}

void launch_extract_count(const int64_t *rp, const int32_t *ci, int64_t r0, int64_t r1, WindowSpec w,
                          int64_t *row_len, hipStream_t st) {
    k_extract_count<<<grid_for(r1 - r0 + 1, TPB), TPB, 0, st>>>(rp, ci, r0, r1, w, row_len);
}
void launch_extract_fill(const int64_t *rp, const int32_t *ci, const double *val, int64_t r0, int64_t r1,
                         WindowSpec w, int64_t cshift, const int64_t *out_rp, int32_t *out_ci,
                         double *out_val, hipStream_t st) {
    k_extract_fill<<<grid_for((r1 - r0) * 64, TPB), TPB, 0, st>>>(rp, ci, val, r0, r1, w, cshift, out_rp,
                                                                  out_ci, out_val);
}

// ================================================================= SpMV ====
// y = alpha * (M x) + beta * z.  LPR lanes per row; 256 / LPR rows per block.
template <int LPR>
__global__ __launch_bounds__(TPB) void k_spmv(int64_t nrows, const int64_t *__restrict__ rp,
                                              const int32_t *__restrict__ ci, const double *__restrict__ val,
                                              const double *__restrict__ x, double *__restrict__ y,
                                              double alpha, double beta, const double *__restrict__ z) {
    const int sub = threadIdx.x & (LPR - 1);
    const int64_t row = ((int64_t)blockIdx.x * TPB + threadIdx.x) / LPR;
    if (row >= nrows) return;
    const int64_t s = rp[row], e = rp[row + 1];
    double acc = row_dot<LPR, 4, true>(s, e, sub, ci, val, x);
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (sub == 0) {
        double r = alpha * acc;
        if (beta != 0.0) r += beta * z[row];
        y[row] = r;
    }
}

// Long rows (mean >= 96 nnz): one wave walks `rpw` consecutive rows two at a
// time; for each row pair all U*64 val/col loads per row are issued before the
// x gathers, so a wave keeps ~4.6 KB of HBM loads in flight (the one-row-per-
// wave form is latency bound at ~2 TB/s).
template <int U>
__global__ __launch_bounds__(TPB) void k_spmv_w64(int64_t nrows, int rpw, const int64_t *__restrict__ rp,
                                                  const int32_t *__restrict__ ci, const double *__restrict__ val,
                                                  const double *__restrict__ x, double *__restrict__ y,
                                                  double alpha, double beta, const double *__restrict__ z) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (TPB / 64) + (threadIdx.x >> 6)));
    const int64_t r0 = (int64_t)wave * rpw;
    if (r0 >= nrows) return;
    const int64_t r1 = (r0 + rpw < nrows) ? r0 + rpw : nrows;
    for (int64_t r = r0; r < r1; r += 2) {
        const bool two = (r + 1 < r1);
        const int64_t sa = rp[r], ea = rp[r + 1];
        const int64_t eb = two ? rp[r + 2] : ea;
        double acc_a = 0.0, acc_b = 0.0;
        for (int64_t ka = sa, kb = ea; ka < ea || kb < eb; ka += U * 64, kb += U * 64) {
            int32_t ca[U], cb[U];
            double va[U], vb[U];
// unconditional loads at a clamped index (entry 0 is always valid), value
            // masked to 0: no exec-masked branch, so all 4U loads issue back to back
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t k = ka + u * 64 + lane;
                const int64_t kk = k < ea ? k : 0;
                ca[u] = __builtin_nontemporal_load(ci + kk);
                const double v = __builtin_nontemporal_load(val + kk);
                va[u] = k < ea ? v : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t k = kb + u * 64 + lane;
                const int64_t kk = k < eb ? k : 0;
                cb[u] = __builtin_nontemporal_load(ci + kk);
                const double v = __builtin_nontemporal_load(val + kk);
                vb[u] = k < eb ? v : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                acc_a += va[u] * x[(uint32_t)ca[u]];
                acc_b += vb[u] * x[(uint32_t)cb[u]];
            }
        }
        acc_a = wave_reduce(acc_a);
        acc_b = wave_reduce(acc_b);
        if (lane == 0) {
            double ra = alpha * acc_a;
            if (beta != 0.0) ra += beta * z[r];
            y[r] = ra;
            if (two) {
                double rb = alpha * acc_b;
                if (beta != 0.0) rb += beta * z[r + 1];
                y[r + 1] = rb;
            }
        }
    }
}

// Few, very long rows (AMG restriction R = P^T, Galerkin coarse operators,
// the dense coarsest inverse): one 256-lane workgroup per row, U loads per
// lane in flight, fixed-order wave + LDS reduction (deterministic).
template <int U>
__global__ __launch_bounds__(TPB) void k_spmv_wg(int64_t nrows, const int64_t *__restrict__ rp,
                                                 const int32_t *__restrict__ ci, const double *__restrict__ val,
                                                 const double *__restrict__ x, double *__restrict__ y, double alpha,
                                                 double beta, const double *__restrict__ z) {
    __shared__ double part[TPB / 64];
    const int64_t row = blockIdx.x;
    const int64_t s = rp[row], e = rp[row + 1];
    double acc = 0.0;
    for (int64_t k0 = s; k0 < e; k0 += U * TPB) {
        int32_t c[U];
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t k = k0 + u * TPB + threadIdx.x;
            const int64_t kk = k < e ? k : s;
            c[u] = __builtin_nontemporal_load(ci + kk);
            const double vv = __builtin_nontemporal_load(val + kk);
            v[u] = k < e ? vv : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc += v[u] * x[(uint32_t)c[u]];
    }
    acc = wave_reduce(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = part[0];
#pragma unroll
        for (int w = 1; w < TPB / 64; ++w) t += part[w];
        double r = alpha * t;
        if (beta != 0.0) r += beta * z[row];
        y[row] = r;
    }
}

void launch_spmv(int64_t nrows, int64_t nnz, const int64_t *rp, const int32_t *ci, const double *val,
                 const double *x, double *y, double alpha, double beta, const double *z, hipStream_t st) {
    if (nrows <= 0) return;
    const double mean = (double)nnz / (double)nrows;
    if (mean >= 512.0 || (mean >= 96.0 && nrows < 16384)) {
        k_spmv_wg<4><<<(unsigned)nrows, TPB, 0, st>>>(nrows, rp, ci, val, x, y, alpha, beta, z);
    } else if (mean >= 96.0) {
        const int rpw = 8;
        const int64_t waves = (nrows + rpw - 1) / rpw;
        k_spmv_w64<3><<<grid_for(waves, TPB / 64), TPB, 0, st>>>(nrows, rpw, rp, ci, val, x, y, alpha, beta, z);
    } else if (mean >= 40.0)
        k_spmv<32><<<grid_for(nrows, TPB / 32), TPB, 0, st>>>(nrows, rp, ci, val, x, y, alpha, beta, z);
    else if (mean >= 16.0)
        k_spmv<16><<<grid_for(nrows, TPB / 16), TPB, 0, st>>>(nrows, rp, ci, val, x, y, alpha, beta, z);
    else
        k_spmv<8><<<grid_for(nrows, TPB / 8), TPB, 0, st>>>(nrows, rp, ci, val, x, y, alpha, beta, z);
}

// =============================================================== BLAS-1 ====
__global__ __launch_bounds__(TPB) void k_copy(int64_t n, const double *x, double *y) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) y[i] = x[i];
}
__global__ __launch_bounds__(TPB) void k_set(int64_t n, double a, double *y) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) y[i] = a;
}
__global__ __launch_bounds__(TPB) void k_scale(int64_t n, double a, double *y) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) y[i] *= a;
}
// (pa / pb: the scalars read from device memory instead, skip: no-op when *skip
// -- the device-resident CG; one kernel body, so both paths round alike)
__global__ __launch_bounds__(TPB) void k_axpby(int64_t n, double a, const double *x, double b, double *y,
                                               const double *pa, const double *pb, const int64_t *skip) {
    if (skip && *skip) return;
    if (pa) a = *pa;
    if (pb) b = *pb;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB)
        y[i] = a * x[i] + b * y[i];
}
__global__ __launch_bounds__(TPB) void k_waxpby(int64_t n, double a, const double *x, double b,
                                                const double *y, double *w) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB)
        w[i] = a * x[i] + b * y[i];
}
__global__ __launch_bounds__(TPB) void k_pmult(int64_t n, const double *x, const double *d, double *y) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB)
        y[i] = x[i] * d[i];
}
__global__ __launch_bounds__(TPB) void k_zero_entries(int64_t m, const int32_t *idx, double *y) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i < m) y[idx[i]] = 0.0;
}
__global__ __launch_bounds__(TPB) void k_gather(int64_t n, const int64_t *idx, const double *x, double *y) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB)
        y[i] = x[idx[i]];
}
__global__ __launch_bounds__(TPB) void k_scatter(int64_t n, const int64_t *idx, const double *x, double *y) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB)
        y[idx[i]] = x[i];
}

// AMG Chebyshev/Jacobi step (oracle/amg.py PCAMG._cheb), fused:
// d = a d + bc (dinv . r), x += d;  flags 1: d not read (d = bc (dinv . r)),
// flags 2: x not read (x = d)
__global__ __launch_bounds__(TPB) void k_cheb_step(int64_t n, const double *__restrict__ dinv,
                                                   const double *__restrict__ r, double *__restrict__ d,
                                                   double *__restrict__ x, double a, double bc, int flags) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const double t = dinv[i] * r[i];
        const double dn = (flags & 1) ? bc * t : a * d[i] + bc * t;
        d[i] = dn;
        x[i] = (flags & 2) ? dn : x[i] + dn;
    }
}

// BoomerAMG's Jacobi-type / Chebyshev smoothing step after the row's residual (kernels.hpp
// RELAX_*): dn = a dold + g (m res), the two products rounded, the a dold term one fma or
// absent.  The fused launch (k_d16_spmv, D16_AUX_RELAX) and k_relax_step share it, so both
// give the same bits whatever the compiler contracts elsewhere.
__device__ __forceinline__ double relax_dn(double res, double m, double g, double a, double dold, bool read_d) {
    const double u = __dmul_rn(g, __dmul_rn(m, res));
    return read_d ? fma(a, dold, u) : u;
}
__global__ __launch_bounds__(TPB) void k_relax_step(int64_t n, const double *__restrict__ res, const double *x,
                                                    double *x_new, const double *__restrict__ m, double *d,
                                                    double a, double g, int flags) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const bool rd = flags & RELAX_READ_D;
        const double dn = relax_dn(res[i], m[i], g, a, rd ? d[i] : 0.0, rd);
        if (flags & RELAX_WRITE_D) d[i] = dn;
        x_new[i] = (flags & RELAX_X_ZERO) ? dn : __dadd_rn(x[i], dn);
    }
}

// Polynomial KSP update (richardson, chebyshev; ksp.cpp): out = a pm1 + b pk + c t with
// t = dinv . z (the Jacobi PC fused in) or t = z.  A null pm1 / pk term is omitted, not
// multiplied by zero; out may alias pm1 or pk (every entry is read before it is written,
// by the thread that writes it).  One body for the first step (c t), Richardson's
// x += scale z and the three-term step: t is a rounded product, then one fma per term.
__global__ __launch_bounds__(TPB) void k_poly_update(int64_t n, double a, const double *pm1, double b,
                                                     const double *pk, double c, const double *dinv,
                                                     const double *z, double *out) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const double t = dinv ? dinv[i] * z[i] : z[i];
        double v = c * t;
        if (pk) v = fma(b, pk[i], v);
        if (pm1) v = fma(a, pm1[i], v);
        out[i] = v;
    }
}

static inline unsigned stream_grid(int64_t n) {
    int64_t g = (n + TPB - 1) / TPB;
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// streaming probes (the achievable HBM rate): 16 B per lane,
// four loads in flight per lane, nontemporal.  mode 0: copy (read + write),
// mode 1: read-only (the SpMV's traffic mix is ~99 % reads)
typedef double probe_d2 __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(TPB) void k_copy_probe(int64_t n2, const probe_d2 *__restrict__ x,
                                                    probe_d2 *__restrict__ y, int mode, double *sink) {
    const int64_t stride = (int64_t)gridDim.x * TPB;
    probe_d2 acc = {0.0, 0.0};
    for (int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x; i0 < n2; i0 += 4 * stride) {
        probe_d2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = i0 + u * stride;
            v[u] = i < n2 ? __builtin_nontemporal_load(x + i) : probe_d2{0.0, 0.0};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = i0 + u * stride;
            if (mode == 0) {
                if (i < n2) __builtin_nontemporal_store(v[u], y + i);
            } else {
                acc += v[u];
            }
        }
    }
    if (mode == 1 && acc.x + acc.y == 12345.678) sink[0] = acc.x;
}
void launch_copy_probe(int64_t n, const double *x, double *y, int mode, hipStream_t st) {
    if (n > 1)
        k_copy_probe<<<8192, TPB, 0, st>>>(n / 2, reinterpret_cast<const probe_d2 *>(x), reinterpret_cast<probe_d2 *>(y),
                                            mode, y);
}
void launch_copy(int64_t n, const double *x, double *y, hipStream_t st) {
    if (n > 0) k_copy<<<stream_grid(n), TPB, 0, st>>>(n, x, y);
}
void launch_set(int64_t n, double a, double *y, hipStream_t st) {
    if (n > 0) k_set<<<stream_grid(n), TPB, 0, st>>>(n, a, y);
}
void launch_scale(int64_t n, double a, double *y, hipStream_t st) {
    if (n > 0) k_scale<<<stream_grid(n), TPB, 0, st>>>(n, a, y);
}
void launch_axpby(int64_t n, double a, const double *x, double b, double *y, hipStream_t st) {
    if (n > 0) k_axpby<<<stream_grid(n), TPB, 0, st>>>(n, a, x, b, y, nullptr, nullptr, nullptr);
}
void launch_axpby_dev(int64_t n, const double *pa, const double *x, const double *pb, double *y, const int64_t *skip,
                      hipStream_t st) {
    if (n > 0) k_axpby<<<stream_grid(n), TPB, 0, st>>>(n, 0.0, x, 0.0, y, pa, pb, skip);
}

// ------------------------------------------------ device-resident CG state --
// KSPSolve_CG's scalar recurrences (runtime.cpp KSP::solve_cg) on the device,
// one thread, so the host enqueues iterations without reading a scalar back:
// every phase returns at once when the solve has ended (I[CG_DONE]); the
// vector updates that follow check the same flag.  Same operations as the host
// loop (IEEE division and square root): bitwise the same iterates.
__device__ int cg_conv(const CgParams &p, double r, double rnorm0, double ttol) {
    if (isnan(r) || isinf(r)) return p.r_nan;
    if (r <= ttol) return r < p.atol ? p.r_atol : p.r_rtol;
    if (r >= p.dtol * rnorm0) return p.r_dtol;
    return 0;
}
__global__ void k_cg_state(int phase, int64_t i, double *S, int64_t *I, double *hist, CgParams p) {
    if (threadIdx.x != 0 || I[CG_DONE]) return;
    auto stop = [&](int reason) {
        I[CG_REASON] = reason;
        I[CG_DONE] = 1;
    };
    switch (phase) {
        case CG_TOP: {  // loop head of iteration i (beta = (z, r) of the previous step)
            I[CG_ITS] = i + 1;
            const double beta = S[CG_BETA], betaold = S[CG_BETAOLD];
            if (beta == 0.0) return stop(p.r_atol);
            if (i > 0 && beta * betaold < 0.0) return stop(p.r_indef_pc);
            if (i > 0) S[CG_BB] = beta / betaold;
            return;
        }
        case CG_MID: {  // dpi = (p, A p) in S[CG_SLOT]
            const double dpiold = S[CG_DPI], dpi = S[CG_SLOT];
            S[CG_DPI] = dpi;
            S[CG_BETAOLD] = S[CG_BETA];
            const int sd = (dpi > 0) - (dpi < 0), so = (dpiold > 0) - (dpiold < 0);
            if (dpi == 0.0 || (i > 0 && sd * so < 0)) return stop(p.r_indef_mat);
            const double a = S[CG_BETA] / dpi;
            S[CG_A] = a;
            S[CG_NEGA] = -a;
            return;
        }
        case CG_POST: {  // the residual norm's square (or 0) in S[CG_SLOT]
            const double dp = p.norm ? sqrt(S[CG_SLOT]) : 0.0;
            S[CG_RNORM] = dp;
            hist[I[CG_HCOUNT]++] = dp;
            if (p.norm) {
                const int r = cg_conv(p, dp, S[CG_RNORM0], S[CG_TTOL]);
                if (r) return stop(r);
            }
            return;
        }
        case CG_END: {  // beta = (z, r) in S[CG_SLOT2]; i counts this iteration
            S[CG_BETA] = S[CG_SLOT2];
            if (i + 1 >= p.maxit) return stop(p.r_its);
            return;
        }
    }
}
void launch_cg_state(int phase, int64_t i, double *S, int64_t *I, double *hist, const CgParams &p, hipStream_t st) {
    k_cg_state<<<1, 64, 0, st>>>(phase, i, S, I, hist, p);
}
void launch_waxpby(int64_t n, double a, const double *x, double b, const double *y, double *w, hipStream_t st) {
    if (n > 0) k_waxpby<<<stream_grid(n), TPB, 0, st>>>(n, a, x, b, y, w);
}
void launch_pointwise_mult(int64_t n, const double *x, const double *d, double *y, hipStream_t st) {
    if (n > 0) k_pmult<<<stream_grid(n), TPB, 0, st>>>(n, x, d, y);
}
void launch_cheb_step(int64_t n, const double *dinv, const double *r, double *d, double *x, double a, double bc,
                      int flags, hipStream_t st) {
    if (n > 0) k_cheb_step<<<stream_grid(n), TPB, 0, st>>>(n, dinv, r, d, x, a, bc, flags);
}
void launch_relax_step(int64_t n, const double *res, const double *x, double *x_new, const double *m, double *d,
                       double a, double g, int flags, hipStream_t st) {
    if (n > 0) k_relax_step<<<stream_grid(n), TPB, 0, st>>>(n, res, x, x_new, m, d, a, g, flags);
}
void launch_poly_update(int64_t n, double a, const double *pm1, double b, const double *pk, double c,
                        const double *dinv, const double *z, double *out, hipStream_t st) {
    if (n > 0) k_poly_update<<<stream_grid(n), TPB, 0, st>>>(n, a, pm1, b, pk, c, dinv, z, out);
}
void launch_zero_entries(int64_t m, const int32_t *idx, double *y, hipStream_t st) {
    if (m > 0) k_zero_entries<<<grid_for(m, TPB), TPB, 0, st>>>(m, idx, y);
}
void launch_gather(int64_t n, const int64_t *idx, const double *x, double *y, hipStream_t st) {
    if (n > 0) k_gather<<<stream_grid(n), TPB, 0, st>>>(n, idx, x, y);
}
void launch_scatter(int64_t n, const int64_t *idx, const double *x, double *y, hipStream_t st) {
    if (n > 0) k_scatter<<<stream_grid(n), TPB, 0, st>>>(n, idx, x, y);
}

// ---------------------------------------------- deterministic reductions --
// up to 4096 blocks (16 waves per CU): with 1024 the multi-vector CGS
// kernels (k_mdot / k_maxpy_norm) held 4 waves per CU and read the Krylov
// basis at ~2.8 TB/s (profiles/r04_hyp59)
static constexpr int NB_MAX = 4096;
int reduce_blocks(int64_t n) {
    int64_t nb = (n + 4095) / 4096;
    if (nb < 1) nb = 1;
    if (nb > NB_MAX) nb = NB_MAX;
    return (int)nb;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// fixed-order block reduction (TPB threads); result valid in thread 0
__device__ __forceinline__ double block_sum(double v, double *lds) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < TPB / 64; ++i) r += lds[i];
    }
    __syncthreads();
    return r;
}

__device__ __forceinline__ void chunk_of(int64_t n, int nb, int b, int64_t &s, int64_t &e) {
    const int64_t c = (n + nb - 1) / nb;
    s = (int64_t)b * c;
    e = s + c;
    if (e > n) e = n;
    if (s > n) s = n;
}

// final pass: out[j] = sum_b partial[j*nb + b]
__global__ __launch_bounds__(TPB) void k_final(int nb, const double *partial, double *out, int sqrt_it) {
    __shared__ double lds[TPB / 64];
    const int j = blockIdx.x;
    double v = 0.0;
    for (int b = threadIdx.x; b < nb; b += TPB) v += partial[(int64_t)j * nb + b];
    v = block_sum(v, lds);
    if (threadIdx.x == 0) out[j] = sqrt_it ? sqrt(v) : v;
}

// ----------------------------------------------------- Krylov basis kernels --
// k_mdot / k_maxpy_norm / k_mgs_step / k_lincomb over a Krylov basis stored as T: double, or
// float (compressed-basis GMRES, pls_gmres_basis single: the columns are read as floats and
// promoted, w and every sum stay fp64).  One data path: 16-B loads of a column -- R rows per
// lane, 2 of a double basis and 4 of a float one, with R / 2 loads for the matching rows of
// w -- chunks that start on multiples of R rows (columns are 512-B aligned), two trips of
// loads issued ahead of their FMAs, each lane summing its rows in ascending order (first trip
// before second), the n mod R tail rows of the last chunk in thread 0 after its vector rows.
typedef double cgs_d2 __attribute__((ext_vector_type(2)));
typedef float cb_f4 __attribute__((ext_vector_type(4)));
template <class T>
struct basis_load;  // one 16-B load of a basis column
template <>
struct basis_load<double> {
    static constexpr int R = 2;
    typedef cgs_d2 vec;
};
template <>
struct basis_load<float> {
    static constexpr int R = 4;
    typedef cb_f4 vec;
};
template <int R>
struct w_rows {  // the R rows of w (or of a sum) beside one basis load
    cgs_d2 p[R / 2];
};
template <int N>
__device__ __forceinline__ void chunk_rows(int64_t n, int nb, int b, int64_t &s, int64_t &e) {
    int64_t c = (n + nb - 1) / nb;
    c = (c + N - 1) & ~(int64_t)(N - 1);
    s = (int64_t)b * c;
    e = s + c;
    if (e > n) e = n;
    if (s > n) s = n;
}
__device__ __forceinline__ cgs_d2 cb_ld2(const double *p) { return *reinterpret_cast<const cgs_d2 *>(p); }
template <class T>
__device__ __forceinline__ typename basis_load<T>::vec basis_ld(const T *p) {
    return *reinterpret_cast<const typename basis_load<T>::vec *>(p);
}
template <int R>
__device__ __forceinline__ w_rows<R> w_ld(const double *p) {
    w_rows<R> t;
#pragma unroll
    for (int q = 0; q < R / 2; ++q) t.p[q] = cb_ld2(p + 2 * q);
    return t;
}
template <int R>
__device__ __forceinline__ void w_st(double *p, const w_rows<R> &t) {
#pragma unroll
    for (int q = 0; q < R / 2; ++q) *reinterpret_cast<cgs_d2 *>(p + 2 * q) = t.p[q];
}
// a += v . w over the R rows, ascending
template <class VEC, int R>
__device__ __forceinline__ void rows_dot(double &a, const VEC v, const w_rows<R> &w) {
#pragma unroll
    for (int r = 0; r < R; ++r) a += (double)v[r] * w.p[r >> 1][r & 1];
}
// t -= h v over the R rows
template <class VEC, int R>
__device__ __forceinline__ void rows_sub(w_rows<R> &t, double h, const VEC v) {
#pragma unroll
    for (int r = 0; r < R; ++r) t.p[r >> 1][r & 1] -= h * (double)v[r];
}
// a += t . t
template <int R>
__device__ __forceinline__ void rows_sq(double &a, const w_rows<R> &t) {
#pragma unroll
    for (int r = 0; r < R; ++r) a += t.p[r >> 1][r & 1] * t.p[r >> 1][r & 1];
}

// mdot: blockIdx.x = chunk, blockIdx.y = group of MDOT_NJ vectors
// CGS dot block h_j = V_j . w, j in [0, k): blocks of MDOT_NJ columns per
// grid row, one partial per (column, block) -> k_final in fixed order.
static constexpr int MDOT_NJ = 16;
template <class T>
__global__ __launch_bounds__(TPB) void k_mdot(int64_t n, int k, const T *__restrict__ V, int64_t ldv,
                                              const double *__restrict__ w, double *partial) {
    constexpr int R = basis_load<T>::R;
    __shared__ double lds[TPB / 64];
    const int nb = gridDim.x;
    int64_t s, e;
    chunk_rows<R>(n, nb, blockIdx.x, s, e);
    const int j0 = blockIdx.y * MDOT_NJ;
    const int nj = (k - j0) < MDOT_NJ ? (k - j0) : MDOT_NJ;
    double a[MDOT_NJ];
#pragma unroll
    for (int u = 0; u < MDOT_NJ; ++u) a[u] = 0.0;
    const T *v0 = V + (int64_t)j0 * ldv;
    int64_t i = s + R * threadIdx.x;
    // two loads per column and trip, all of them issued before the FMAs (twice the
    // bytes in flight; the same per-thread summation order as one load a trip)
    for (; i + R * TPB + R - 1 < e; i += 2 * R * TPB) {
        const w_rows<R> wa = w_ld<R>(w + i), wb = w_ld<R>(w + i + R * TPB);
        typename basis_load<T>::vec va[MDOT_NJ], vb[MDOT_NJ];
#pragma unroll
        for (int u = 0; u < MDOT_NJ; ++u) {
            if (u < nj) {
                va[u] = basis_ld(v0 + (int64_t)u * ldv + i);
                vb[u] = basis_ld(v0 + (int64_t)u * ldv + i + R * TPB);
            }
        }
#pragma unroll
        for (int u = 0; u < MDOT_NJ; ++u) {
            if (u < nj) {
                rows_dot(a[u], va[u], wa);
                rows_dot(a[u], vb[u], wb);
            }
        }
    }
    for (; i + R - 1 < e; i += R * TPB) {
        const w_rows<R> wi = w_ld<R>(w + i);
#pragma unroll
        for (int u = 0; u < MDOT_NJ; ++u)
            if (u < nj) rows_dot(a[u], basis_ld(v0 + (int64_t)u * ldv + i), wi);
    }
    if (threadIdx.x == 0) {
        for (int64_t l = e - ((e - s) & (R - 1)); l < e; ++l) {
#pragma unroll
            for (int u = 0; u < MDOT_NJ; ++u)
                if (u < nj) a[u] += (double)v0[(int64_t)u * ldv + l] * w[l];
        }
    }
#pragma unroll
    for (int u = 0; u < MDOT_NJ; ++u) {
        if (u < nj) {
            const double r = block_sum(a[u], lds);
            if (threadIdx.x == 0) partial[(int64_t)(j0 + u) * nb + blockIdx.x] = r;
        }
    }
}

template <class T>
static void mdot(int64_t n, int k, const T *V, int64_t ldv, const double *w, double *partial, double *out,
                 hipStream_t st) {
    if (k <= 0) return;
    const int nb = reduce_blocks(n);
    dim3 grid(nb, (k + MDOT_NJ - 1) / MDOT_NJ);
    k_mdot<T><<<grid, TPB, 0, st>>>(n, k, V, ldv, w, partial);
    k_final<<<k, TPB, 0, st>>>(nb, partial, out, 0);
}
void launch_mdot(int64_t n, int k, const double *V, int64_t ldv, const double *w, double *partial, double *out,
                 hipStream_t st) {
    mdot(n, k, V, ldv, w, partial, out, st);
}
void launch_mdot(int64_t n, int k, const float *V, int64_t ldv, const double *w, double *partial, double *out,
                 hipStream_t st) {
    mdot(n, k, V, ldv, w, partial, out, st);
}

__global__ __launch_bounds__(TPB) void k_dot(int64_t n, const double *__restrict__ x, const double *__restrict__ y,
                                             double *partial) {
    __shared__ double lds[TPB / 64];
    int64_t s, e;
    chunk_of(n, gridDim.x, blockIdx.x, s, e);
    double a = 0.0;
    for (int64_t i = s + threadIdx.x; i < e; i += TPB) a += x[i] * y[i];
    a = block_sum(a, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = a;
}

void launch_dot(int64_t n, const double *x, const double *y, double *partial, double *out, hipStream_t st) {
    const int nb = reduce_blocks(n);
    k_dot<<<nb, TPB, 0, st>>>(n, x, y, partial);
    k_final<<<1, TPB, 0, st>>>(nb, partial, out, 0);
}
void launch_norm2(int64_t n, const double *x, double *partial, double *out, hipStream_t st) {
    const int nb = reduce_blocks(n);
    k_dot<<<nb, TPB, 0, st>>>(n, x, x, partial);
    k_final<<<1, TPB, 0, st>>>(nb, partial, out, 1);
}

// ------------------------------------------------------------- BiCGStab --
// KSPSolve_BCGS (runtime.cpp KSP::solve_bcgs / solve_bcgs_dev).  Both drivers
// launch these kernels with their coefficients read from the state S on the
// device, so the iterates round alike whichever driver computed the scalars.
// Every vector kernel returns at once when *skip (the solve has ended).
//
// One thread runs the scalar recurrence; the sums it consumes are in
// S[BC_SLOT0..].  Same operations as the host driver (IEEE division and
// square root, no multiply-add pair a compiler could contract).
__device__ void bcgs_state(int phase, int64_t i, double *S, int64_t *I, double *hist, const BcgsParams &p) {
    if (I[CG_DONE]) return;
    auto stop = [&](int reason) {
        I[CG_REASON] = reason;
        I[CG_DONE] = 1;
    };
    switch (phase) {
        case BC_MID1: {  // d1 = (v, rp)
            const double d1 = S[BC_SLOT0];
            if (d1 == 0.0) return stop(p.r_breakdown);
            const double alpha = S[BC_RHO] / d1;
            S[BC_ALPHA] = alpha;
            S[BC_NEGALPHA] = -alpha;
            return;
        }
        case BC_MID2: {  // d1 = (s, t), d2 = (t, t)
            const double d1 = S[BC_SLOT0], d2 = S[BC_SLOT1];
            if (d2 == 0.0) return stop(p.r_pending);  // the host looks at (s, s)
            const double omega = d1 / d2;
            S[BC_OMEGA] = omega;
            S[BC_NEGOMEGA] = -omega;
            return;
        }
        case BC_POST: {  // (r, r) and the next rho = (r, rp); i counts this iteration
            const double dp = p.c.norm ? sqrt(S[BC_SLOT0]) : 0.0;
            const double rho = S[BC_RHO];
            S[BC_RHOOLD] = rho;
            S[BC_OMEGAOLD] = S[BC_OMEGA];
            S[BC_RHO] = S[BC_SLOT1];
            I[CG_ITS] = i + 1;
            hist[I[CG_HCOUNT]++] = dp;
            if (p.c.norm) {
                const int r = cg_conv(p.c, dp, S[BC_RNORM0], S[BC_TTOL]);
                if (r) return stop(r);
            }
            if (rho == 0.0) return stop(p.r_breakdown);
            if (i + 1 >= p.c.maxit) return stop(p.c.r_its);
            const double beta = (S[BC_RHO] / S[BC_RHOOLD]) * (S[BC_ALPHA] / S[BC_OMEGAOLD]);
            S[BC_BETA] = beta;
            S[BC_C1] = S[BC_OMEGAOLD] * beta;
            return;
        }
    }
}
__global__ void k_bcgs_state(int phase, int64_t i, double *S, int64_t *I, double *hist, BcgsParams p) {
    if (threadIdx.x == 0) bcgs_state(phase, i, S, I, hist, p);
}
void launch_bcgs_state(int phase, int64_t i, double *S, int64_t *I, double *hist, const BcgsParams &p,
                       hipStream_t st) {
    k_bcgs_state<<<1, 64, 0, st>>>(phase, i, S, I, hist, p);
}

// End of a reducing kernel, single launch: a[r] (valid in thread 0) is this
// block's part of row r.  Thread 0 stores the parts with agent-scope atomic
// stores (write-through), waits for them, and draws a ticket; the block that
// draws the last one re-reads every part with agent-scope atomic loads (past
// its L1) and sums them in k_final's order.  True (in every thread) in that
// block alone, with the totals valid in its thread 0; the caller consumes them
// and calls ticket_reset.  Nobody waits for anybody.  Shared by BiCGStab
// (bcgs_finish) and the MGS step of GMRES (k_mgs_step).
template <int NR>
__device__ __forceinline__ bool ticket_totals(const double (&a)[NR], double *partial, double *lds, unsigned *ticket,
                                              double (&tot)[NR]) {
    const int nb = gridDim.x;
    __shared__ int last;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int r = 0; r < NR; ++r)
            __hip_atomic_store(partial + (int64_t)r * nb + blockIdx.x, a[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = (t == (unsigned)(nb - 1));
    }
    __syncthreads();
    if (!last) return false;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nb; b += TPB)
            v += __hip_atomic_load(partial + (int64_t)r * nb + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tot[r] = block_sum(v, lds);
    }
    return true;
}
__device__ __forceinline__ void ticket_reset(unsigned *ticket) {
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// BiCGStab's end of a reducing kernel.  Without a ticket the parts go to
// partial[r * nb + block] for k_final.  With one (pls.bcgs_fused_reduce) the
// last block to arrive (ticket_totals) writes the sums into S[BC_SLOT0 + r]
// and runs the state phase that follows.
template <int NR>
__device__ __forceinline__ void bcgs_finish(const double (&a)[NR], double *partial, double *lds, const BcgsFuse &f) {
    const int nb = gridDim.x;
    if (!f.ticket) {
        if (threadIdx.x == 0) {
#pragma unroll
            for (int r = 0; r < NR; ++r) partial[(int64_t)r * nb + blockIdx.x] = a[r];
        }
        return;
    }
    double tot[NR];
    if (!ticket_totals<NR>(a, partial, lds, f.ticket, tot)) return;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int r = 0; r < NR; ++r) f.S[BC_SLOT0 + r] = tot[r];
        bcgs_state(f.phase, f.i, f.S, f.I, f.hist, f.p);
        ticket_reset(f.ticket);
    }
}

// p = r - c1 v + c2 p  (c1 = omegaold beta, c2 = beta)
__global__ __launch_bounds__(TPB) void k_bcgs_p(int64_t n, const double *__restrict__ r, const double *__restrict__ v,
                                                double *__restrict__ p, const double *S, const int64_t *skip) {
    if (*skip) return;
    const double c1 = S[BC_C1], c2 = S[BC_BETA];
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB)
        p[i] = (r[i] - c1 * v[i]) + c2 * p[i];
}
// w = a x + b y with a = *pa, b = *pb
__global__ __launch_bounds__(TPB) void k_waxpby_dev(int64_t n, const double *pa, const double *__restrict__ x,
                                                    const double *pb, const double *__restrict__ y,
                                                    double *__restrict__ w, const int64_t *skip) {
    if (*skip) return;
    const double a = *pa, b = *pb;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB)
        w[i] = a * x[i] + b * y[i];
}
// (x, y)
__global__ __launch_bounds__(TPB) void k_bcgs_dot(int64_t n, const double *__restrict__ x,
                                                  const double *__restrict__ y, double *partial, BcgsFuse f,
                                                  const int64_t *skip) {
    __shared__ double lds[TPB / 64];
    if (*skip) return;
    int64_t s, e;
    chunk_of(n, gridDim.x, blockIdx.x, s, e);
    double a[1] = {0.0};
    for (int64_t i = s + threadIdx.x; i < e; i += TPB) a[0] += x[i] * y[i];
    a[0] = block_sum(a[0], lds);
    bcgs_finish<1>(a, partial, lds, f);
}
// (s, t) and (t, t) in one pass
__global__ __launch_bounds__(TPB) void k_dot2(int64_t n, const double *__restrict__ sv, const double *__restrict__ tv,
                                              double *partial, BcgsFuse f, const int64_t *skip) {
    __shared__ double lds[TPB / 64];
    if (*skip) return;
    int64_t s, e;
    chunk_of(n, gridDim.x, blockIdx.x, s, e);
    double a[2] = {0.0, 0.0};
    for (int64_t i = s + threadIdx.x; i < e; i += TPB) {
        const double ti = tv[i];
        a[0] += sv[i] * ti;
        a[1] += ti * ti;
    }
    a[0] = block_sum(a[0], lds);
    a[1] = block_sum(a[1], lds);
    bcgs_finish<2>(a, partial, lds, f);
}
// x += alpha p + omega s, r = s - omega t; (r, r) and (r, rp)
__global__ __launch_bounds__(TPB) void k_bcgs_update(int64_t n, const double *__restrict__ p,
                                                     const double *__restrict__ sv, const double *__restrict__ tv,
                                                     const double *__restrict__ rp, double *__restrict__ x,
                                                     double *__restrict__ r, double *partial, BcgsFuse f,
                                                     const int64_t *skip) {
    __shared__ double lds[TPB / 64];
    if (*skip) return;
    const double alpha = f.S[BC_ALPHA], omega = f.S[BC_OMEGA];
    int64_t s, e;
    chunk_of(n, gridDim.x, blockIdx.x, s, e);
    double a[2] = {0.0, 0.0};
    for (int64_t i = s + threadIdx.x; i < e; i += TPB) {
        const double si = sv[i];
        x[i] = (x[i] + alpha * p[i]) + omega * si;
        const double rn = si - omega * tv[i];
        r[i] = rn;
        a[0] += rn * rn;
        a[1] += rn * rp[i];
    }
    a[0] = block_sum(a[0], lds);
    a[1] = block_sum(a[1], lds);
    bcgs_finish<2>(a, partial, lds, f);
}

void launch_bcgs_p(int64_t n, const double *r, const double *v, double *p, const double *S, const int64_t *skip,
                   hipStream_t st) {
    if (n > 0) k_bcgs_p<<<stream_grid(n), TPB, 0, st>>>(n, r, v, p, S, skip);
}
void launch_waxpby_dev(int64_t n, const double *pa, const double *x, const double *pb, const double *y, double *w,
                       const int64_t *skip, hipStream_t st) {
    if (n > 0) k_waxpby_dev<<<stream_grid(n), TPB, 0, st>>>(n, pa, x, pb, y, w, skip);
}
void launch_bcgs_dot(int64_t n, const double *x, const double *y, double *partial, const BcgsFuse &f,
                     const int64_t *skip, hipStream_t st) {
    k_bcgs_dot<<<reduce_blocks(n), TPB, 0, st>>>(n, x, y, partial, f, skip);
}
void launch_dot2(int64_t n, const double *s, const double *t, double *partial, const BcgsFuse &f, const int64_t *skip,
                 hipStream_t st) {
    k_dot2<<<reduce_blocks(n), TPB, 0, st>>>(n, s, t, partial, f, skip);
}
void launch_bcgs_update(int64_t n, const double *p, const double *s, const double *t, const double *rp, double *x,
                        double *r, double *partial, const BcgsFuse &f, const int64_t *skip, hipStream_t st) {
    k_bcgs_update<<<reduce_blocks(n), TPB, 0, st>>>(n, p, s, t, rp, x, r, partial, f, skip);
}
// out[j] = sum_b partial[j * nb + b], j < rows (the separate final pass of the kernels above)
void launch_final(int64_t n, int rows, const double *partial, double *out, hipStream_t st) {
    k_final<<<rows, TPB, 0, st>>>(reduce_blocks(n), partial, out, 0);
}

// w -= sum_j h[j] V[:, j] (j ascending, as VecMAXPY); partial ||w||^2.
// Eight basis columns loaded ahead of their FMAs so every lane keeps 8-9 loads in flight.
template <class T>
__global__ __launch_bounds__(TPB) void k_maxpy_norm(int64_t n, int k, const T *__restrict__ V, int64_t ldv,
                                                    const double *__restrict__ h, double *__restrict__ w,
                                                    double *partial) {
    constexpr int R = basis_load<T>::R;
    typedef typename basis_load<T>::vec vec;
    __shared__ double lds[TPB / 64];
    __shared__ double hs[512];
    for (int j = threadIdx.x; j < k && j < 512; j += TPB) hs[j] = h[j];
    __syncthreads();
    int64_t s, e;
    chunk_rows<R>(n, gridDim.x, blockIdx.x, s, e);
    double a = 0.0;
    int64_t i = s + R * threadIdx.x;
    // two loads per column and trip (both ahead of their FMAs; the norm sums
    // the rows in the same order as one load a trip)
    for (; i + R * TPB + R - 1 < e; i += 2 * R * TPB) {
        w_rows<R> ta = w_ld<R>(w + i), tb = w_ld<R>(w + i + R * TPB);
        int j = 0;
        for (; j + 8 <= k; j += 8) {
            vec va[8], vb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                va[u] = basis_ld(V + (int64_t)(j + u) * ldv + i);
                vb[u] = basis_ld(V + (int64_t)(j + u) * ldv + i + R * TPB);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const double hj = (j + u) < 512 ? hs[j + u] : h[j + u];
                rows_sub(ta, hj, va[u]);
                rows_sub(tb, hj, vb[u]);
            }
        }
        for (; j < k; ++j) {
            const vec va = basis_ld(V + (int64_t)j * ldv + i);
            const vec vb = basis_ld(V + (int64_t)j * ldv + i + R * TPB);
            const double hj = j < 512 ? hs[j] : h[j];
            rows_sub(ta, hj, va);
            rows_sub(tb, hj, vb);
        }
        w_st<R>(w + i, ta);
        w_st<R>(w + i + R * TPB, tb);
        rows_sq(a, ta);
        rows_sq(a, tb);
    }
    for (; i + R - 1 < e; i += R * TPB) {
        w_rows<R> t = w_ld<R>(w + i);
        int j = 0;
        for (; j + 8 <= k; j += 8) {
            vec v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = basis_ld(V + (int64_t)(j + u) * ldv + i);
#pragma unroll
            for (int u = 0; u < 8; ++u) rows_sub(t, (j + u) < 512 ? hs[j + u] : h[j + u], v[u]);
        }
        for (; j < k; ++j) rows_sub(t, j < 512 ? hs[j] : h[j], basis_ld(V + (int64_t)j * ldv + i));
        w_st<R>(w + i, t);
        rows_sq(a, t);
    }
    if (threadIdx.x == 0) {
        for (int64_t l = e - ((e - s) & (R - 1)); l < e; ++l) {
            double t = w[l];
            for (int j = 0; j < k; ++j) t -= (j < 512 ? hs[j] : h[j]) * (double)V[(int64_t)j * ldv + l];
            w[l] = t;
            a += t * t;
        }
    }
    if (partial) {
        a = block_sum(a, lds);
        if (threadIdx.x == 0) partial[blockIdx.x] = a;
    }
}

template <class T>
static void maxpy_norm(int64_t n, int k, const T *V, int64_t ldv, const double *h_dev, double *w, double *partial,
                       double *out, hipStream_t st) {
    const int nb = reduce_blocks(n);
    k_maxpy_norm<T><<<nb, TPB, 0, st>>>(n, k, V, ldv, h_dev, w, out ? partial : nullptr);
    if (out) k_final<<<1, TPB, 0, st>>>(nb, partial, out, 0);  // ||w||^2 (rank-local)
}
void launch_maxpy_norm(int64_t n, int k, const double *V, int64_t ldv, const double *h_dev, double *w,
                       double *partial, double *out, hipStream_t st) {
    maxpy_norm(n, k, V, ldv, h_dev, w, partial, out, st);
}
void launch_maxpy_norm(int64_t n, int k, const float *V, int64_t ldv, const double *h_dev, double *w, double *partial,
                       double *out, hipStream_t st) {
    maxpy_norm(n, k, V, ldv, h_dev, w, partial, out, st);
}

// One step of modified Gram-Schmidt (KSPGMRESModifiedGramSchmidtOrthogonalization):
// w -= (*hprev) vprev first (vprev != null), then this block's part of (w, vj)
// over the updated rows -- (w, w) when vj is null.  k_mdot's data path.  Every
// row is read and written by one thread of one block, so no block depends on
// another's rows.  Without a ticket the parts go to partial[block] for k_final.
// With one (double basis only) the last block to arrive sums them
// (ticket_totals, in k_final's order) into *out, where the next step's launch
// reads its coefficient.
template <class T>
__global__ __launch_bounds__(TPB) void k_mgs_step(int64_t n, const T *__restrict__ vprev,
                                                  const double *__restrict__ hprev, const T *__restrict__ vj,
                                                  double *w, double *partial, double *out, unsigned *ticket) {
    constexpr int R = basis_load<T>::R;
    typedef typename basis_load<T>::vec vec;
    __shared__ double lds[TPB / 64];
    int64_t s, e;
    chunk_rows<R>(n, gridDim.x, blockIdx.x, s, e);
    const double hp = vprev ? *hprev : 0.0;
    double a[1] = {0.0};
    // the R rows at i: the update by vprev, then their part of (w, vj) or (w, w)
    auto rows = [&](int64_t i, w_rows<R> t, const vec p, const vec v) {
        if (vprev) {
            rows_sub(t, hp, p);
            w_st<R>(w + i, t);
        }
        if (vj) rows_dot(a[0], v, t);
        else rows_sq(a[0], t);
    };
    const vec zero = {};
    int64_t i = s + R * threadIdx.x;
    for (; i + R * TPB + R - 1 < e; i += 2 * R * TPB) {
        const w_rows<R> ta = w_ld<R>(w + i), tb = w_ld<R>(w + i + R * TPB);
        vec pa = zero, pb = zero, va = zero, vb = zero;
        if (vprev) {
            pa = basis_ld(vprev + i);
            pb = basis_ld(vprev + i + R * TPB);
        }
        if (vj) {
            va = basis_ld(vj + i);
            vb = basis_ld(vj + i + R * TPB);
        }
        rows(i, ta, pa, va);
        rows(i + R * TPB, tb, pb, vb);
    }
    for (; i + R - 1 < e; i += R * TPB)
        rows(i, w_ld<R>(w + i), vprev ? basis_ld(vprev + i) : zero, vj ? basis_ld(vj + i) : zero);
    if (threadIdx.x == 0) {
        for (int64_t l = e - ((e - s) & (R - 1)); l < e; ++l) {
            double t = w[l];
            if (vprev) {
                t -= hp * (double)vprev[l];
                w[l] = t;
            }
            a[0] += (vj ? (double)vj[l] : t) * t;
        }
    }
    a[0] = block_sum(a[0], lds);
    if constexpr (std::is_same<T, double>::value) {
        if (ticket) {
            double tot[1];
            if (!ticket_totals<1>(a, partial, lds, ticket, tot)) return;
            if (threadIdx.x == 0) {
                *out = tot[0];
                ticket_reset(ticket);
            }
            return;
        }
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = a[0];
}
void launch_mgs_step(int64_t n, const double *vprev, const double *hprev, const double *vj, double *w, double *partial,
                     double *out, unsigned *ticket, hipStream_t st) {
    k_mgs_step<double><<<reduce_blocks(n), TPB, 0, st>>>(n, vprev, hprev, vj, w, partial, out, ticket);
}
void launch_mgs_step(int64_t n, const float *vprev, const double *hprev, const float *vj, double *w, double *partial,
                     double *out, unsigned *ticket, hipStream_t st) {
    k_mgs_step<float><<<reduce_blocks(n), TPB, 0, st>>>(n, vprev, hprev, vj, w, partial, out, ticket);
}

template <class T>
__global__ __launch_bounds__(TPB) void k_lincomb(int64_t n, int k, const T *__restrict__ V, int64_t ldv,
                                                 const double *__restrict__ c, double *__restrict__ y) {
    __shared__ double cs[512];
    for (int j = threadIdx.x; j < k && j < 512; j += TPB) cs[j] = c[j];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        double t = 0.0;
        for (int j = 0; j < k; ++j) t += (j < 512 ? cs[j] : c[j]) * (double)V[(int64_t)j * ldv + i];
        y[i] = t;
    }
}
void launch_lincomb(int64_t n, int k, const double *V, int64_t ldv, const double *c_dev, double *y,
                    hipStream_t st) {
    if (n > 0) k_lincomb<double><<<stream_grid(n), TPB, 0, st>>>(n, k, V, ldv, c_dev, y);
}
void launch_lincomb(int64_t n, int k, const float *V, int64_t ldv, const double *c_dev, double *y, hipStream_t st) {
    if (n > 0) k_lincomb<float><<<stream_grid(n), TPB, 0, st>>>(n, k, V, ldv, c_dev, y);
}

// ------------------------------------------- Fischer guess (KSPGuess, model 2) --
// The update of the projection space after a solve (KSP::guess_update): with y = A x and
// alpha = B^T y, xo = x - sum_j alpha_j X_j and yo = y - sum_j alpha_j B_j (j ascending, as
// VecMAXPY), written straight into slot m of X and B (xo, yo: column m, never a column
// read), and one partial ||yo||^2 per block for k_final.  k_maxpy_norm's data path: chunks
// on even rows, 16-B loads of row pairs, two pairs per trip, GU_NJ column pairs (X_j, B_j)
// loaded ahead of their FMAs (16 loads in flight per lane), the odd tail row in thread 0.
// m = 0 is a copy plus a norm.  x and y are 16-B aligned (the host checks x).  The second
// Gram-Schmidt pass runs in place, x = xo and y = yo (every row is read and written by one
// thread), so those four pointers carry no restrict.
static constexpr int GU_NJ = 4;
__global__ __launch_bounds__(TPB) void k_guess_update(int64_t n, int m, const double *__restrict__ X,
                                                      const double *__restrict__ B, int64_t ldv,
                                                      const double *__restrict__ alpha,
                                                      const double *x, const double *y, double *xo, double *yo,
                                                      double *partial) {
    __shared__ double lds[TPB / 64];
    __shared__ double as[GUESS_MAX];
    for (int j = threadIdx.x; j < m && j < GUESS_MAX; j += TPB) as[j] = alpha[j];
    __syncthreads();
    int64_t s, e;
    chunk_rows<2>(n, gridDim.x, blockIdx.x, s, e);
    double a = 0.0;
    int64_t i = s + 2 * threadIdx.x;
    for (; i + 2 * TPB + 1 < e; i += 4 * TPB) {
        cgs_d2 xa = *reinterpret_cast<const cgs_d2 *>(x + i);
        cgs_d2 xb = *reinterpret_cast<const cgs_d2 *>(x + i + 2 * TPB);
        cgs_d2 ya = *reinterpret_cast<const cgs_d2 *>(y + i);
        cgs_d2 yb = *reinterpret_cast<const cgs_d2 *>(y + i + 2 * TPB);
        int j = 0;
        for (; j + GU_NJ <= m; j += GU_NJ) {
            cgs_d2 pa[GU_NJ], pb[GU_NJ], qa[GU_NJ], qb[GU_NJ];
#pragma unroll
            for (int u = 0; u < GU_NJ; ++u) {
                pa[u] = *reinterpret_cast<const cgs_d2 *>(X + (int64_t)(j + u) * ldv + i);
                pb[u] = *reinterpret_cast<const cgs_d2 *>(X + (int64_t)(j + u) * ldv + i + 2 * TPB);
                qa[u] = *reinterpret_cast<const cgs_d2 *>(B + (int64_t)(j + u) * ldv + i);
                qb[u] = *reinterpret_cast<const cgs_d2 *>(B + (int64_t)(j + u) * ldv + i + 2 * TPB);
            }
#pragma unroll
            for (int u = 0; u < GU_NJ; ++u) {
                const double aj = as[j + u];
                xa.x -= aj * pa[u].x;
                xa.y -= aj * pa[u].y;
                xb.x -= aj * pb[u].x;
                xb.y -= aj * pb[u].y;
                ya.x -= aj * qa[u].x;
                ya.y -= aj * qa[u].y;
                yb.x -= aj * qb[u].x;
                yb.y -= aj * qb[u].y;
            }
        }
        for (; j < m; ++j) {
            const cgs_d2 pa = *reinterpret_cast<const cgs_d2 *>(X + (int64_t)j * ldv + i);
            const cgs_d2 pb = *reinterpret_cast<const cgs_d2 *>(X + (int64_t)j * ldv + i + 2 * TPB);
            const cgs_d2 qa = *reinterpret_cast<const cgs_d2 *>(B + (int64_t)j * ldv + i);
            const cgs_d2 qb = *reinterpret_cast<const cgs_d2 *>(B + (int64_t)j * ldv + i + 2 * TPB);
            const double aj = as[j];
            xa.x -= aj * pa.x;
            xa.y -= aj * pa.y;
            xb.x -= aj * pb.x;
            xb.y -= aj * pb.y;
            ya.x -= aj * qa.x;
            ya.y -= aj * qa.y;
            yb.x -= aj * qb.x;
            yb.y -= aj * qb.y;
        }
        *reinterpret_cast<cgs_d2 *>(xo + i) = xa;
        *reinterpret_cast<cgs_d2 *>(xo + i + 2 * TPB) = xb;
        *reinterpret_cast<cgs_d2 *>(yo + i) = ya;
        *reinterpret_cast<cgs_d2 *>(yo + i + 2 * TPB) = yb;
        a += ya.x * ya.x;
        a += ya.y * ya.y;
        a += yb.x * yb.x;
        a += yb.y * yb.y;
    }
    for (; i + 1 < e; i += 2 * TPB) {
        cgs_d2 xt = *reinterpret_cast<const cgs_d2 *>(x + i);
        cgs_d2 yt = *reinterpret_cast<const cgs_d2 *>(y + i);
        int j = 0;
        for (; j + GU_NJ <= m; j += GU_NJ) {
            cgs_d2 p[GU_NJ], q[GU_NJ];
#pragma unroll
            for (int u = 0; u < GU_NJ; ++u) {
                p[u] = *reinterpret_cast<const cgs_d2 *>(X + (int64_t)(j + u) * ldv + i);
                q[u] = *reinterpret_cast<const cgs_d2 *>(B + (int64_t)(j + u) * ldv + i);
            }
#pragma unroll
            for (int u = 0; u < GU_NJ; ++u) {
                const double aj = as[j + u];
                xt.x -= aj * p[u].x;
                xt.y -= aj * p[u].y;
                yt.x -= aj * q[u].x;
                yt.y -= aj * q[u].y;
            }
        }
        for (; j < m; ++j) {
            const cgs_d2 p = *reinterpret_cast<const cgs_d2 *>(X + (int64_t)j * ldv + i);
            const cgs_d2 q = *reinterpret_cast<const cgs_d2 *>(B + (int64_t)j * ldv + i);
            const double aj = as[j];
            xt.x -= aj * p.x;
            xt.y -= aj * p.y;
            yt.x -= aj * q.x;
            yt.y -= aj * q.y;
        }
        *reinterpret_cast<cgs_d2 *>(xo + i) = xt;
        *reinterpret_cast<cgs_d2 *>(yo + i) = yt;
        a += yt.x * yt.x;
        a += yt.y * yt.y;
    }
    if (((e - s) & 1) && threadIdx.x == 0) {
        const int64_t l = e - 1;
        double xt = x[l], yt = y[l];
        for (int j = 0; j < m; ++j) {
            xt -= as[j] * X[(int64_t)j * ldv + l];
            yt -= as[j] * B[(int64_t)j * ldv + l];
        }
        xo[l] = xt;
        yo[l] = yt;
        a += yt * yt;
    }
    a = block_sum(a, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = a;
}
void launch_guess_update(int64_t n, int m, double *X, double *B, int64_t ldv, const double *alpha_dev,
                         const double *x, const double *y, double *partial, double *out, hipStream_t st) {
    // (x == nullptr: in place, the column pair already in slot m)
    if (m < 0 || m >= GUESS_MAX) return;  // (never: the host keeps m < size <= GUESS_MAX)
    const int nb = reduce_blocks(n);
    if (!x) {
        x = X + (int64_t)m * ldv;
        y = B + (int64_t)m * ldv;
    }
    k_guess_update<<<nb, TPB, 0, st>>>(n, m, X, B, ldv, alpha_dev, x, y, X + (int64_t)m * ldv,
                                       B + (int64_t)m * ldv, partial);
    k_final<<<1, TPB, 0, st>>>(nb, partial, out, 0);  // ||yo||^2 (rank-local)
}

// the two new columns scaled by a = 1 / ||yo|| in one launch (u, v: 16-B aligned)
__global__ __launch_bounds__(TPB) void k_scale2(int64_t n, double a, double *__restrict__ u, double *__restrict__ v) {
    const int64_t np = n >> 1;
    for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < np; p += (int64_t)gridDim.x * TPB) {
        cgs_d2 s = *reinterpret_cast<const cgs_d2 *>(u + 2 * p);
        cgs_d2 t = *reinterpret_cast<const cgs_d2 *>(v + 2 * p);
        s.x *= a;
        s.y *= a;
        t.x *= a;
        t.y *= a;
        *reinterpret_cast<cgs_d2 *>(u + 2 * p) = s;
        *reinterpret_cast<cgs_d2 *>(v + 2 * p) = t;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        u[n - 1] *= a;
        v[n - 1] *= a;
    }
}
void launch_scale2(int64_t n, double a, double *u, double *v, hipStream_t st) {
    if (n > 0) k_scale2<<<stream_grid((n + 1) / 2), TPB, 0, st>>>(n, a, u, v);
}

// ------------------------------------------ compressed-basis GMRES (fp32 V) --
// The new basis vector: vf = fl32(a w) (round to nearest even) and vd = vf promoted, the
// vector the next operator / PC application reads, in one pass over w.  Four rows per lane
// (vf, vd and w 32-B aligned, n >= 0 rows; the n mod 4 tail rows one lane each).
__global__ __launch_bounds__(TPB) void k_scale_round(int64_t n, double a, const double *__restrict__ w,
                                                     float *__restrict__ vf, double *__restrict__ vd) {
    const int64_t nq = n >> 2, tid = (int64_t)blockIdx.x * TPB + threadIdx.x, stride = (int64_t)gridDim.x * TPB;
    for (int64_t q = tid; q < nq; q += stride) {
        const int64_t i = 4 * q;
        const cgs_d2 w0 = cb_ld2(w + i), w1 = cb_ld2(w + i + 2);
        const cb_f4 f = {(float)(w0.x * a), (float)(w0.y * a), (float)(w1.x * a), (float)(w1.y * a)};
        *reinterpret_cast<cb_f4 *>(vf + i) = f;
        *reinterpret_cast<cgs_d2 *>(vd + i) = cgs_d2{(double)f.x, (double)f.y};
        *reinterpret_cast<cgs_d2 *>(vd + i + 2) = cgs_d2{(double)f.z, (double)f.w};
    }
    const int64_t l = 4 * nq + tid;
    if (l < n) {
        const float f = (float)(w[l] * a);
        vf[l] = f;
        vd[l] = (double)f;
    }
}
void launch_scale_round(int64_t n, double a, const double *w, float *vf, double *vd, hipStream_t st) {
    if (n > 0) k_scale_round<<<stream_grid((n + 3) / 4), TPB, 0, st>>>(n, a, w, vf, vd);
}

// TSQR leaf / tree step for the Anderson least squares (numpy Householder QR
// in the reference, lib/AAR.py:102-105): workgroup b takes rows
// [b C, b C + C) of the m <= 16 columns cols[k] (rows >= n read as zero),
// factors that C x m panel in LDS by m Householder reflections (LAPACK dlarfg
// conventions: beta = -sign(alpha) ||x||, tau = (beta - alpha) / beta,
// v = x / (alpha - beta) below the diagonal) and writes its m x m R (zero
// below the diagonal) as rows [b m, b m + m) of a column-major matrix with
// leading dimension ldo.  Stacked R's are factored again by the same kernel
// until one R is left (a fixed tree: bitwise reproducible).  Each reflection
// is one block reduction of the m - j dots sum_{r>j} A[j][r] A[k][r] (fixed
// order: per-thread rows ascending, xor-shuffle tree, 4 waves in order).
constexpr int TSQR_C = 512;
template <int M>
__global__ __launch_bounds__(256) void k_tsqr(int64_t n, const double *const *cols, double *Rout, int64_t ldo) {
    constexpr int C = TSQR_C, RPT = C / 256;
    __shared__ double A[M * C];
    __shared__ double red[4][M];
    __shared__ double w[M];
    __shared__ double cf[3];  // tau, scal, beta
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * C;
#pragma unroll
    for (int k = 0; k < M; ++k) {
        const double *cp = cols[k];
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            const int r = tid + q * 256;
            const int64_t g = r0 + r;
            A[k * C + r] = g < n ? cp[g] : 0.0;
        }
    }
    __syncthreads();
    for (int j = 0; j < M; ++j) {
        double p[M];
#pragma unroll
        for (int k = 0; k < M; ++k) p[k] = 0.0;
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            const int r = tid + q * 256;
            if (r > j) {
                const double vj = A[j * C + r];
#pragma unroll
                for (int k = 0; k < M; ++k)
                    if (k >= j) p[k] += vj * A[k * C + r];
            }
        }
#pragma unroll
        for (int k = 0; k < M; ++k) {
            if (k < j) continue;
            double v = p[k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (lane == 0) red[wv][k] = v;
        }
        __syncthreads();
        if (tid < M) {
            const double sigma = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
            const double alpha = A[j * C + j];
            double tau = 0.0, scal = 0.0, beta = alpha;
            if (sigma != 0.0) {
                const double nrm = sqrt(alpha * alpha + sigma);
                beta = alpha >= 0.0 ? -nrm : nrm;
                tau = (beta - alpha) / beta;
                scal = 1.0 / (alpha - beta);
            }
            if (tid > j) {
                const double sk = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
                w[tid] = A[tid * C + j] + scal * sk;
            }
            if (tid == 0) { cf[0] = tau; cf[1] = scal; cf[2] = beta; }
        }
        __syncthreads();
        const double tau = cf[0], scal = cf[1];
        if (tau != 0.0) {
#pragma unroll
            for (int q = 0; q < RPT; ++q) {
                const int r = tid + q * 256;
                if (r > j) {
                    const double v = A[j * C + r] * scal;
#pragma unroll
                    for (int k = 0; k < M; ++k)
                        if (k > j) A[k * C + r] -= tau * w[k] * v;
                } else if (r == j) {
#pragma unroll
                    for (int k = 0; k < M; ++k)
                        if (k > j) A[k * C + j] -= tau * w[k];
                }
            }
        }
        if (tid == j) A[j * C + j] = cf[2];
        __syncthreads();
    }
    for (int t = tid; t < M * M; t += 256) {
        const int k = t / M, i = t % M;
        Rout[(int64_t)k * ldo + (int64_t)blockIdx.x * M + i] = i <= k ? A[k * C + i] : 0.0;
    }
}

int tsqr_rows_per_block() { return TSQR_C; }

void launch_tsqr(int64_t n, int m, const double *const *cols_dev, double *Rout, int64_t ldo, hipStream_t st) {
    const unsigned nb = (unsigned)((n + TSQR_C - 1) / TSQR_C);
    if (nb == 0) return;
    switch (m) {
#define PLS_TSQR(M) case M: k_tsqr<M><<<nb, 256, 0, st>>>(n, cols_dev, Rout, ldo); break;
        PLS_TSQR(1) PLS_TSQR(2) PLS_TSQR(3) PLS_TSQR(4) PLS_TSQR(5) PLS_TSQR(6) PLS_TSQR(7) PLS_TSQR(8)
        PLS_TSQR(9) PLS_TSQR(10) PLS_TSQR(11) PLS_TSQR(12) PLS_TSQR(13) PLS_TSQR(14) PLS_TSQR(15) PLS_TSQR(16)
#undef PLS_TSQR
        default: return;
    }
}

// ============================================================== SELL-64 ====
// Sliced ELLPACK, slice height = one 64-lane wave: slice s holds rows
// [64 s, 64 s + 64), entry k of its rows stored contiguously
// (sptr[s] + 64 k + lane).  Lane = row, so the val / col streams are fully
// coalesced, no cross-lane reduction is needed, each row sums its entries in
// column order, and for banded / stencil columns the 64 x gathers of one
// wave-instruction hit 4-5 consecutive cache lines instead of 64.
__global__ __launch_bounds__(TPB) void k_sell_slice_len(int64_t nrows, int64_t nslices, const int64_t *rp,
                                                        int64_t *slen) {
    const int64_t sl = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (sl > nslices) return;
    if (sl == nslices) { if (lane == 0) slen[nslices] = 0; return; }
    const int64_t row = sl * 64 + lane;
    int64_t len = row < nrows ? rp[row + 1] - rp[row] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t t = __shfl_xor(len, o);
        len = t > len ? t : len;
    }
    if (lane == 0) slen[sl] = 64 * len;
}

__global__ __launch_bounds__(TPB) void k_sell_fill(int64_t nrows, int64_t nslices, const int64_t *rp, const int32_t *ci,
                                                   const double *val, const int64_t *sptr, int32_t *scol, double *sval) {
    const int64_t sl = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (sl >= nslices) return;
    const int64_t row = sl * 64 + lane;
    const int64_t base = sptr[sl];
    const int64_t L = (sptr[sl + 1] - base) >> 6;
    const int64_t s0 = row < nrows ? rp[row] : 0;
    const int64_t len = row < nrows ? rp[row + 1] - s0 : 0;
    const int32_t padc = len > 0 ? ci[s0 + len - 1] : 0;
    for (int64_t k = 0; k < L; ++k) {
        const int64_t pos = base + k * 64 + lane;
        if (k < len) {
            scol[pos] = ci[s0 + k];
            sval[pos] = val[s0 + k];
        } else {
            scol[pos] = padc;
            sval[pos] = 0.0;
        }
    }
}

// TAG only separates the outer-operator instantiation (TAG 1: y = A x of the
// Krylov loop) from the preconditioner's block products in profiles.
template <int U, int TAG, bool HALO>
__global__ __launch_bounds__(TPB) void k_sell_spmv(int64_t nrows, int64_t nslices, const int64_t *__restrict__ sptr,
                                                   const int32_t *__restrict__ scol, const double *__restrict__ sval,
                                                   const double *__restrict__ x, double *__restrict__ y, double alpha,
                                                   double beta, const double *__restrict__ z,
                                                   const double *__restrict__ ghost, int32_t nlocal) {
    const int lane = threadIdx.x & 63;
    const int64_t sl = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (TPB / 64) + (threadIdx.x >> 6)));
    if (sl >= nslices) return;
    const int64_t base = sptr[sl];
    const int64_t L = (sptr[sl + 1] - base) >> 6;
    const int32_t *cp = scol + base + lane;
    const double *vp = sval + base + lane;
    double acc = 0.0;
    for (int64_t k0 = 0; k0 < L; k0 += U) {
        int32_t c[U];
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t k = k0 + u;
            const int64_t kk = k < L ? k : L - 1;  // wave-uniform clamp, value masked
            c[u] = __builtin_nontemporal_load(cp + kk * 64);
            const double t = __builtin_nontemporal_load(vp + kk * 64);
            v[u] = k < L ? t : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (HALO) {
                const bool loc = c[u] < nlocal;
                const double xv = loc ? x[(uint32_t)c[u]] : ghost[(uint32_t)(c[u] - nlocal)];
                acc += v[u] * xv;
            } else {
                acc += v[u] * x[(uint32_t)c[u]];
            }
        }
    }
    const int64_t row = sl * 64 + lane;
    if (row < nrows) {
        double r = alpha * acc;
        if (beta != 0.0) r += beta * z[row];
        y[row] = r;
    }
}

int64_t sell_nslices(int64_t nrows) { return (nrows + 63) / 64; }

void launch_sell_slice_len(int64_t nrows, const int64_t *rp, int64_t *slen, hipStream_t st) {
    const int64_t ns = sell_nslices(nrows);
    k_sell_slice_len<<<grid_for((ns + 1) * 64, TPB), TPB, 0, st>>>(nrows, ns, rp, slen);
}
void launch_sell_fill(int64_t nrows, const int64_t *rp, const int32_t *ci, const double *val, const int64_t *sptr,
                      int32_t *scol, double *sval, hipStream_t st) {
    const int64_t ns = sell_nslices(nrows);
    if (ns > 0) k_sell_fill<<<grid_for(ns * 64, TPB), TPB, 0, st>>>(nrows, ns, rp, ci, val, sptr, scol, sval);
}
void launch_sell_spmv(int64_t nrows, const int64_t *sptr, const int32_t *scol, const double *sval, const double *x,
                      double *y, double alpha, double beta, const double *z, int tag, const double *ghost,
                      int64_t nlocal, hipStream_t st) {
    const int64_t ns = sell_nslices(nrows);
    if (ns <= 0) return;
    const unsigned g = grid_for(ns, TPB / 64);
    const int32_t nl = (int32_t)nlocal;
    if (ghost) {
        if (tag) k_sell_spmv<8, 1, true><<<g, TPB, 0, st>>>(nrows, ns, sptr, scol, sval, x, y, alpha, beta, z, ghost, nl);
        else k_sell_spmv<8, 0, true><<<g, TPB, 0, st>>>(nrows, ns, sptr, scol, sval, x, y, alpha, beta, z, ghost, nl);
    } else {
        if (tag) k_sell_spmv<8, 1, false><<<g, TPB, 0, st>>>(nrows, ns, sptr, scol, sval, x, y, alpha, beta, z, ghost, nl);
        else k_sell_spmv<8, 0, false><<<g, TPB, 0, st>>>(nrows, ns, sptr, scol, sval, x, y, alpha, beta, z, ghost, nl);
    }
}

// ====================================================== SELL-64 / D16 =====
// Compressed SELL-64: entry k of a lane's stream stores a 16-bit column delta
// (col_k - col_{k-1}, 1..65535) instead of an int32 column, 10 B per entry
// instead of 12.  A delta of 0 means "start the next segment": the column is
// the next of the lane's D16_SEG absolute segment bases (the first entry, and
// every jump > 65535 -- field-block changes, ghost columns).  Padding entries
// are segment starts with value 0.0 (the base index clamps to the last one).
// Lanes per row: a slice is 64 lanes; LPR = 1 (64 rows, lane = row) for rows
// whose neighbours use neighbouring columns, LPR = 8 (8 rows, entry j of a row
// on lane j % 8) for "wide" rows whose neighbours' columns lie far apart (a
// pressure row couples to runs of ~(n_u / n_p) displacement columns): there a
// lane-per-row gather touches 64 cache lines per instruction, 8 lanes per row
// read 8 consecutive columns.  The LPR partial sums are combined by lane
// shuffles (LPR = 1 rows sum in CSR order: bitwise equal to SELL-64).
// Layout for 16-B-per-lane loads (1 KiB per wave instruction):
//   deltas  dl[base + (k / 8) * 512 + lane * 8 + k % 8]   (one uint4 = 8 deltas)
//   values  dv[base + (k / 2) * 128 + lane * 2 + k % 2]   (one double2 = 2 values)
//   bases   seg[(slice * 64 + lane) * D16_SEG + j]        (one int4 per lane)
//   slices  sfirst[slice] (first row), slpr[slice] (lanes per row)
__device__ __forceinline__ void d16_lane(int64_t sl, int lane, const int64_t *sfirst, const int32_t *slpr,
                                         int64_t nrows, int64_t &row, int &lpr, int &sub,
                                         const int32_t *rowmap) {
    lpr = slpr[sl];
    row = sfirst[sl] + lane / lpr;
    sub = lane % lpr;
    if (row >= sfirst[sl + 1] || row >= nrows) row = -1;
    else if (rowmap) row = rowmap[row];
}

// Rows of a reduced layout (rstart): a row served by lpr lanes keeps every remaining entry on
// the lane it has in the full row.  The row lost m = rstart[row] - rp[row] leading entries, so
// with phase = m % lpr lane `sub` takes the remaining entries j' = 0, 1, ... with
// (j' + phase) % lpr == sub: the first at (sub - phase) mod lpr, then every lpr-th.  Phase 0
// (no rstart, nothing skipped, lane-per-row) is the plain rule j' % lpr == sub.
__device__ __forceinline__ int d16_first(int64_t row, int lpr, int sub, const int64_t *rp, const int64_t *rstart) {
    if (!rstart || row < 0 || lpr == 1) return sub;
    const int phase = (int)((rstart[row] - rp[row]) % lpr);
    return (sub - phase + lpr) % lpr;
}

__global__ __launch_bounds__(TPB) void k_d16_slice_len(int64_t nslices, const int64_t *sfirst, const int32_t *slpr,
                                                       const int64_t *rp, int64_t nrows, int64_t *slen,
                                                       const int32_t *rowmap, const int64_t *rstart) {
    const int64_t sl = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (sl > nslices) return;
    if (sl == nslices) { if (lane == 0) slen[nslices] = 0; return; }
    int64_t row;
    int lpr, sub;
    d16_lane(sl, lane, sfirst, slpr, nrows, row, lpr, sub, rowmap);
    const int64_t len = row >= 0 ? rp[row + 1] - (rstart ? rstart[row] : rp[row]) : 0;
    const int first = d16_first(row, lpr, sub, rp, rstart);
    int64_t mine = len > first ? (len - first + lpr - 1) / lpr : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t t = __shfl_xor(mine, o);
        mine = t > mine ? t : mine;
    }
    if (lane == 0) slen[sl] = 64 * ((mine + 7) & ~(int64_t)7);
}

// segments each lane's entry stream needs; *maxseg = max over lanes
__global__ __launch_bounds__(TPB) void k_d16_count(int64_t nslices, const int64_t *sfirst, const int32_t *slpr,
                                                   const int64_t *rp, const int32_t *ci, int64_t nrows,
                                                   int32_t *maxseg, const int32_t *rowmap,
                                                   const int64_t *rstart) {
    const int64_t sl = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (sl >= nslices) return;
    int64_t row;
    int lpr, sub;
    d16_lane(sl, lane, sfirst, slpr, nrows, row, lpr, sub, rowmap);
    if (row < 0) return;
    const int64_t s = rstart ? rstart[row] : rp[row], e = rp[row + 1];
    int nseg = 0;
    int64_t last = -1;
    for (int64_t k = s + d16_first(row, lpr, sub, rp, rstart); k < e; k += lpr) {
        const int64_t c = ci[k];
        if (last < 0 || c - last > 65535 || c <= last) ++nseg;
        last = c;
    }
    if (nseg > 0) atomicMax(maxseg, nseg);
}

__global__ __launch_bounds__(TPB) void k_d16_fill(int64_t nslices, const int64_t *sfirst, const int32_t *slpr,
                                                  const int64_t *rp, const int32_t *ci, const double *val,
                                                  int64_t nrows, const int64_t *sptr, uint16_t *dl, double *dv,
                                                  int32_t *seg, int nsegs, const int32_t *rowmap,
                                                  const int64_t *rstart) {
    const int64_t sl = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (sl >= nslices) return;
    int64_t row;
    int lpr, sub;
    d16_lane(sl, lane, sfirst, slpr, nrows, row, lpr, sub, rowmap);
    const int64_t base = sptr[sl];
    const int64_t L = (sptr[sl + 1] - base) >> 6;
    const int64_t s0 = row >= 0 ? (rstart ? rstart[row] : rp[row]) : 0;
    const int64_t len = row >= 0 ? rp[row + 1] - s0 : 0;
    const int64_t slot = sl * 64 + lane;
    const int first = d16_first(row, lpr, sub, rp, rstart);
    int nseg = 0;
    int32_t last = 0;
    for (int64_t k = 0; k < L; ++k) {
        const int64_t j = k * lpr + first;  // this lane's k-th entry of the row
        uint16_t d = 0;
        double v = 0.0;
        if (j < len) {
            const int32_t c = ci[s0 + j];
            v = val[s0 + j];
            const int64_t gap = (int64_t)c - (int64_t)last;
            if (k == 0 || gap > 65535 || gap <= 0) {
                seg[slot * nsegs + nseg++] = c;
            } else {
                d = (uint16_t)gap;
            }
            last = c;
        }
        dl[base + (k >> 3) * 512 + lane * 8 + (k & 7)] = d;
        dv[base + (k >> 1) * 128 + lane * 2 + (k & 1)] = v;
    }
    if (nseg == 0) seg[slot * nsegs + nseg++] = 0;
    for (int j = nseg; j < nsegs; ++j) seg[slot * nsegs + j] = seg[slot * nsegs + nseg - 1];
}

// ---- shared delta streams (pls.d16_share) ----
// Lanes of a slice whose delta streams are equal over the slice's whole length (padding
// included) form a class; the shared stream stores one 16-B pack per class and 8-entry group,
//   deltas  dls[dptr[slice] + (g * C + cls[slice * 64 + lane]) * 8 + k % 8]   (g = k / 8)
// C = classes of the slice, ids ordered by lowest member lane.  C = 64 with cls = lane is the
// plain stream.  Both kernels read the plain stream k_d16_fill wrote (rowmap and rstart are in
// it already), one wave per slice.
typedef uint32_t d16_u4 __attribute__((ext_vector_type(4)));

// lowest lane whose 64-bit key equals this lane's
__device__ __forceinline__ int d16_lowest_equal(uint64_t key, int lane) {
    int rep = lane;
    for (int j = 63; j >= 0; --j) {
        const uint64_t kj = __shfl(key, j);
        if (kj == key) rep = j;
    }
    return rep;
}

// cls[slice * 64 + lane] and cnt[slice] = C * L (the slice's stored deltas); *nshared counts
// the slices with C < 64.  Each lane hashes its stream, takes the lowest lane with the same
// hash as representative and compares its stream with the representative's pack by pack; one
// mismatch anywhere in the slice (a hash collision) and the slice keeps C = 64.
__global__ __launch_bounds__(TPB) void k_d16_share_classes(int64_t nslices, const int64_t *__restrict__ sptr,
                                                           const uint16_t *__restrict__ dl, uint8_t *cls,
                                                           int64_t *cnt, int64_t *nshared) {
    const int64_t sl = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (sl > nslices) return;
    if (sl == nslices) { if (lane == 0) cnt[nslices] = 0; return; }
    const int64_t base = sptr[sl];
    const int64_t L = (sptr[sl + 1] - base) >> 6;
    const int64_t ng = L >> 3;
    const d16_u4 *dp = reinterpret_cast<const d16_u4 *>(dl + base);
    uint64_t h = 0xcbf29ce484222325ull;
    for (int64_t g = 0; g < ng; ++g) {
        const d16_u4 d = dp[g * 64 + lane];
        h = (h ^ (((uint64_t)d.y << 32) | d.x)) * 0x9e3779b97f4a7c15ull;
        h ^= h >> 29;
        h = (h ^ (((uint64_t)d.w << 32) | d.z)) * 0xbf58476d1ce4e5b9ull;
        h ^= h >> 32;
    }
    const int rep = d16_lowest_equal(h, lane);
    bool same = true;
    if (rep != lane)
        for (int64_t g = 0; g < ng && same; ++g) {
            const d16_u4 a = dp[g * 64 + lane], b = dp[g * 64 + rep];
            same = a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
        }
    const bool ok = !__any(!same);
    const uint64_t reps = ok ? __ballot(rep == lane) : ~0ull;
    const int c = ok ? __popcll(reps & ((1ull << rep) - 1ull)) : lane;
    const int C = __popcll(reps);
    cls[sl * 64 + lane] = (uint8_t)c;
    if (lane == 0) {
        cnt[sl] = C * L;
        if (C < 64) atomicAdd(reinterpret_cast<unsigned long long *>(nshared), 1ull);
    }
}

// the shared stream from the plain one: the lowest lane of every class copies its packs
__global__ __launch_bounds__(TPB) void k_d16_share_fill(int64_t nslices, const int64_t *__restrict__ sptr,
                                                        const int64_t *__restrict__ dptr,
                                                        const uint8_t *__restrict__ cls,
                                                        const uint16_t *__restrict__ dl, uint16_t *dls) {
    const int64_t sl = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (sl >= nslices) return;
    const int64_t base = sptr[sl];
    const int64_t ng = (sptr[sl + 1] - base) >> 9;
    const int c = cls[sl * 64 + lane];
    const bool first = d16_lowest_equal((uint64_t)c, lane) == lane;
    const int C = __popcll(__ballot(first));
    if (!first) return;
    const d16_u4 *src = reinterpret_cast<const d16_u4 *>(dl + base) + lane;
    d16_u4 *dst = reinterpret_cast<d16_u4 *>(dls + dptr[sl]) + c;
    for (int64_t g = 0; g < ng; ++g) dst[g * C] = src[g * 64];
}

// first column of every row (-1: empty row) -- input of the host slice plan
__global__ __launch_bounds__(TPB) void k_first_col(int64_t nrows, const int64_t *rp, const int32_t *ci, int32_t *c0) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r < nrows) c0[r] = rp[r + 1] > rp[r] ? ci[rp[r]] : -1;
}

typedef int32_t d16_i4 __attribute__((ext_vector_type(4)));
typedef double d16_d2 __attribute__((ext_vector_type(2)));
typedef float d16_f4 __attribute__((ext_vector_type(4)));

// The value stream of a D16 layout as k_d16_spmv reads it: one 16-B pack per lane and load,
//   fp64  dv[base + (k / 2) * 128 + lane * 2 + k % 2]    four packs per 8-entry group
//   fp32  dv32[base + (k / 4) * 256 + lane * 4 + k % 4]  two (the low operator, see below)
// get(v, e): entry e of a pack as the fp64 factor of the product.  UNROLL_MAX: the deepest
// unroll of the stream; AUX_STORE: whether the raw-sum store is instantiated for it.
template <class V>
struct d16_values;
template <>
struct d16_values<double> {
    typedef d16_d2 pack;
    static constexpr int PER = 2, UNROLL_MAX = 4;
    static constexpr bool AUX_STORE = true;
    static __device__ __forceinline__ double get(const pack v, int e) { return e ? v.y : v.x; }
};
template <>
struct d16_values<float> {
    typedef d16_f4 pack;
    static constexpr int PER = 4, UNROLL_MAX = 8;
    static constexpr bool AUX_STORE = false;  // the raw-sum store belongs to the fp64 launch
    static __device__ __forceinline__ double get(const pack v, int e) {
        return (double)(e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w);
    }
};

// AUX (a lane's sum is one chain acc += a * x[col] over its entries in CSR order, so a chain
// stopped after a row's first columns and continued from the stored value gives the bits of the
// unbroken one):
//   D16_AUX_STORE  aux[row] = acc, the raw row sum before alpha / beta
//   D16_AUX_INIT   acc starts from aux[row] instead of 0
// on lane-per-row slices.  Slices of W.lpr > 1 lanes per row do the same per lane, before the
// shuffle combine, for the rows [W.lo, W.hi) through W.q[(row - W.lo) * W.lpr + lane % W.lpr]
// (D16Wide; lpr 0: no such rows).  The lanes' entries must be the same in the storing and in
// the continuing layout: d16_first's phase rule.
// V: the value stream's type (d16_values); x, every product (double)a * x[col] and every sum are
// fp64 and in the same order for both.
// (the second launch bound: the unroll-8 halo instantiations stay at 128 VGPRs, 4 waves per SIMD,
// as before the class addressing; without it the allocator takes 138)
template <int G2, int TAG, bool HALO, int SEG, int AUX, class V>
__global__ __launch_bounds__(TPB, (G2 == 8 && SEG == 4 && HALO) ? 4 : 1) void k_d16_spmv(int64_t nrows, int64_t nslices, const int64_t *__restrict__ sptr,
                                                  const int64_t *__restrict__ sfirst,
                                                  const int32_t *__restrict__ slpr,
                                                  const uint16_t *__restrict__ dl, const V *__restrict__ dv,
                                                  const int32_t *__restrict__ seg, const double *__restrict__ x,
                                                  double *__restrict__ y, double alpha, double beta,
                                                  const double *__restrict__ z, const double *__restrict__ ghost,
                                                  int32_t nlocal, const int32_t *__restrict__ slist,
                                                  const int32_t *__restrict__ rowmap, double *aux, int d16_xcd,
                                                  const int64_t *__restrict__ dptr,
                                                  const uint8_t *__restrict__ cls, D16Wide W) {
    static_assert(SEG == 4 || SEG == 8, "segment bases are one or two int4 per lane");
    static_assert(AUX != D16_AUX_STORE || d16_values<V>::AUX_STORE, "the raw-sum store belongs to the fp64 launch");
    typedef typename d16_values<V>::pack pack;
    constexpr int PER = d16_values<V>::PER, NQ = 8 / PER;  // entries per pack, packs per 8-entry group
    const int lane = threadIdx.x & 63;
    // nslices: slices this launch processes -- all of them, or the subset
    // listed in slist (interior / halo rows of a distributed product)
    // d16_xcd (pls.d16_xcd 1): workgroup b runs on XCD b % 8; give each XCD a
    // contiguous range of slices (its L2 then holds one window of x) instead
    // of every 8th slice.  The launcher rounds the grid up to a multiple of 8
    // blocks by the same value, so the map is a permutation of the blocks
    unsigned blk = blockIdx.x;
    if (d16_xcd) {
        const unsigned per = (gridDim.x + 7) / 8;
        blk = (blockIdx.x % 8) * per + blockIdx.x / 8;
    }
    const int64_t idx = __builtin_amdgcn_readfirstlane((int)(blk * (TPB / 64) + (threadIdx.x >> 6)));
    if (idx >= nslices) return;
    const int64_t sl = slist ? (int64_t)__builtin_amdgcn_readfirstlane(slist[idx]) : idx;
    const int64_t base = sptr[sl];
    const int64_t L = (sptr[sl + 1] - base) >> 6;  // multiple of 8
    const int lpr = slpr[sl];
    const int64_t r0 = sfirst[sl], r1 = sfirst[sl + 1];
    const int64_t row = r0 + lane / lpr;
    const d16_i4 sb = __builtin_nontemporal_load(reinterpret_cast<const d16_i4 *>(seg) + (sl * 64 + lane) * (SEG / 4));
    d16_i4 sb2 = sb;
    if (SEG == 8) sb2 = __builtin_nontemporal_load(reinterpret_cast<const d16_i4 *>(seg) + (sl * 64 + lane) * 2 + 1);
    // the delta packs of an 8-entry group lie gs packs apart: 64 (one per lane), or with a
    // shared stream (cls, see k_d16_share_classes) one per class of the slice
    int64_t dbase = base, gs = 64;
    int dlane = lane;
    if (cls) {
        dlane = cls[sl * 64 + lane];
        int C = dlane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int t = __shfl_xor(C, o);
            C = t > C ? t : C;
        }
        gs = __builtin_amdgcn_readfirstlane(C) + 1;
        dbase = dptr[sl];
    }
    const d16_u4 *dp = reinterpret_cast<const d16_u4 *>(dl + dbase) + dlane;
    const pack *vp = reinterpret_cast<const pack *>(dv + base) + lane;
    int32_t col = 0;
    int si = 0;
    double acc = 0.0;
    // (wave-uniform but for the row bounds: a slice is lane-per-row or W.lpr lanes per row)
    const bool wide = AUX != D16_AUX_NONE && lpr > 1 && lpr == W.lpr && row < r1 && row >= W.lo && row < W.hi;
    if (AUX == D16_AUX_INIT && lpr == 1 && row < r1) acc = aux[row];
    if (AUX == D16_AUX_INIT && wide) acc = W.q[(row - W.lo) * lpr + lane % lpr];
    const int64_t ng = L >> 3;
    for (int64_t g0 = 0; g0 < ng; g0 += G2) {
        d16_u4 d[G2];
        pack v[G2][NQ];
#pragma unroll
        for (int u = 0; u < G2; ++u) {
            const int64_t g = g0 + u < ng ? g0 + u : ng - 1;  // wave-uniform clamp, values masked
            d[u] = __builtin_nontemporal_load(dp + g * gs);
#pragma unroll
            for (int q = 0; q < NQ; ++q) v[u][q] = __builtin_nontemporal_load(vp + (g * NQ + q) * 64);
        }
#pragma unroll
        for (int u = 0; u < G2; ++u) {
            if (g0 + u >= ng) break;
            const uint32_t w[4] = {d[u].x, d[u].y, d[u].z, d[u].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int32_t dd = (int32_t)((w[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
                int32_t b = si == 0 ? sb.x : si == 1 ? sb.y : si == 2 ? sb.z : sb.w;
                if (SEG == 8 && si >= 4) b = si == 4 ? sb2.x : si == 5 ? sb2.y : si == 6 ? sb2.z : sb2.w;
                col = dd == 0 ? b : col + dd;
                si += dd == 0 ? 1 : 0;
                const double a = d16_values<V>::get(v[u][e / PER], e % PER);
                if (HALO) {
                    const bool loc = col < nlocal;
                    const double xv = loc ? x[(uint32_t)col] : ghost[(uint32_t)(col - nlocal)];
                    acc += a * xv;
                } else {
                    acc += a * x[(uint32_t)col];
                }
            }
        }
    }
    if (AUX == D16_AUX_STORE && wide) W.q[(row - W.lo) * lpr + lane % lpr] = acc;
    if (lpr > 1) {  // wave-uniform: combine the LPR partial sums of a row
        for (int o = 1; o < lpr; o <<= 1) acc += __shfl_xor(acc, o);
        if (lane % lpr) return;
    }
    if (row < r1) {
        if (AUX == D16_AUX_STORE && lpr == 1) aux[row] = acc;
        // rowmap: slices hold rows sorted by length inside windows (SELL-C-sigma);
        // the lane's result goes to its row's place
        const int64_t yr = rowmap ? (int64_t)rowmap[row] : row;
        if (AUX == D16_AUX_RELAX) {
            // the smoothing step on the row sum (launch_d16_relax): z is b, y is x_new, and the
            // slots this mode leaves free carry a (alpha), g (beta), m (ghost), d (aux) and the
            // RELAX_* flags (nlocal); z[yr] - acc has the bits of spmv's alpha -1, beta 1
            const bool rd = nlocal & RELAX_READ_D;
            const double dn = relax_dn(z[yr] - acc, ghost[yr], beta, alpha, rd ? aux[yr] : 0.0, rd);
            if (nlocal & RELAX_WRITE_D) aux[yr] = dn;
            y[yr] = __dadd_rn(x[yr], dn);
            return;
        }
        double r = alpha * acc;
        if (beta != 0.0) r += beta * z[yr];
        y[yr] = r;
    }
}

void launch_d16_slice_len(int64_t nslices, const int64_t *sfirst, const int32_t *slpr, const int64_t *rp,
                          int64_t nrows, int64_t *slen, hipStream_t st, const int32_t *rowmap, const int64_t *rstart) {
    k_d16_slice_len<<<grid_for((nslices + 1) * 64, TPB), TPB, 0, st>>>(nslices, sfirst, slpr, rp, nrows, slen, rowmap,
                                                                       rstart);
}
void launch_d16_count(int64_t nslices, const int64_t *sfirst, const int32_t *slpr, const int64_t *rp,
                      const int32_t *ci, int64_t nrows, int32_t *maxseg, hipStream_t st, const int32_t *rowmap,
                      const int64_t *rstart) {
    if (nslices > 0)
        k_d16_count<<<grid_for(nslices * 64, TPB), TPB, 0, st>>>(nslices, sfirst, slpr, rp, ci, nrows, maxseg, rowmap,
                                                                 rstart);
}
void launch_d16_fill(int64_t nslices, const int64_t *sfirst, const int32_t *slpr, const int64_t *rp,
                     const int32_t *ci, const double *val, int64_t nrows, const int64_t *sptr, uint16_t *dl,
                     double *dv, int32_t *seg, int nsegs, hipStream_t st, const int32_t *rowmap,
                     const int64_t *rstart) {
    if (nslices > 0)
        k_d16_fill<<<grid_for(nslices * 64, TPB), TPB, 0, st>>>(nslices, sfirst, slpr, rp, ci, val, nrows, sptr, dl,
                                                                dv, seg, nsegs, rowmap, rstart);
}
void launch_d16_share_classes(int64_t nslices, const int64_t *sptr, const uint16_t *dl, uint8_t *cls, int64_t *cnt,
                              int64_t *nshared, hipStream_t st) {
    k_d16_share_classes<<<grid_for((nslices + 1) * 64, TPB), TPB, 0, st>>>(nslices, sptr, dl, cls, cnt, nshared);
}
void launch_d16_share_fill(int64_t nslices, const int64_t *sptr, const int64_t *dptr, const uint8_t *cls,
                           const uint16_t *dl, uint16_t *dls, hipStream_t st) {
    if (nslices > 0)
        k_d16_share_fill<<<grid_for(nslices * 64, TPB), TPB, 0, st>>>(nslices, sptr, dptr, cls, dl, dls);
}
// see launch_coupling_rows (kernels.hpp); one thread per row
__global__ __launch_bounds__(TPB) void k_coupling_rows(int64_t n, int64_t ns, const int64_t *rp, const int32_t *ci,
                                                       const double *val, const int64_t *mrp, const int32_t *mci,
                                                       const double *mval, const uint8_t *reuse, int64_t *rstart,
                                                       int32_t *differs) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= n) return;
    const int64_t s = rp[r], e = rp[r + 1];
    if (r < ns) {
        rstart[r] = s;
        return;
    }
    int64_t lo = s, hi = e;  // first entry with a column >= ns
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ci[mid] < ns) lo = mid + 1;
        else hi = mid;
    }
    const int64_t m0 = mrp[r - ns], cnt = lo - s;
    bool same = mrp[r - ns + 1] - m0 == cnt;
    for (int64_t k = 0; k < cnt && same; ++k)
        same = ci[s + k] == mci[m0 + k] && __double_as_longlong(val[s + k]) == __double_as_longlong(mval[m0 + k]);
    if (!same) *differs = 1;
    rstart[r] = reuse[r] ? lo : s;
}
void launch_coupling_rows(int64_t n, int64_t ns, const int64_t *rp, const int32_t *ci, const double *val,
                          const int64_t *mrp, const int32_t *mci, const double *mval, const uint8_t *reuse,
                          int64_t *rstart, int32_t *differs, hipStream_t st) {
    if (n > 0)
        k_coupling_rows<<<grid_for(n, TPB), TPB, 0, st>>>(n, ns, rp, ci, val, mrp, mci, mval, reuse, rstart, differs);
}
void launch_first_col(int64_t nrows, const int64_t *rp, const int32_t *ci, int32_t *c0, hipStream_t st) {
    if (nrows > 0) k_first_col<<<grid_for(nrows, TPB), TPB, 0, st>>>(nrows, rp, ci, c0);
}
// one launch of k_d16_spmv: the kernel's arguments and where it goes
template <class V>
struct D16Call {
    unsigned g;
    size_t shm;
    hipStream_t st;
    int64_t nrows, ns;
    D16Streams L;
    const V *dv;
    const double *x;
    double *y;
    double alpha, beta;
    const double *z, *ghost;
    int32_t nl;
    const int32_t *slist, *rm;
    double *aux;
    int d16_xcd;
    D16Wide W;
};
template <int G2, int TAG, bool HALO, int SEG, int AUX, class V>
static void d16_go(const D16Call<V> &a) {
    k_d16_spmv<G2, TAG, HALO, SEG, AUX, V><<<a.g, TPB, a.shm, a.st>>>(a.nrows, a.ns, a.L.sptr, a.L.sfirst, a.L.slpr,
                                                                      a.L.dl, a.dv, a.L.seg, a.x, a.y, a.alpha, a.beta,
                                                                      a.z, a.ghost, a.nl, a.slist, a.rm, a.aux, a.d16_xcd,
                                                                      a.L.dptr, a.L.cls, a.W);
}
// the raw-sum store serves the block PC's coupling launches (tag 0, fp64 values only), the
// initial value the outer operator's reduced launch (tag 1); both on one rank only, plain
// layouts (no ghost columns, no rowmap: spmv_slices / MatOp check)
template <int G2, int SEG, class V>
static void d16_dispatch(const D16Call<V> &a, int tag, int aux_mode) {
    if constexpr (d16_values<V>::AUX_STORE)
        if (aux_mode == D16_AUX_STORE) return d16_go<G2, 0, false, SEG, D16_AUX_STORE>(a);
    if (aux_mode != D16_AUX_NONE) return d16_go<G2, 1, false, SEG, D16_AUX_INIT>(a);
    if (a.ghost) {
        if (tag) d16_go<G2, 1, true, SEG, D16_AUX_NONE>(a);
        else d16_go<G2, 0, true, SEG, D16_AUX_NONE>(a);
    } else {
        if (tag) d16_go<G2, 1, false, SEG, D16_AUX_NONE>(a);
        else d16_go<G2, 0, false, SEG, D16_AUX_NONE>(a);
    }
}
// unroll: 1, 2 or 4 (anything else is 4) over fp64 values; 1, 2, 4 or 8 (anything else is 8) over fp32
template <int SEG, class V>
static void d16_unrolled(int unroll, const D16Call<V> &a, int tag, int aux_mode) {
    switch (unroll) {
        case 1: d16_dispatch<1, SEG>(a, tag, aux_mode); break;
        case 2: d16_dispatch<2, SEG>(a, tag, aux_mode); break;
        case 4: d16_dispatch<4, SEG>(a, tag, aux_mode); break;
        default: d16_dispatch<d16_values<V>::UNROLL_MAX, SEG>(a, tag, aux_mode); break;
    }
}
template <class V>
static void d16_launch(int64_t nrows, int64_t nslices, const D16Streams &L, const V *dv, const double *x, double *y,
                       double alpha, double beta, const double *z, int tag, const double *ghost, int64_t nlocal,
                       int unroll, int d16_xcd, hipStream_t st, const int32_t *slist, const int32_t *rowmap,
                       size_t lds_reserve, int aux_mode, double *aux, const D16Wide &W) {
    if (nslices <= 0) return;
    unsigned g = grid_for(nslices, TPB / 64);
    if (d16_xcd) g = (g + 7) / 8 * 8;  // every XCD range the same length (surplus blocks exit)
    D16Call<V> a{g, lds_reserve, st, nrows, nslices, L, dv, x, y, alpha, beta, z, ghost, (int32_t)nlocal, slist,
                 rowmap, aux, d16_xcd, W};
    if (aux_mode != D16_AUX_NONE) {
        a.ghost = nullptr;
        a.nl = 0;
        a.rm = nullptr;
    } else {
        a.aux = nullptr;
        a.W = D16Wide();
    }
    if (L.nsegs == 8) d16_unrolled<8>(unroll, a, tag, aux_mode);
    else d16_unrolled<4>(unroll, a, tag, aux_mode);
}
void launch_d16_spmv(int64_t nrows, int64_t nslices, const D16Streams &L, const double *dv, const double *x, double *y,
                     double alpha, double beta, const double *z, int tag, const double *ghost, int64_t nlocal,
                     int unroll, int d16_xcd, hipStream_t st, const int32_t *slist, const int32_t *rowmap,
                     size_t lds_reserve, int aux_mode, double *aux, const D16Wide &W) {
    d16_launch(nrows, nslices, L, dv, x, y, alpha, beta, z, tag, ghost, nlocal, unroll, d16_xcd, st, slist, rowmap,
               lds_reserve, aux_mode, aux, W);
}
void launch_d16_spmv(int64_t nrows, int64_t nslices, const D16Streams &L, const float *dv32, const double *x, double *y,
                     double alpha, double beta, const double *z, int tag, const double *ghost, int64_t nlocal,
                     int unroll, int d16_xcd, hipStream_t st, const int32_t *slist, const int32_t *rowmap,
                     size_t lds_reserve, const double *aux_init, const D16Wide &W) {
    d16_launch(nrows, nslices, L, dv32, x, y, alpha, beta, z, tag, ghost, nlocal, unroll, d16_xcd, st, slist, rowmap,
               lds_reserve, aux_init ? D16_AUX_INIT : D16_AUX_NONE, const_cast<double *>(aux_init), W);
}
// the smoothing step as k_d16_spmv's epilogue (D16_AUX_RELAX): instantiations of their own beside
// d16_dispatch's (tag 0, no ghost columns, fp64 values), the step's arguments in the free slots
template <int G2, int SEG>
static void d16_relax_go(const D16Call<double> &a) {
    d16_go<G2, 0, false, SEG, D16_AUX_RELAX>(a);
}
void launch_d16_relax(int64_t nrows, int64_t nslices, const D16Streams &L, const double *dv, const double *x,
                      double *x_new, const double *b, const double *m, double *d, double a, double g, int flags,
                      int unroll, int d16_xcd, hipStream_t st, const int32_t *rowmap) {
    if (nslices <= 0) return;
    unsigned grid = grid_for(nslices, TPB / 64);
    if (d16_xcd) grid = (grid + 7) / 8 * 8;
    const D16Call<double> c{grid, 0, st, nrows, nslices, L, dv, x, x_new, a, g, b, m, (int32_t)flags, nullptr,
                            rowmap, d, d16_xcd, D16Wide()};
    const bool s8 = L.nsegs == 8;
    switch (unroll) {
        case 1: s8 ? d16_relax_go<1, 8>(c) : d16_relax_go<1, 4>(c); break;
        case 2: s8 ? d16_relax_go<2, 8>(c) : d16_relax_go<2, 4>(c); break;
        default: s8 ? d16_relax_go<4, 8>(c) : d16_relax_go<4, 4>(c); break;
    }
}

// ------------------------------------------- D16 with fp32 values (low) ---
// The low-precision operator of compressed-operator GMRES (pls_gmres_operator single): the
// layout's deltas, bases and slices as they are, and a second value stream in fp32,
//   values  dv32[base + (k / 4) * 256 + lane * 4 + k % 4]   (one float4 = 4 values)
// so an 8-entry group is one delta load and two value loads of 16 B per lane, 6 B per entry.
// k_d16_round_values fills it from the fp64 stream: every value rounded to nearest even once
// (padding stays 0.0f).  A slice's base is a multiple of 512 entries, so the 256-entry blocks of
// the two streams coincide and the copy needs no slice table: thread t writes float4 t from
// double2 (t / 64) * 128 + t % 64 and the one 64 further.  *overflow = 1 when a finite value
// rounds to an infinity.
__global__ __launch_bounds__(TPB) void k_d16_round_values(int64_t nquads, const double *__restrict__ dv,
                                                          float *__restrict__ dv32, int32_t *overflow) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= nquads) return;
    const d16_d2 *src = reinterpret_cast<const d16_d2 *>(dv) + (t >> 6) * 128 + (t & 63);
    const d16_d2 a = src[0], b = src[64];
    d16_f4 f;
    f.x = (float)a.x;
    f.y = (float)a.y;
    f.z = (float)b.x;
    f.w = (float)b.y;
    const bool bad = (isinf(f.x) && !isinf(a.x)) || (isinf(f.y) && !isinf(a.y)) || (isinf(f.z) && !isinf(b.x)) ||
                     (isinf(f.w) && !isinf(b.y));
    if (bad) *overflow = 1;
    reinterpret_cast<d16_f4 *>(dv32)[t] = f;
}
void launch_d16_round_values(int64_t stored, const double *dv, float *dv32, int32_t *overflow, hipStream_t st) {
    const int64_t nquads = stored / 4;  // stored is a multiple of 512
    if (nquads > 0) k_d16_round_values<<<grid_for(nquads, TPB), TPB, 0, st>>>(nquads, dv, dv32, overflow);
}

// ============================================================ SELL/B3 ======
// Row triples of FE vector fields: the 3 components of a P2 node have the same
// sparsity pattern, so a triple shares one column list.  B3_LPT lanes per
// triple (entry j of the triple's list on lane j % B3_LPT), slices of 64 /
// B3_LPT triples (sorted by length inside windows, tmap[position] = the
// triple's first row); per lane entry kk one column (one x gather serves 3
// rows) and 3 values:  col[base + kk * 64 + lane],
// val[3 * base + (3 kk + r) * 64 + lane].  The lanes' partial sums of a row
// combine by DPP (quad_perm xor 1, xor 2).
constexpr int B3_LPT = 4;

// flag[r] = 1 when rows r, r + 1, r + 2 have the same column list
__global__ __launch_bounds__(TPB) void k_triple_flags(int64_t n, const int64_t *rp, const int32_t *ci, uint8_t *flag) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= n) return;
    uint8_t f = 0;
    if (r + 2 < n) {
        const int64_t s0 = rp[r], len = rp[r + 1] - s0;
        if (len > 0 && rp[r + 2] - rp[r + 1] == len && rp[r + 3] - rp[r + 2] == len) {
            const int64_t s1 = rp[r + 1], s2 = rp[r + 2];
            f = 1;
            for (int64_t k = 0; k < len && f; ++k) f = (ci[s0 + k] == ci[s1 + k] && ci[s0 + k] == ci[s2 + k]) ? 1 : 0;
        }
    }
    flag[r] = f;
}
void launch_triple_flags(int64_t n, const int64_t *rp, const int32_t *ci, uint8_t *flag, hipStream_t st) {
    if (n > 0) k_triple_flags<<<grid_for(n, TPB), TPB, 0, st>>>(n, rp, ci, flag);
}
int b3_lanes_per_triple() { return B3_LPT; }

__global__ __launch_bounds__(TPB) void k_b3_fill(int64_t nslices, int64_t ntrip, const int64_t *bptr,
                                                 const int32_t *tmap, const int64_t *rp, const int32_t *ci,
                                                 const double *val, int32_t *bcol, double *bval) {
    const int64_t sl = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63, sub = lane % B3_LPT;
    if (sl >= nslices) return;
    const int64_t base = bptr[sl], L = (bptr[sl + 1] - base) >> 6;
    const int64_t pos = sl * (64 / B3_LPT) + lane / B3_LPT;
    const int64_t h = pos < ntrip ? tmap[pos] : -1;
    const int64_t s0 = h >= 0 ? rp[h] : 0, len = h >= 0 ? rp[h + 1] - s0 : 0;
    const int32_t c0 = len > 0 ? ci[s0] : 0;
    for (int64_t kk = 0; kk < L; ++kk) {
        const int64_t k = kk * B3_LPT + sub;
        const bool in = k < len;
        bcol[base + kk * 64 + lane] = in ? ci[s0 + k] : c0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int64_t sj = h >= 0 ? rp[h + j] : 0;
            bval[3 * base + (3 * kk + j) * 64 + lane] = in ? val[sj + k] : 0.0;
        }
    }
}

void launch_b3_fill(int64_t nslices, int64_t ntrip, const int64_t *bptr, const int32_t *tmap, const int64_t *rp,
                    const int32_t *ci, const double *val, int32_t *bcol, double *bval, hipStream_t st) {
    if (nslices > 0)
        k_b3_fill<<<grid_for(nslices * 64, TPB), TPB, 0, st>>>(nslices, ntrip, bptr, tmap, rp, ci, val, bcol, bval);
}

__device__ __forceinline__ double b3_dpp(double v, int ctrl_xor) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    if (ctrl_xor == 1)
        return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xF, 0xF, false),
                                __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xF, 0xF, false));
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xF, 0xF, false),
                            __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xF, 0xF, false));
}

template <int TAG>
__global__ __launch_bounds__(TPB) void k_b3_spmv(int64_t nslices, int64_t ntrip, const int64_t *__restrict__ bptr,
                                                 const int32_t *__restrict__ tmap, const int32_t *__restrict__ bcol,
                                                 const double *__restrict__ bval, const double *__restrict__ x,
                                                 double *__restrict__ y, double alpha, double beta,
                                                 const double *__restrict__ z) {
    const int64_t sl = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (TPB / 64) + (threadIdx.x >> 6)));
    if (sl >= nslices) return;
    const int lane = threadIdx.x & 63;
    const int64_t base = bptr[sl], L = (bptr[sl + 1] - base) >> 6;
    const int32_t *cp = bcol + base + lane;
    const double *vp = bval + 3 * base + lane;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    int64_t k = 0;
    for (; k + 4 <= L; k += 4) {  // 4 entries per lane in flight
        int32_t c[4];
        double v[4][3], xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) c[u] = __builtin_nontemporal_load(cp + (k + u) * 64);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int j = 0; j < 3; ++j) v[u][j] = __builtin_nontemporal_load(vp + (3 * (k + u) + j) * 64);
            xv[u] = x[(uint32_t)c[u]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a0 += v[u][0] * xv[u];
            a1 += v[u][1] * xv[u];
            a2 += v[u][2] * xv[u];
        }
    }
    for (; k < L; ++k) {
        const double xv = x[(uint32_t)cp[k * 64]];
        a0 += vp[(3 * k) * 64] * xv;
        a1 += vp[(3 * k + 1) * 64] * xv;
        a2 += vp[(3 * k + 2) * 64] * xv;
    }
    static_assert(B3_LPT == 4, "two DPP steps combine the lanes of a triple");
    a0 += b3_dpp(a0, 1); a1 += b3_dpp(a1, 1); a2 += b3_dpp(a2, 1);
    a0 += b3_dpp(a0, 2); a1 += b3_dpp(a1, 2); a2 += b3_dpp(a2, 2);
    const int64_t pos = sl * (64 / B3_LPT) + lane / B3_LPT;
    if (pos >= ntrip || (lane % B3_LPT) >= 3) return;
    // lanes 0, 1, 2 of a triple write its rows 0, 1, 2
    const int j = lane % B3_LPT;
    const int64_t row = tmap[pos] + j;
    const double acc = j == 0 ? a0 : j == 1 ? a1 : a2;
    double r = alpha * acc;
    if (beta != 0.0) r += beta * z[row];
    y[row] = r;
}
void launch_b3_spmv(int64_t nslices, int64_t ntrip, const int64_t *bptr, const int32_t *tmap, const int32_t *bcol,
                    const double *bval, const double *x, double *y, double alpha, double beta, const double *z,
                    int tag, hipStream_t st) {
    if (nslices <= 0) return;
    const unsigned g = grid_for(nslices, TPB / 64);
    if (tag) k_b3_spmv<1><<<g, TPB, 0, st>>>(nslices, ntrip, bptr, tmap, bcol, bval, x, y, alpha, beta, z);
    else k_b3_spmv<0><<<g, TPB, 0, st>>>(nslices, ntrip, bptr, tmap, bcol, bval, x, y, alpha, beta, z);
}

// rows whose last (largest) column is a ghost column (rows sorted): flag 1
__global__ __launch_bounds__(TPB) void k_row_has_ghost(int64_t nrows, const int64_t *rp, const int32_t *ci,
                                                       int64_t nlocal, uint8_t *flag) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r < nrows) flag[r] = (rp[r + 1] > rp[r] && ci[rp[r + 1] - 1] >= nlocal) ? 1 : 0;
}
void launch_row_has_ghost(int64_t nrows, const int64_t *rp, const int32_t *ci, int64_t nlocal, uint8_t *flag,
                          hipStream_t st) {
    if (nrows > 0) k_row_has_ghost<<<grid_for(nrows, TPB), TPB, 0, st>>>(nrows, rp, ci, nlocal, flag);
}

// ======================================================= chain sweep ====
// Blocks whose level DAG is deep and narrow -- FE rows in their natural
// order, ~2-3 rows per level: the classical AMG's hybrid Gauss-Seidel chunks
// (footing's solid block, the synthetic N=59 s block) -- spend their time in
// the per-level hand-off, not in bytes: the workgroup sweep above pays a
// barrier and a two-level-deep prefetch per level (~0.77 us per level on the
// footing N=128 chunks).  Here ONE wave walks a block's rows in STEPS of one
// 16-lane DPP row each -- the rows of a step belong to one level, so they are
// independent; a level with more rows takes several steps, one after the
// other -- with no barrier (the LDS accesses of one wave complete in order).
// A slice packs up to 4 consecutive steps (lanes 16q .. 16q + 15: step q),
// and NW_D slices of factor data are in flight (6 loads each: the in-order
// vmcnt covers <= 63 outstanding), i.e. up to 32 steps of look-ahead.
//
// Stream layout (per triangle, runtime.cpp build_chain_tri): a slice is nl *
// L entries (nl = 16 x its steps, L = 8 entries per lane, lane-major), lane
// l's header (col = local row | count << SW_ROW_BITS, SW_ROW_PAD: no row; val
// = 1 / U_ii for the upper triangle) then its factor entries at l * L, unused
// ones (column 0, value 0: summed unmasked); slices follow one another, and a separate array holds every slice's size
// | (L == 8), read 64 slices at a time into a vector register (lane l: slice
// w0 + l) and picked with v_readlane.  A row's entries are dealt round robin
// over its LPR lanes and the partial sums combined by the DPP tree of
// sw2_finish, as in the LDS sweep: with the same lanes per row the results are
// bitwise those of k_ilu_blocks_lds.
static constexpr int NW_D = 8;  // slices in flight per wave
struct NwSlot {
    int32_t c[8];
    double v[8];
    int nl;  // active lanes of this slice (16 per step)
};

__device__ __forceinline__ void nw_issue(const int32_t *col, const double *val, int64_t base, int32_t szf, int lane,
                                         NwSlot &s) {
    const int L = (szf & 1) ? 8 : 4;
    s.nl = (szf & ~3) / L;
    const int sz = szf & ~3;
    // range-checked to the slice: lanes past nl and slices past the block's
    // end (size 0) read zeros without traffic; every path issues the same
    // 6 loads, so the compiler's vmcnt bookkeeping stays exact
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void *)(col + base), (short)0, sz * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void *)(val + base), (short)0, sz * 8, 0x00020000);
    const int off = lane * L;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const auto c4 = __builtin_amdgcn_raw_buffer_load_b128(rc, (off + 4 * q) * 4, 0, 0);
        s.c[4 * q + 0] = (int32_t)c4[0];
        s.c[4 * q + 1] = (int32_t)c4[1];
        s.c[4 * q + 2] = (int32_t)c4[2];
        s.c[4 * q + 3] = (int32_t)c4[3];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const auto v4 = __builtin_amdgcn_raw_buffer_load_b128(rv, (off + 2 * q) * 8, 0, 0);
        s.v[2 * q + 0] = __builtin_bit_cast(double, ((uint64_t)v4[1] << 32) | v4[0]);
        s.v[2 * q + 1] = __builtin_bit_cast(double, ((uint64_t)v4[3] << 32) | v4[2]);
    }
}

template <int LPR>
__device__ __forceinline__ void nw_compute(const NwSlot &s, double *ys, int lane, bool upper) {
    const int nsteps = s.nl >> 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // the slice's steps in order: step q is lanes 16q .. 16q + 15
        if (q < nsteps && (lane >> 4) == q) {
            const int32_t h = s.c[0];
            const int32_t li = h & SW_ROW_PAD;
            // the row's own input first, then every dependency read before the first is consumed
            const double yi = ys[li != SW_ROW_PAD ? li : 0];
            double acc = 0.0, d[8];
            // entries past a lane's count are stored as (column 0, value 0): no
            // per-entry masking, and 0 * y adds nothing (the LDS sweep's sums bitwise)
#pragma unroll
            for (int u = 1; u < 8; ++u) d[u] = ys[s.c[u]];
#pragma unroll
            for (int u = 1; u < 8; ++u) acc += __dmul_rn(s.v[u], d[u]);  // no contraction: the LDS sweep's rounding
            constexpr int lg = LPR >= 16 ? 4 : LPR >= 8 ? 3 : LPR >= 4 ? 2 : LPR >= 2 ? 1 : 0;
            if (lg >= 1) acc += dpp_d<0xB1>(acc);
            if (lg >= 2) acc += dpp_d<0x4E>(acc);
            if (lg >= 3) acc += dpp_d<0x141>(acc);
            if (lg >= 4) acc += dpp_d<0x140>(acc);
            if ((lane & (LPR - 1)) == 0 && li != SW_ROW_PAD)
                ys[li] = upper ? (yi - acc) * s.v[0] : yi - acc;
        }
    }
}

template <int LPR>
__device__ __forceinline__ void nw_sweep(int64_t base, const int32_t *sz, int64_t nsl, const int32_t *col,
                                         const double *val, double *ys, int lane, bool upper) {
    if (nsl <= 0) return;
    // slice sizes: lane l of `win` holds slice w0 + l, of `nxt` slice w0 + 64 + l
    // (loaded a window ahead, so picking from it never waits on a fresh load)
    int64_t w0 = 0;
    int32_t win = lane < nsl ? sz[lane] : 0;
    int32_t nxt = 64 + lane < nsl ? sz[64 + lane] : 0;
    auto size_of = [&](int64_t t) -> int32_t {
        if (t >= nsl) return 0;
        const int d = (int)(t - w0);
        return d < 64 ? __builtin_amdgcn_readlane(win, d) : __builtin_amdgcn_readlane(nxt, d - 64);
    };
    NwSlot s[NW_D];
    int64_t ib = base;  // where the next issued slice starts
#pragma unroll
    for (int k = 0; k < NW_D; ++k) {
        const int32_t f = size_of(k);
        nw_issue(col, val, ib, f, lane, s[k]);
        ib += f & ~3;
    }
    // whole rounds of NW_D slices without an exit inside (a loop exit between the
    // slots makes the compiler's vmcnt bookkeeping give up at the loop header and
    // drain every load in flight), then the last nsl % NW_D slices
    const int64_t rounds = nsl / NW_D;
    for (int64_t j = 0; j < rounds; ++j) {
        const int64_t t0 = (j + 1) * NW_D;  // first slice issued this round
        if (t0 >= w0 + 64) {  // move the window (the next one is loaded now, needed >= 7 rounds later)
            w0 += 64;
            win = nxt;
            nxt = w0 + 64 + lane < nsl ? sz[w0 + 64 + lane] : 0;
        }
#pragma unroll
        for (int k = 0; k < NW_D; ++k) {
            nw_compute<LPR>(s[k], ys, lane, upper);
            const int32_t f = size_of(t0 + k);
            nw_issue(col, val, ib, f, lane, s[k]);
            ib += f & ~3;
        }
    }
    const int rem = (int)(nsl - rounds * NW_D);
#pragma unroll
    for (int k = 0; k < NW_D; ++k)
        if (k < rem) nw_compute<LPR>(s[k], ys, lane, upper);
}

__device__ __forceinline__ void nw_dispatch(int lpr, int64_t base, const int32_t *sz, int64_t nsl,
                                            const int32_t *col, const double *val, double *ys, int lane,
                                            bool upper) {
    switch (lpr) {
        case 16: nw_sweep<16>(base, sz, nsl, col, val, ys, lane, upper); break;
        case 8: nw_sweep<8>(base, sz, nsl, col, val, ys, lane, upper); break;
        case 4: nw_sweep<4>(base, sz, nsl, col, val, ys, lane, upper); break;
        case 2: nw_sweep<2>(base, sz, nsl, col, val, ys, lane, upper); break;
        default: nw_sweep<1>(base, sz, nsl, col, val, ys, lane, upper); break;
    }
}

__global__ __launch_bounds__(64) void k_ilu_blocks_chain(
    int64_t n, int64_t nblocks, const int64_t *__restrict__ bstart, const int64_t *__restrict__ Lbase,
    const int64_t *__restrict__ Lsoff, const int32_t *__restrict__ Lsz, const int64_t *__restrict__ Lnsl,
    const int32_t *__restrict__ Llpr,
    const int32_t *__restrict__ Lcol, const double *__restrict__ Lval, const int64_t *__restrict__ Ubase,
    const int64_t *__restrict__ Usoff, const int32_t *__restrict__ Usz, const int64_t *__restrict__ Unsl,
    const int32_t *__restrict__ Ulpr,
    const int32_t *__restrict__ Ucol, const double *__restrict__ Uval, const double *x, double *y) {
    extern __shared__ __attribute__((aligned(16))) double ys[];
    const int64_t blk = nblocks - 1 - (int64_t)blockIdx.x;  // heaviest (last) blocks first
    int64_t b0, len;
    block_range(blk, n, nblocks, bstart, b0, len);
    const int lane = threadIdx.x;
    for (int64_t t = lane; t < len; t += 64) ys[t] = x[b0 + t];
    __syncthreads();
    nw_dispatch(Llpr[blk], Lbase[blk], Lsz + Lsoff[blk], Lnsl[blk], Lcol, Lval, ys, lane, false);
    nw_dispatch(Ulpr[blk], Ubase[blk], Usz + Usoff[blk], Unsl[blk], Ucol, Uval, ys, lane, true);
    __syncthreads();
    for (int64_t t = lane; t < len; t += 64) y[b0 + t] = ys[t];
}

int ilu_chain_depth() { return NW_D; }
int ilu_chain_max_lpr() { return 16; }

void launch_ilu_blocks_chain(int64_t n, int64_t nblocks, const int64_t *bstart, const int64_t *Lbase,
                             const int64_t *Lsoff, const int32_t *Lsz, const int64_t *Lnsl, const int32_t *Llpr,
                             const int32_t *Lcol, const double *Lval, const int64_t *Ubase, const int64_t *Usoff,
                             const int32_t *Usz, const int64_t *Unsl, const int32_t *Ulpr, const int32_t *Ucol,
                             const double *Uval, const double *x, double *y, int64_t max_len, hipStream_t st) {
    static bool configured = false;
    if (!configured) {
        (void)hipFuncSetAttribute((const void *)k_ilu_blocks_chain, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)163840);
        configured = true;
    }
    const size_t bytes = (size_t)std::max<int64_t>(max_len, 1) * 8;
    k_ilu_blocks_chain<<<(unsigned)nblocks, 64, bytes, st>>>(n, nblocks, bstart, Lbase, Lsoff, Lsz, Lnsl, Llpr, Lcol,
                                                             Lval, Ubase, Usoff, Usz, Unsl, Ulpr, Ucol, Uval, x, y);
}

// ============================================================ window sweep ====
// Triangular sweeps of LDS-resident blocks in windows of 64 consecutive rows
// (lane = row): y_w = T_w^-1 (b_w - A_{w,off} y_off) with T_w the window's
// diagonal block of the triangle (unit lower for L, with the diagonal for U)
// inverted once at setup and stored column-major ([k][lane]), and A_{w,off}
// the rows' entries outside the window on the solved side (SELL: [k][lane],
// block-local columns, padding = column 0 with value 0).  The dependent chain
// of a block is its windows (len / 64 steps of a 64 x 64 GEMV) instead of its
// levels: FE rows in natural order have ~1 row per level (the AMG smoother's
// chunks: ~970 levels per 2,405-row chunk, 38 windows).
// Four waves per block: wave q takes the stream entries k = q, q + 4, ... and
// the inverse's columns [16 q, 16 q + 16); the partial sums meet in LDS in a
// fixed order (two barriers per window).  Each wave prefetches its share of
// the next window (16 columns of T^-1, WIN_KPW stream entries per lane) into
// registers, reloading each right after its use with range-checked buffer
// loads (the zero triangle of T^-1 and entries past the window's stream read
// 0 without traffic), so a window's data was requested a window earlier and
// the register set stays small enough for the compiler to count the loads in
// flight.  (One wave with all 64 columns spilled to AGPRs and drained vmcnt at
// every window; staging through LDS by LDS-DMA cost ~4.4 us per window in
// 1-KiB copies.)  Rows have at most WIN_KP off-window entries (the setup
// keeps other blocks on the other sweeps), so every load is of fixed count.
static constexpr int WIN_NW = 4, WIN_KPW = 8;
static constexpr int WIN_KP = WIN_NW * WIN_KPW;  // stream entries per row (every one prefetched); blocks with more use other sweeps

// a block's window stream offsets, 64 per vector register (lane l: window j * 64 + l),
// picked with v_readlane: no scalar load (and its latency) per window
// (WIN_OFFR registers hold 64 * WIN_OFFR offsets: every window of a block up to
// ilu_window_max_rows() rows plus the end offset -- 312 for 19,904 rows)
static constexpr int WIN_OFFR = 5;
// the ring variant (blocks longer than LDS): offsets in LDS, up to 1,023 windows
static constexpr int WIN_OFFR_RING = 16, WIN_RING = 16384;
template <int R>
struct WinOff {
    int64_t r[R];
    __device__ __forceinline__ int64_t at(int64_t w) const {  // branch-free: R readlanes, scalar selects
        // (vector selects of the window's register and one readlane: the compiler
        // turned r[] into a scratch array indexed per window, whose loads drain
        // vmcnt -- the ring variant keeps its offsets in LDS instead)
        const int j = (int)(w >> 6), l = (int)(w & 63);
        int64_t v = readlane64(r[0], l);
#pragma unroll
        for (int k = 1; k < R; ++k) {
            const int64_t t = readlane64(r[k], l);
            v = j == k ? t : v;
        }
        return v;
    }
};

// a wave-uniform value forced into scalar registers (buffer resources must be SGPRs;
// without this the compiler may build them in VGPRs and waterfall every load)
__device__ __forceinline__ int64_t sgpr64(int64_t v) {
    const int32_t lo = __builtin_amdgcn_readfirstlane((int32_t)(uint32_t)(uint64_t)v);
    const int32_t hi = __builtin_amdgcn_readfirstlane((int32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t win_rsrc(const void *base, int64_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)(uintptr_t)sgpr64((int64_t)(uintptr_t)base), (short)0,
                                             __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
}

typedef double win_d2 __attribute__((ext_vector_type(2)));
typedef int win_i3 __attribute__((ext_vector_type(3)));  // a stream record: value (lo, hi), column
template <int KPW>
struct WinBuf {  // one wave's share of a window's data in registers
    win_d2 tv[8];     // T^-1 columns 16 q + 2 j, + 1 of the lane's row
    win_i3 sr[KPW];   // stream records: value (.x lo, .y hi), column (.z)
    double rx;            // (ring variant) the window's input rows, from global memory
};

// Range-checked buffer loads (the inverse's column pairs 16 bytes, stream
// records 12) issued through inline asm: the compiler does not track them, so
// it cannot drain them at the loop header (its waits for loop-carried loads
// were vmcnt(0)); the sweep counts them itself -- every window issues the same
// number -- and win_wait ties the registers to the wait (no use or copy can
// move above it).  (Round 6: 8-byte loads, two per stream entry, were 33
// instructions per wave and window, and the loads -- whole wave-wide
// transfers: out-of-range or exec-masked lanes cost the same -- took ~1.1 of
// the ~1.9 us per window on the swelling N = 160 chunks.)
// (KPW: stream records per wave and window -- 4 where no row has more than 16
// off-window entries, else WIN_KPW.  Loading only the records inside each
// window's stream -- a wave-uniform count, waited for through a switch of
// vmcnt immediates -- was measured slower: 274 against 239 us per swelling
// N = 80 level-0 sweep, 1,420 against 1,361 at N = 160)
template <bool RING, int KPW>
constexpr int win_loads() { return 8 + KPW + (RING ? 1 : 0); }
__device__ __forceinline__ double win_ld64(__amdgpu_buffer_rsrc_t r, int off) {
    double v;
    asm volatile("buffer_load_dwordx2 %0, %1, %2, 0 offen" : "=v"(v) : "v"(off), "s"(r) : "memory");
    return v;
}
__device__ __forceinline__ win_d2 win_ld128(__amdgpu_buffer_rsrc_t r, int off) {
    win_d2 v;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(v) : "v"(off), "s"(r) : "memory");
    return v;
}
__device__ __forceinline__ win_i3 win_ld96(__amdgpu_buffer_rsrc_t r, int off) {
    win_i3 v;
    asm volatile("buffer_load_dwordx3 %0, %1, %2, 0 offen" : "=v"(v) : "v"(off), "s"(r) : "memory");
    return v;
}
__device__ __forceinline__ void win_st64(__amdgpu_buffer_rsrc_t r, int off, double v) {
    asm volatile("buffer_store_dwordx2 %0, %1, %2, 0 offen" ::"v"(v), "v"(off), "s"(r) : "memory");
}
template <int N, bool RING, int KPW>
__device__ __forceinline__ void win_wait(WinBuf<KPW> &B) {  // vmcnt(N), B's registers pinned to it
    asm volatile("s_waitcnt vmcnt(%c0)" ::"n"(N) : "memory");
#pragma unroll
    for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(B.tv[k]));
#pragma unroll
    for (int u = 0; u < KPW; ++u) asm volatile("" : "+v"(B.sr[u]));
    if (RING) asm volatile("" : "+v"(B.rx));
}

// RING: ys is a ring of WIN_RING rows (row r in slot r mod WIN_RING; the setup
// checks that no row depends on one more than WIN_RING - 64 rows away), the
// window's input rows come from global memory (in, prefetched with the window's
// data) and its solution goes to global memory (out) as well as to the ring
template <bool UP, int WD, bool RING, int KPW>
__device__ __forceinline__ void win_sweep(int64_t len, int64_t w0, const int64_t *__restrict__ woff,
                                          const int32_t *__restrict__ rec, const double *__restrict__ tinv, double *ys,
                                          double *part, int lane, int q, const double *in = nullptr,
                                          double *out = nullptr, int64_t *lwo_lds = nullptr) {
    constexpr int R = RING ? 1 : WIN_OFFR, NL = win_loads<RING, KPW>();  // (ring: offsets in LDS)
    constexpr int64_t RM = WIN_RING - 1;
    const int64_t nw = (len + 63) >> 6;
    if (nw == 0) return;
    // the block's window stream offsets: registers (64 per register, picked by a
    // vector select and one readlane), or -- ring variant -- LDS (part + 576,
    // up to 1,024; a same-address read per window)
    // (the LDS variant too where they fit after the block: lwo_lds)
    WinOff<R> wo;
    int64_t *lwo = RING ? reinterpret_cast<int64_t *>(part + 576) : lwo_lds;
    const bool in_lds = RING || lwo_lds != nullptr;  // (uniform)
    if (in_lds) {
        for (int64_t t = threadIdx.x; t <= nw; t += 256) lwo[t] = woff[w0 + t];
        __syncthreads();
    } else {
#pragma unroll
        for (int j = 0; j < R; ++j) wo.r[j] = j * 64 + lane <= nw ? woff[w0 + j * 64 + lane] : 0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the offsets (ordinary loads) before the counted ones
    auto at = [&](int64_t w) -> int64_t { return in_lds ? sgpr64(lwo[w]) : wo.at(w); };
    const auto rin = win_rsrc(in, RING ? len * 8 : 0), rout = win_rsrc(out, RING ? len * 8 : 0);
    auto wi = [&](int64_t ww) { return UP ? nw - 1 - ww : ww; };
    // T^-1[lane][k], T^-1[lane][k + 1] (k even): both zero above (L) / below (U)
    // the diagonal -- those lanes read out of range
    auto toff = [&](int k) {
        return (UP ? k + 1 >= lane : k <= lane) ? (k >> 1) * 1024 + lane * 16 : 0x40000000;
    };
    auto sk = [&](int u) { return (u * WIN_NW + q) * 64 + lane; };  // this wave's u-th stream slot
    // every window's loads, NL in one fixed order (past the block: 0 bytes in range, no traffic)
    auto issue = [&](int64_t ww, WinBuf<KPW> &B) {
        const int64_t ok = ww < nw ? 1 : 0;
        const int64_t w = wi(ww < nw ? ww : 0);
        const int64_t s0 = at(w), s1 = at(w + 1);
        const auto rt = win_rsrc(tinv + (w0 + w) * 4096, ok * 32768);
        const auto rs = win_rsrc(rec + 3 * s0, ok * (s1 - s0) * 12);
#pragma unroll
        for (int u = 0; u < KPW; ++u) B.sr[u] = win_ld96(rs, sk(u) * 12);
#pragma unroll
        for (int j = 0; j < 8; ++j) B.tv[j] = win_ld128(rt, toff(16 * q + 2 * j));
        // (ring: wave 0 alone loads the input rows and stores the solution -- the
        // load instructions, not their lanes, are what a window costs)
        if (RING && q == 0) B.rx = win_ld64(rin, (int)(ok * (w * 64 + lane) * 8 + (1 - ok) * 0x40000000));
    };
    // one window, branch-free (a window past the block computes zeros into a dummy slot)
    auto compute = [&](int64_t ww, const WinBuf<KPW> &B) {
        const int64_t w = wi(ww < nw ? ww : 0);
        const int64_t r = w * 64 + lane;
        const bool act = ww < nw && r < len;
        double d[KPW];
#pragma unroll
        for (int u = 0; u < KPW; ++u) {
            const int32_t c = B.sr[u].z;
            d[u] = ys[RING ? (c & RM) : c];
        }
        double acc = 0.0;
#pragma unroll
        for (int u = 0; u < KPW; ++u) acc += __dmul_rn(__hiloint2double(B.sr[u].y, B.sr[u].x), d[u]);
        part[q * 64 + lane] = acc;
        double *rxs = part + 512;  // (ring: wave 0's input rows for every wave)
        if (RING && q == 0) rxs[lane] = B.rx;
        __syncthreads();
        const double rhs = RING ? rxs[lane] : ys[act ? r : 0];
        const double t = act ? rhs - (((part[lane] + part[64 + lane]) + part[128 + lane]) + part[192 + lane]) : 0.0;
        // t_k to every lane through the wave's own LDS slot (its own write: no
        // barrier; same-address reads broadcast) -- 32 v_readlane before
        double *tbq = part + 256 + q * 64;
        tbq[lane] = t;
        double out = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) out += __dmul_rn((k & 1) ? B.tv[k >> 1].y : B.tv[k >> 1].x, tbq[16 * q + k]);
        __syncthreads();  // every wave has read part[] (t) before it is overwritten
        part[q * 64 + lane] = out;
        __syncthreads();
        const double yr = ((part[lane] + part[64 + lane]) + part[128 + lane]) + part[192 + lane];
        if (RING) {
            // every wave stores the window (the same values): one counted store per
            // wave and window, issued after the window's loads
            ys[act ? (r & RM) : WIN_RING + lane] = yr;
            if (q == 0) win_st64(rout, act ? (int)(r * 8) : 0x40000000, yr);
        } else {
            ys[act ? r : len + lane] = yr;  // every wave writes the same value (its own later reads see it)
        }
        __syncthreads();  // part[] free for the next window
        // (measured: double-buffering part[] to drop this barrier and the one above
        // was no faster -- 1,612 against 1,531 us per swelling N=160 chunk sweep)
    };
    if (WD == 3 && !RING) {
        // three windows of data in flight: the oldest window's loads are followed
        // by exactly 2 NL younger ones
        static_assert(2 * NL <= 63, "vmcnt counts 63");
        WinBuf<KPW> A, B, C;
        issue(0, A);
        issue(1, B);
        issue(2, C);
        for (int64_t ww = 0; ww < nw; ww += 3) {
            win_wait<2 * NL, false>(A);
            compute(ww, A);
            issue(ww + 3, A);
            win_wait<2 * NL, false>(B);
            compute(ww + 1, B);
            issue(ww + 4, B);
            win_wait<2 * NL, false>(C);
            compute(ww + 2, C);
            issue(ww + 5, C);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    }
    // (ring: a window's store sits between its successor's loads and the next
    // issue; vector memory completes in issue order, so one more may be pending)
    // (ring: only wave 0 has the input load and the store; the other waves
    // count NL - 1 loads per window and no store)
    auto run = [&](auto w0) {
        constexpr bool S = RING && decltype(w0)::value;
        constexpr int NLq = RING && !S ? NL - 1 : NL, WT = S ? NL + 1 : NLq;
        WinBuf<KPW> A, B;
        issue(0, A);
        issue(1, B);
        if (S) win_wait<NLq, RING>(A);  // (no store yet between A and B)
        for (int64_t ww = 0; ww < nw; ww += 2) {  // two windows per trip: loads of window ww + 2 fly during ww + 1
            win_wait<WT, RING>(A);                // A's loads are older than B's (and a store)
            compute(ww, A);
            issue(ww + 2, A);
            win_wait<WT, RING>(B);
            compute(ww + 1, B);
            issue(ww + 3, B);
        }
    };
    if (RING && q == 0)
        run(std::integral_constant<bool, true>{});
    else
        run(std::integral_constant<bool, false>{});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the prefetches past the block: nothing in range)
}

template <int WD, bool RING, int KL, int KU>
__global__ __launch_bounds__(256) void k_ilu_blocks_window(int64_t n, int64_t nblocks, const int64_t *__restrict__ bstart,
                                                           const int64_t *__restrict__ wstart,
                                                           const int64_t *__restrict__ Lwoff, const int32_t *__restrict__ Lrec,
                                                           const double *__restrict__ Ltinv,
                                                           const int64_t *__restrict__ Uwoff, const int32_t *__restrict__ Urec,
                                                           const double *__restrict__ Utinv, const double *x, double *y,
                                                           int tri, int lwo_ok) {
    // one dynamic LDS array: the partial sums (4 x 64), the waves' t (4 x 64), then the block solution
    extern __shared__ __attribute__((aligned(16))) double lds_win[];
    double *part = lds_win, *ys = lds_win + 512;
    const int64_t blk = nblocks - 1 - (int64_t)blockIdx.x;
    int64_t b0, len;
    block_range(blk, n, nblocks, bstart, b0, len);
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (v_readlane's lane is a scalar)
    if (RING)  // (padding entries read slot 0 with value 0: every slot finite)
        for (int64_t t = threadIdx.x; t < WIN_RING; t += 256) ys[1088 + t] = 0.0;  // (the ring: after rows, offsets)
    else
        for (int64_t t = threadIdx.x; t < len; t += 256) ys[t] = x[b0 + t];
    __syncthreads();
    // block bounds as scalars (buffer resources built from them must live in SGPRs)
    auto uni = [](int64_t v) {
        const int32_t lo = __builtin_amdgcn_readfirstlane((int32_t)(uint32_t)(uint64_t)v);
        const int32_t hi = __builtin_amdgcn_readfirstlane((int32_t)((uint64_t)v >> 32));
        return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
    };
    len = uni(len);
    const int64_t w0 = uni(wstart[blk]);
    if (RING) {
        // L: x -> y (global and the ring); U: y -> y in place, its input rows read
        // from global memory after every wave's L stores completed (win_sweep ends
        // with vmcnt(0); the barrier orders them before U's first loads)
        // (tri: 1 L, 2 U -- y already holds L's solution, the ring then only U's rows -- 3 both)
        // (ring layout: partial sums, t, wave 0's input rows (64), the window
        // offsets (1,024), then the ring)
        if (tri & 1) win_sweep<false, 2, true, KL>(len, w0, Lwoff, Lrec, Ltinv, ys + 1088, part, lane, q, x + b0, y + b0);
        __syncthreads();
        if (tri & 2) win_sweep<true, 2, true, KU>(len, w0, Uwoff, Urec, Utinv, ys + 1088, part, lane, q, y + b0, y + b0);
        return;
    }
    // (the window offsets after the block and its dummy slots, where the launch sized LDS for them)
    int64_t *lwo = lwo_ok ? reinterpret_cast<int64_t *>(ys + len + 64) : nullptr;
    win_sweep<false, WD, false, KL>(len, w0, Lwoff, Lrec, Ltinv, ys, part, lane, q, nullptr, nullptr, lwo);
    __syncthreads();  // (L's last offset reads before U's fill)
    win_sweep<true, WD, false, KU>(len, w0, Uwoff, Urec, Utinv, ys, part, lane, q, nullptr, nullptr, lwo);
    __syncthreads();
    for (int64_t t = threadIdx.x; t < len; t += 256) y[b0 + t] = ys[t];
}

int ilu_window_max_rows() { return 163840 / 8 - 512 - 64; }  // LDS: partial sums, t, the block, a dummy slot per lane
static_assert((163840 / 8 - 512 - 64 + 63) / 64 + 1 <= 64 * WIN_OFFR, "window offsets exceed WinOff's registers");
int ilu_window_ring_rows() { return WIN_RING; }
int64_t ilu_window_ring_max_rows() { return (int64_t)(64 * WIN_OFFR_RING - 1) * 64; }
static_assert(1600 + WIN_RING + 64 <= 163840 / 8, "the ring exceeds LDS");
static_assert(64 * WIN_OFFR_RING <= 1024, "the ring variant's window offsets exceed their LDS slots");
int ilu_window_stream_pad() { return 0; }
int ilu_window_max_entries() { return WIN_KP; }

template <int KL, int KU>
static void window_launch(int64_t n, int64_t nblocks, const int64_t *bstart, const int64_t *wstart,
                          const int64_t *Lwoff, const int32_t *Lrec, const double *Ltinv, const int64_t *Uwoff,
                          const int32_t *Urec, const double *Utinv, const double *x, double *y, int64_t max_len,
                          hipStream_t st, int depth, bool ring, int tri) {
    static bool configured = false;
    if (!configured) {
        for (const void *k : {(const void *)k_ilu_blocks_window<2, false, KL, KU>,
                              (const void *)k_ilu_blocks_window<3, false, KL, KU>,
                              (const void *)k_ilu_blocks_window<2, true, KL, KU>})
            (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)163840);
        configured = true;
    }
    if (ring) {  // (x may be y: a window's input rows are read before its solution is stored)
        const size_t bytes = (size_t)(1600 + WIN_RING + 64) * 8;
        k_ilu_blocks_window<2, true, KL, KU><<<(unsigned)nblocks, 256, bytes, st>>>(
            n, nblocks, bstart, wstart, Lwoff, Lrec, Ltinv, Uwoff, Urec, Utinv, x, y, tri, 0);
        return;
    }
    size_t bytes = (size_t)(512 + std::max<int64_t>(max_len, 1) + 64) * 8;  // + a dummy slot per lane
    const size_t obytes = (size_t)((std::max<int64_t>(max_len, 1) + 63) / 64 + 1) * 8;  // the window offsets
    const int lwo_ok = bytes + obytes <= 163840 ? 1 : 0;
    if (lwo_ok) bytes += obytes;
    if (depth == 3)
        k_ilu_blocks_window<3, false, KL, KU><<<(unsigned)nblocks, 256, bytes, st>>>(
            n, nblocks, bstart, wstart, Lwoff, Lrec, Ltinv, Uwoff, Urec, Utinv, x, y, 3, lwo_ok);
    else
        k_ilu_blocks_window<2, false, KL, KU><<<(unsigned)nblocks, 256, bytes, st>>>(
            n, nblocks, bstart, wstart, Lwoff, Lrec, Ltinv, Uwoff, Urec, Utinv, x, y, 3, lwo_ok);
}
int window_records(int max_entries) {  // stream records per wave and window: 4, 6 or 8
    return max_entries <= 4 * WIN_NW ? 4 : max_entries <= 6 * WIN_NW ? 6 : WIN_KPW;
}
template <int KL>
static void window_launch_u(int ku, int64_t n, int64_t nblocks, const int64_t *bstart, const int64_t *wstart,
                            const int64_t *Lwoff, const int32_t *Lrec, const double *Ltinv, const int64_t *Uwoff,
                            const int32_t *Urec, const double *Utinv, const double *x, double *y, int64_t max_len,
                            hipStream_t st, int depth, bool ring, int tri) {
    if (ku == 4)
        window_launch<KL, 4>(n, nblocks, bstart, wstart, Lwoff, Lrec, Ltinv, Uwoff, Urec, Utinv, x, y, max_len, st,
                             depth, ring, tri);
    else if (ku == 6)
        window_launch<KL, 6>(n, nblocks, bstart, wstart, Lwoff, Lrec, Ltinv, Uwoff, Urec, Utinv, x, y, max_len, st,
                             depth, ring, tri);
    else
        window_launch<KL, WIN_KPW>(n, nblocks, bstart, wstart, Lwoff, Lrec, Ltinv, Uwoff, Urec, Utinv, x, y, max_len,
                                   st, depth, ring, tri);
}
void launch_ilu_blocks_window(int64_t n, int64_t nblocks, const int64_t *bstart, const int64_t *wstart,
                              const int64_t *Lwoff, const int32_t *Lrec, const double *Ltinv, const int64_t *Uwoff,
                              const int32_t *Urec, const double *Utinv, const double *x, double *y, int64_t max_len,
                              hipStream_t st, int depth, bool ring, int tri, int max_entries_L, int max_entries_U) {
    const int kl = window_records(max_entries_L), ku = window_records(max_entries_U);
    if (kl == 4)
        window_launch_u<4>(ku, n, nblocks, bstart, wstart, Lwoff, Lrec, Ltinv, Uwoff, Urec, Utinv, x, y, max_len, st,
                           depth, ring, tri);
    else if (kl == 6)
        window_launch_u<6>(ku, n, nblocks, bstart, wstart, Lwoff, Lrec, Ltinv, Uwoff, Urec, Utinv, x, y, max_len, st,
                           depth, ring, tri);
    else
        window_launch_u<WIN_KPW>(ku, n, nblocks, bstart, wstart, Lwoff, Lrec, Ltinv, Uwoff, Urec, Utinv, x, y, max_len,
                                 st, depth, ring, tri);
}

// ======================================================= super-window sweep ==
// Triangular sweeps of blocks too long for LDS (whole FE blocks: ~47k rows at
// 3-D N=12, 353k at N=24, whose level DAGs are ~1,440 / ~2,985 levels deep).
// Rows are cut into windows of 64 (lane = row) and consecutive windows into
// super-windows (build_swin_tri): per super-window, in processing order,
//   1. all waves stage the super-window's packed window inverses and near
//      streams into LDS, and every row's input minus its far terms (entries
//      before the super-window, read from the block solution in global
//      memory -- final since earlier super-windows) goes to LDS;
//   2. one wave walks the windows: t = input - near terms (LDS gathers),
//      y = T_w^-1 t (a 64 x 64 triangular GEMV from LDS, t broadcast with
//      v_readlane), y to LDS -- no barrier between windows (a wave's LDS
//      accesses complete in order);
//   3. the super-window's y to global memory.
// The dependent chain is the windows' GEMVs (len / 64 per triangle) instead of
// the levels; no global load sits on it.  L: input x, output y; U: in place on
// y.  Sums: far terms, near terms (stream order), then the window inverse --
// the explicit inverses reassociate the substitution's sums (<= 1e-12 against
// the level-order sweeps, tests/test_gpu_sweeps.py).
static constexpr int SWIN_TPB = 256, SWIN_TRI = 2080;

// global -> LDS copies of the staged streams: 8 x 16 bytes in flight per thread
__device__ __forceinline__ void swin_copy(const double *__restrict__ src, double *dst, int64_t n, int tid) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const bool al = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    if (!al) {
        for (int64_t k = tid; k < n; k += SWIN_TPB) dst[k] = src[k];
        return;
    }
    const int64_t n2 = n >> 1;
    const d2 *s2 = reinterpret_cast<const d2 *>(src);
    d2 *t2 = reinterpret_cast<d2 *>(dst);
    for (int64_t k0 = 0; k0 < n2; k0 += 8 * SWIN_TPB) {
        d2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t k = k0 + u * SWIN_TPB + tid;
            v[u] = k < n2 ? s2[k] : d2{0.0, 0.0};
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t k = k0 + u * SWIN_TPB + tid;
            if (k < n2) t2[k] = v[u];
        }
    }
    if ((n & 1) && tid == 0) dst[n - 1] = src[n - 1];
}
__device__ __forceinline__ void swin_copy32(const int32_t *__restrict__ src, int32_t *dst, int64_t n, int tid) {
    for (int64_t k0 = 0; k0 < n; k0 += 8 * SWIN_TPB) {
        int32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t k = k0 + u * SWIN_TPB + tid;
            v[u] = k < n ? src[k] : 0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t k = k0 + u * SWIN_TPB + tid;
            if (k < n) dst[k] = v[u];
        }
    }
}

template <bool UP>
__device__ __forceinline__ void swin_sweep(int64_t len, int64_t bs0, int64_t bs1, const int64_t *__restrict__ sw,
                                           const int64_t *__restrict__ wnear, const int32_t *__restrict__ ncol,
                                           const double *__restrict__ nval, const int64_t *__restrict__ wfar,
                                           const int32_t *__restrict__ fcol, const double *__restrict__ fval,
                                           const double *__restrict__ tinv, int64_t wfirst, const double *in,
                                           double *out, double *lds) {
    double *ys = lds;            // the super-window's rows (<= 512)
    double *tb = lds + 512;      // the window's t, broadcast
    double *ts = lds + 576;      // staged inverses, then near values
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t s = bs0; s < bs1; ++s) {
        const int64_t w0 = sw[4 * s], nwn = sw[4 * s + 1], r0 = sw[4 * s + 2], r1 = sw[4 * s + 3];
        // 1. stage: inverses (nwn * 2080 doubles), near values and columns
        const int64_t nt = nwn * SWIN_TRI, e0 = wnear[w0], ne = wnear[w0 + nwn] - e0;
        double *nv = ts + nt;
        int32_t *nc = reinterpret_cast<int32_t *>(nv + ne);
        // (eight 16-byte loads in flight per thread, then their LDS stores: the copies
        // are latency-bound, one round trip per round)
        swin_copy(reinterpret_cast<const double *>(tinv) + w0 * SWIN_TRI, ts, nt, tid);
        swin_copy(nval + e0, nv, ne, tid);
        swin_copy32(ncol + e0, nc, ne, tid);
        // far terms: one row per thread (64-row slices: [k][lane] streams), eight gathers in flight
        for (int64_t r = r0 + tid; r < r1; r += SWIN_TPB) {
            const int64_t w = wfirst + (r >> 6), l = r & 63;
            const int64_t f0 = wfar[w], K = (wfar[w + 1] - f0) >> 6;
            double acc = 0.0;
            const double xin = in[r];
            for (int64_t k = 0; k < K; k += 8) {
                int32_t cc[8];
                double vv[8], yy[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int64_t kk = k + u < K ? k + u : K - 1;  // (clamped: the value is zeroed below)
                    cc[u] = fcol[f0 + kk * 64 + l];
                    vv[u] = fval[f0 + kk * 64 + l];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) yy[u] = out[cc[u]];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += __dmul_rn(k + u < K ? vv[u] : 0.0, yy[u]);
            }
            ys[r - r0] = xin - acc;
        }
        __syncthreads();
        // 2. the windows, one wave
        if (wave == 0) {
            for (int64_t j0 = 0; j0 < nwn; ++j0) {
                const int64_t j = UP ? nwn - 1 - j0 : j0;
                const int64_t w = w0 + j, wr = (w - wfirst) * 64;  // window's first row (block-local)
                const bool act = wr + lane < len;
                const int64_t q0 = wnear[w] - e0, K = (wnear[w + 1] - wnear[w]) >> 6;
                // near terms, eight at a time: their column / value reads, then the
                // eight y gathers, all issued before the first is used (branch-free:
                // padding and the tail read entry 0 with value 0)
                double acc = 0.0;
                for (int64_t k0 = 0; k0 < K; k0 += 8) {
                    int32_t cc[8];
                    double vv[8], yy[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int64_t q = q0 + (k0 + u < K ? k0 + u : 0) * 64 + lane;
                        cc[u] = nc[q];
                        vv[u] = k0 + u < K ? nv[q] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) yy[u] = ys[cc[u]];
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc += __dmul_rn(vv[u], yy[u]);
                }
                const double t = act ? ys[wr - r0 + lane] - acc : 0.0;
                tb[lane] = t;  // broadcast through LDS (one wave: in order, no barrier)
                const double *T = ts + j * SWIN_TRI;
                // y = T^-1 t: 16 columns per step, their LDS reads (T column entries and
                // the broadcast t_k) issued together; four partial sums (k mod 4) added
                // in a fixed order
                double ya[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k0 = 0; k0 < 64; k0 += 16) {
                    double a[16], tk[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        const int k = k0 + u;
                        const bool nz = UP ? lane <= k : lane >= k;
                        const int off = UP ? k * (k + 1) / 2 + lane : 64 * k - k * (k - 1) / 2 + (lane - k);
                        a[u] = T[nz ? off : 0];
                        tk[u] = tb[k];
                    }
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        const int k = k0 + u;
                        const bool nz = UP ? lane <= k : lane >= k;
                        ya[u & 3] = __fma_rn(nz ? a[u] : 0.0, tk[u], ya[u & 3]);
                    }
                }
                const double y = (ya[0] + ya[1]) + (ya[2] + ya[3]);
                if (act) ys[wr - r0 + lane] = y;
            }
        }
        __syncthreads();
        // 3. the super-window's solution to global memory (far terms of later super-windows read it)
        for (int64_t r = r0 + tid; r < r1; r += SWIN_TPB) out[r] = ys[r - r0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(SWIN_TPB) void k_ilu_blocks_swin(
    int64_t n, int64_t nblocks, const int64_t *__restrict__ bstart, const int64_t *__restrict__ wstart,
    const int64_t *__restrict__ Lbsw, const int64_t *__restrict__ Lsw, const int64_t *__restrict__ Lwnear,
    const int32_t *__restrict__ Lncol, const double *__restrict__ Lnval, const int64_t *__restrict__ Lwfar,
    const int32_t *__restrict__ Lfcol, const double *__restrict__ Lfval, const double *__restrict__ Ltinv,
    const int64_t *__restrict__ Ubsw, const int64_t *__restrict__ Usw, const int64_t *__restrict__ Uwnear,
    const int32_t *__restrict__ Uncol, const double *__restrict__ Unval, const int64_t *__restrict__ Uwfar,
    const int32_t *__restrict__ Ufcol, const double *__restrict__ Ufval, const double *__restrict__ Utinv,
    const double *x, double *y) {
    extern __shared__ __attribute__((aligned(16))) double lds_sw[];
    const int64_t blk = nblocks - 1 - (int64_t)blockIdx.x;
    int64_t b0, len;
    block_range(blk, n, nblocks, bstart, b0, len);
    const int64_t wf = wstart[blk];
    swin_sweep<false>(len, Lbsw[blk], Lbsw[blk + 1], Lsw, Lwnear, Lncol, Lnval, Lwfar, Lfcol + 0, Lfval, Ltinv, wf,
                      x + b0, y + b0, lds_sw);
    swin_sweep<true>(len, Ubsw[blk], Ubsw[blk + 1], Usw, Uwnear, Uncol, Unval, Uwfar, Ufcol, Ufval, Utinv, wf, y + b0,
                     y + b0, lds_sw);
}

int ilu_swin_lds_budget() { return 163840 - 576 * 8 - 1024; }

void launch_ilu_blocks_swin(int64_t n, int64_t nblocks, const int64_t *bstart, const int64_t *wstart,
                            const int64_t *Lbsw, const int64_t *Lsw, const int64_t *Lwnear, const int32_t *Lncol,
                            const double *Lnval, const int64_t *Lwfar, const int32_t *Lfcol, const double *Lfval,
                            const double *Ltinv, const int64_t *Ubsw, const int64_t *Usw, const int64_t *Uwnear,
                            const int32_t *Uncol, const double *Unval, const int64_t *Uwfar, const int32_t *Ufcol,
                            const double *Ufval, const double *Utinv, const double *x, double *y, int64_t lds_bytes,
                            hipStream_t st) {
    static bool configured = false;
    if (!configured) {
        (void)hipFuncSetAttribute((const void *)k_ilu_blocks_swin, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)163840);
        configured = true;
    }
    k_ilu_blocks_swin<<<(unsigned)nblocks, SWIN_TPB, (size_t)lds_bytes, st>>>(
        n, nblocks, bstart, wstart, Lbsw, Lsw, Lwnear, Lncol, Lnval, Lwfar, Lfcol, Lfval, Ltinv, Ubsw, Usw, Uwnear,
        Uncol, Unval, Uwfar, Ufcol, Ufval, Utinv, x, y);
}

// =========================================================== distribution ====
// flag[c] = 1 for every column c (relative to the column space) of the matrix
// that this rank does not own (own[c] < 0)
__global__ __launch_bounds__(TPB) void k_flag_ghosts(int64_t nnz, const int32_t *ci, const int32_t *own, uint8_t *flag) {
    for (int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * TPB) {
        const int32_t c = ci[k];
        if (own[c] < 0) flag[c] = 1;
    }
}
__global__ __launch_bounds__(TPB) void k_remap_cols(int64_t nnz, int32_t *ci, const int32_t *gmap) {
    for (int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * TPB)
        ci[k] = gmap[ci[k]];
}
__global__ __launch_bounds__(TPB) void k_pack(int64_t m, const int32_t *idx, const double *x, double *buf) {
    const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (k < m) buf[k] = x[idx[k]];
}
void launch_flag_ghosts(int64_t nnz, const int32_t *ci, const int32_t *own, uint8_t *flag, hipStream_t st) {
    if (nnz > 0) k_flag_ghosts<<<stream_grid(nnz), TPB, 0, st>>>(nnz, ci, own, flag);
}
void launch_remap_cols(int64_t nnz, int32_t *ci, const int32_t *gmap, hipStream_t st) {
    if (nnz > 0) k_remap_cols<<<stream_grid(nnz), TPB, 0, st>>>(nnz, ci, gmap);
}
// Remapped rows are sorted runs (owned columns in order, ghosts per owner and
// field in order) -> restore ascending columns; one thread per row, insertion
// sort (setup only; every consumer -- window extraction, diagonal search, ILU
// pattern matching -- binary-searches sorted rows).
__global__ __launch_bounds__(TPB) void k_sort_rows(int64_t n, const int64_t *rp, int32_t *ci, double *val) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int64_t s = rp[i], e = rp[i + 1];
    for (int64_t k = s + 1; k < e; ++k) {
        const int32_t c = ci[k];
        const double v = val[k];
        int64_t j = k - 1;
        while (j >= s && ci[j] > c) {
            ci[j + 1] = ci[j];
            val[j + 1] = val[j];
            --j;
        }
        ci[j + 1] = c;
        val[j + 1] = v;
    }
}
void launch_sort_rows(int64_t n, const int64_t *rp, int32_t *ci, double *val, hipStream_t st) {
    if (n > 0) k_sort_rows<<<grid_for(n, TPB), TPB, 0, st>>>(n, rp, ci, val);
}
__global__ __launch_bounds__(TPB) void k_unpack(int64_t m, const int32_t *idx, const double *buf, double *x) {
    const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (k < m) x[idx[k]] = buf[k];
}
void launch_unpack(int64_t m, const int32_t *idx, const double *buf, double *x, hipStream_t st) {
    if (m > 0) k_unpack<<<grid_for(m, TPB), TPB, 0, st>>>(m, idx, buf, x);
}
void launch_pack(int64_t m, const int32_t *idx, const double *x, double *buf, hipStream_t st) {
    if (m > 0) k_pack<<<grid_for(m, TPB), TPB, 0, st>>>(m, idx, x, buf);
}

}  // namespace pls
