// asm.hip -- overlapping additive Schwarz (pc_type asm): subdomain growth, the extended
// block-diagonal matrix and the gather / combine of the application (asm.cpp: PCASM).
//
// Subdomains (MatIncreaseOverlap_SeqAIJ on bjacobi's contiguous ranges): k rounds, each adding
// every column index stored in the rows the previous round added.  One workgroup per block, at
// most ASM_GROW_GRID of them, each with three n-bit bitmaps in global memory: `in` (the set),
// `front` (the rows the previous round added) and `next` (the rows this round adds).  A round
// walks the front rows' column lists, one wave per bitmap word, and sets bits with atomicOr; the
// bit that was clear before goes into `next`.  The final set is read off `in` in index order
// (popcount + prefix over the words), so it comes out sorted and the same on every run whatever
// order the atomics landed in.  A workgroup touches only its own bitmaps and clears the words it
// used before it takes its next block: no kernel here waits on another workgroup.  The kernel
// runs twice: once to count |I_b|, once (after the scan) to write the rows.
//
// Rows and extended positions are 32-bit; offsets into the matrices are 64-bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace pls {

static constexpr int TPB = 256;
static constexpr int GROW_TPB = 1024;
static inline unsigned blocks_for(int64_t work, int per_block) {
    const int64_t g = (work + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g);
}
int asm_grow_grid() { return ASM_GROW_GRID; }

// bjacobi's sizes rule: block b owns [lo, hi)
__device__ __forceinline__ void asm_owned(int64_t b, int64_t n, int64_t nb, int64_t &lo, int64_t &hi) {
    const int64_t q = n / nb, r = n % nb;
    lo = b * q + (b < r ? b : r);
    hi = lo + q + (b < r ? 1 : 0);
}

// exclusive prefix of v over the workgroup (GROW_TPB threads), total in *tot; wsum: 17 ints of LDS
__device__ __forceinline__ int asm_block_scan(int v, int *wsum, int *tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    __syncthreads();  // (wsum of the previous call has been read)
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, all = 0;
    for (int w = 0; w < GROW_TPB / 64; ++w) {
        const int s = wsum[w];
        if (w < wave) base += s;
        all += s;
    }
    *tot = all;
    return base + inc - v;
}

// FILL false: cnt[b] = |I_b|.  FILL true: rows[ptr[b] ..] = I_b ascending, own = 1 on the rows of [lo, hi).
// bits: gridDim.x x 3 x nw words, zero on entry and on exit.
template <bool FILL>
__global__ __launch_bounds__(GROW_TPB) void k_asm_grow(int64_t n, int64_t nb, int overlap, const int64_t *__restrict__ rp,
                                                       const int32_t *__restrict__ ci, unsigned *bits, int64_t nw,
                                                       int64_t *__restrict__ cnt, const int64_t *__restrict__ ptr,
                                                       int32_t *__restrict__ rows, uint8_t *__restrict__ own) {
    __shared__ int s_lo, s_hi, s_new, wsum[GROW_TPB / 64 + 1];
    unsigned *in = bits + (size_t)blockIdx.x * 3 * nw, *front = in + nw, *next = front + nw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
        int64_t lo, hi;
        asm_owned(b, n, nb, lo, hi);
        const int w0 = (int)(lo >> 5), w1 = (int)((hi - 1) >> 5) + 1;  // owned words [w0, w1) (hi > lo: nb <= n)
        if (threadIdx.x == 0) {
            s_lo = w0;
            s_hi = w1;
        }
        for (int w = w0 + threadIdx.x; w < w1; w += GROW_TPB) {
            const int64_t r0 = (int64_t)w << 5;
            unsigned m = 0xFFFFFFFFu;
            if (r0 < lo) m &= 0xFFFFFFFFu << (int)(lo - r0);
            if (r0 + 32 > hi) m &= 0xFFFFFFFFu >> (int)(r0 + 32 - hi);
            in[w] = m;
            front[w] = m;
        }
        __syncthreads();
        for (int round = 0; round < overlap; ++round) {
            const int f0 = s_lo, f1 = s_hi;  // the front lies inside the words touched so far
            __syncthreads();                 // (read before anybody widens them)
            if (threadIdx.x == 0) s_new = 0;
            __syncthreads();
            for (int w = f0 + wave; w < f1; w += GROW_TPB / 64) {
                unsigned f = front[w];  // written by this workgroup before the barrier
                while (f) {
                    const int bit = __ffs(f) - 1;
                    f &= f - 1;
                    const int64_t r = ((int64_t)w << 5) + bit;
                    for (int64_t e = rp[r] + lane; e < rp[r + 1]; e += 64) {
                        const int32_t j = ci[e];
                        if (j >= lo && j < hi) continue;  // owned: set from the start
                        if (j < 0 || j >= n) continue;    // (a square block has none)
                        const unsigned m = 1u << (j & 31);
                        const unsigned old = atomicOr(&in[j >> 5], m);
                        if (!(old & m)) {
                            atomicOr(&next[j >> 5], m);
                            atomicMin(&s_lo, j >> 5);
                            atomicMax(&s_hi, (j >> 5) + 1);
                            s_new = 1;
                        }
                    }
                }
            }
            __syncthreads();
            const int g0 = s_lo, g1 = s_hi, any = s_new;
            // (atomics on `next` went to L2; read them there, not from this CU's L1)
            for (int w = g0 + threadIdx.x; w < g1; w += GROW_TPB) {
                front[w] = __hip_atomic_load(&next[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                next[w] = 0;
            }
            __syncthreads();
            if (!any) break;
        }
        // read the set off in index order
        const int g0 = s_lo, g1 = s_hi;
        int64_t base = FILL ? ptr[b] : 0;
        for (int c0 = g0; c0 < g1; c0 += GROW_TPB) {
            const int w = c0 + threadIdx.x;
            unsigned m = w < g1 ? __hip_atomic_load(&in[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            int tot;
            const int pre = asm_block_scan(__popc(m), wsum, &tot);
            if (FILL) {
                int64_t o = base + pre;
                while (m) {
                    const int bit = __ffs(m) - 1;
                    m &= m - 1;
                    const int64_t r = ((int64_t)w << 5) + bit;
                    rows[o] = (int32_t)r;
                    own[o] = (r >= lo && r < hi) ? 1 : 0;
                    ++o;
                }
            }
            base += tot;
        }
        if (!FILL && threadIdx.x == 0) cnt[b] = base;
        for (int w = g0 + threadIdx.x; w < g1; w += GROW_TPB) {
            in[w] = 0;
            front[w] = 0;
        }
        __syncthreads();
    }
}

void launch_asm_grow(bool fill, int grid, int64_t n, int64_t nb, int overlap, const int64_t *rp, const int32_t *ci,
                     unsigned *bits, int64_t nw, int64_t *cnt, const int64_t *ptr, int32_t *rows, uint8_t *own,
                     hipStream_t st) {
    if (n <= 0 || nb <= 0 || grid <= 0) return;
    if (fill) k_asm_grow<true><<<grid, GROW_TPB, 0, st>>>(n, nb, overlap, rp, ci, bits, nw, cnt, ptr, rows, own);
    else k_asm_grow<false><<<grid, GROW_TPB, 0, st>>>(n, nb, overlap, rp, ci, bits, nw, cnt, ptr, rows, own);
}

// ------------------------------------------------------- extended matrix ----
// the block of extended position e: the last b with ptr[b] <= e
__device__ __forceinline__ int64_t asm_block_of(const int64_t *__restrict__ ptr, int64_t nb, int64_t e) {
    int64_t a = 0, z = nb;  // ptr[a] <= e < ptr[z]
    while (z - a > 1) {
        const int64_t m = (a + z) >> 1;
        if (ptr[m] <= e) a = m;
        else z = m;
    }
    return a;
}
// position of global row j in the sorted segment rows[s0, s1), or -1
__device__ __forceinline__ int64_t asm_find(const int32_t *__restrict__ rows, int64_t s0, int64_t s1, int32_t j) {
    int64_t a = s0, z = s1;
    while (a < z) {
        const int64_t m = (a + z) >> 1;
        if (rows[m] < j) a = m + 1;
        else z = m;
    }
    return (a < s1 && rows[a] == j) ? a : -1;
}

// E's rows, 16 lanes each: the entries of M's row rows[e] whose column is in the block's set, renumbered to
// extended positions.  The set is sorted, so the renumbering keeps the columns ascending; the 16-lane
// ballot keeps them in place.  FILL false: len[e] only.
template <bool FILL>
__global__ __launch_bounds__(TPB) void k_asm_extend(int64_t ne, int64_t n, int64_t nb, const int64_t *__restrict__ ptr,
                                                    const int32_t *__restrict__ rows, const int64_t *__restrict__ rp,
                                                    const int32_t *__restrict__ ci, const double *__restrict__ val,
                                                    int64_t *__restrict__ len, const int64_t *__restrict__ erp,
                                                    int32_t *__restrict__ eci, double *__restrict__ eval) {
    const int64_t e = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15, sh = (threadIdx.x & 63) & ~15;
    if (e >= ne) return;  // (whole 16-lane groups leave together)
    const int64_t b = asm_block_of(ptr, nb, e), s0 = ptr[b], s1 = ptr[b + 1];
    const int64_t r = rows[e], k0 = rp[r], k1 = rp[r + 1];
    // the owned range [lo, hi) is contiguous in the sorted set, from position plo: no search for its columns
    int64_t lo, hi;
    asm_owned(b, n, nb, lo, hi);
    int64_t plo = s0, z = s1;
    while (plo < z) {
        const int64_t m = (plo + z) >> 1;
        if (rows[m] < lo) plo = m + 1;
        else z = m;
    }
    int64_t out = FILL ? erp[e] : 0;
    for (int64_t k = k0; k < k1; k += 16) {  // (the same trip count on the group's 16 lanes)
        const bool have = k + l < k1;
        const int32_t j = have ? ci[k + l] : -1;
        const int64_t p = !have            ? -1
                          : j < lo         ? asm_find(rows, s0, plo, j)
                          : j < hi         ? plo + (j - lo)
                                           : asm_find(rows, plo + (hi - lo), s1, j);
        const unsigned g = (unsigned)((__ballot(p >= 0) >> sh) & 0xFFFFull);
        if (FILL && p >= 0) {
            const int64_t o = out + __popc(g & ((1u << l) - 1u));
            eci[o] = (int32_t)p;
            eval[o] = val[k + l];
        }
        out += __popc(g);
    }
    if (!FILL && l == 0) len[e] = out;
}
void launch_asm_extend(bool fill, int64_t ne, int64_t n, int64_t nb, const int64_t *ptr, const int32_t *rows, const int64_t *rp,
                       const int32_t *ci, const double *val, int64_t *len, const int64_t *erp, int32_t *eci,
                       double *eval, hipStream_t st) {
    if (ne <= 0) return;
    if (fill)
        k_asm_extend<true><<<blocks_for(ne * 16, TPB), TPB, 0, st>>>(ne, n, nb, ptr, rows, rp, ci, val, len, erp, eci,
                                                                     eval);
    else
        k_asm_extend<false><<<blocks_for(ne * 16, TPB), TPB, 0, st>>>(ne, n, nb, ptr, rows, rp, ci, val, len, erp, eci,
                                                                     eval);
}

// ---------------------------------------------------------- transpose map ----
// per global row its extended positions, ascending (= ascending block order): count, scan, fill
// through cursors, then each row's few positions sorted by one thread; opos[r]: the owned one
__global__ __launch_bounds__(TPB) void k_asm_tcount(int64_t ne, const int32_t *__restrict__ rows,
                                                    const uint8_t *__restrict__ own, int64_t *cnt,
                                                    int32_t *__restrict__ opos) {
    const int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= ne) return;
    atomicAdd((unsigned long long *)&cnt[rows[e]], 1ull);
    if (own[e]) opos[rows[e]] = (int32_t)e;  // (every global row has exactly one owner)
}
__global__ __launch_bounds__(TPB) void k_asm_tfill(int64_t ne, const int32_t *__restrict__ rows,
                                                   const int64_t *__restrict__ tptr, int32_t *cursor,
                                                   int32_t *__restrict__ tpos) {
    const int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= ne) return;
    const int32_t r = rows[e];
    tpos[tptr[r] + atomicAdd(&cursor[r], 1)] = (int32_t)e;
}
__global__ __launch_bounds__(TPB) void k_asm_tsort(int64_t n, const int64_t *__restrict__ tptr, int32_t *tpos) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= n) return;
    const int64_t a = tptr[r], z = tptr[r + 1];
    for (int64_t i = a + 1; i < z; ++i) {  // insertion sort: a row lies in a handful of subdomains
        const int32_t v = tpos[i];
        int64_t j = i;
        for (; j > a && tpos[j - 1] > v; --j) tpos[j] = tpos[j - 1];
        tpos[j] = v;
    }
}
void launch_asm_transpose_count(int64_t ne, const int32_t *rows, const uint8_t *own, int64_t *cnt, int32_t *opos,
                                hipStream_t st) {
    if (ne > 0) k_asm_tcount<<<blocks_for(ne, TPB), TPB, 0, st>>>(ne, rows, own, cnt, opos);
}
void launch_asm_transpose_fill(int64_t ne, int64_t n, const int32_t *rows, const int64_t *tptr, int32_t *cursor,
                               int32_t *tpos, hipStream_t st) {
    if (ne <= 0) return;
    k_asm_tfill<<<blocks_for(ne, TPB), TPB, 0, st>>>(ne, rows, tptr, cursor, tpos);
    k_asm_tsort<<<blocks_for(n, TPB), TPB, 0, st>>>(n, tptr, tpos);
}

// ------------------------------------------------------------ application ----
// x_ext[e] = x[gidx[e]], 0.0 where the type masks the input and the row is not owned
__global__ __launch_bounds__(TPB) void k_asm_gather(int64_t ne, const int32_t *__restrict__ gidx,
                                                    const uint8_t *__restrict__ own, int mask_in,
                                                    const double *__restrict__ x, double *__restrict__ xe) {
    const int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= ne) return;
    xe[e] = (mask_in && !own[e]) ? 0.0 : x[gidx[e]];
}
// y[r]: the owned position's value (restrict, none), or the sum from 0.0 over the row's positions in
// ascending block order (basic, interpolate) -- one thread per row, a fixed order: the same bits every run
__global__ __launch_bounds__(TPB) void k_asm_combine(int64_t n, int mask_out, const int32_t *__restrict__ opos,
                                                     const int64_t *__restrict__ tptr,
                                                     const int32_t *__restrict__ tpos, const double *__restrict__ ye,
                                                     double *__restrict__ y) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= n) return;
    if (mask_out) {
        y[r] = ye[opos[r]];
        return;
    }
    double s = 0.0;
    for (int64_t k = tptr[r]; k < tptr[r + 1]; ++k) s += ye[tpos[k]];
    y[r] = s;
}
void launch_asm_gather(int64_t ne, const int32_t *gidx, const uint8_t *own, int mask_in, const double *x, double *xe,
                       hipStream_t st) {
    if (ne > 0) k_asm_gather<<<blocks_for(ne, TPB), TPB, 0, st>>>(ne, gidx, own, mask_in, x, xe);
}
void launch_asm_combine(int64_t n, int mask_out, const int32_t *opos, const int64_t *tptr, const int32_t *tpos,
                        const double *ye, double *y, hipStream_t st) {
    if (n > 0) k_asm_combine<<<blocks_for(n, TPB), TPB, 0, st>>>(n, mask_out, opos, tptr, tpos, ye, y);
}

}  // namespace pls
