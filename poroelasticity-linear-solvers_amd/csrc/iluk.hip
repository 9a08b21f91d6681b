// iluk.hip -- symbolic phase of ILU(k) (pc_factor_levels > 0) on the device.
//
// PETSc's definition (MatILUFactorSymbolic_SeqAIJ, natural ordering, sum rule): stored entries
// have level 0, lev(i, j) = min over pivots p < min(i, j) of lev(i, p) + lev(p, j) + 1, and an
// entry is kept when lev <= k.  By the fill-path characterisation (Rose & Tarjan; Hysom & Pothen
// 2001) lev(i, j) + 1 is the length of the shortest path i -> j in G(A) whose intermediate
// vertices are all < min(i, j), which makes the rows independent:
//
//   U part of row i   breadth-first search from i in G(A) that expands only vertices < i, to
//                     depth k + 1; every vertex t > i it reaches is an entry (i, t)
//   L part            the same search from j in G(A^T) yields the rows i > j of column j (the
//                     bound "intermediates < j" belongs to the target, so one search on G(A)
//                     cannot give a row's L part); scattered to the rows through per-row cursors
//
// One wave (one 64-thread workgroup) per search.  The visited set is an open-addressing hash
// table in LDS, and the entries are read off the table when the search has ended, so a search
// that outgrows the table (more than slots / 2 vertices) has written nothing: its row goes to
// a list, and a second launch runs the listed rows with tables in global memory.  Two passes:
// the first counts (row lengths -> exclusive scan), the second fills; the rows are then sorted
// ascending (bitonic in LDS), which every consumer of the CSR assumes.  No kernel here waits on
// another workgroup.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "kernels.hpp"

namespace pls {

static constexpr int TPB = 256;
static inline unsigned blocks_for(int64_t work, int per_block) {
    const int64_t g = (work + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g);
}

// ----------------------------------------------------- pattern transpose ----
// Column counts and the (unsorted) transposed pattern: the searches need adjacency lists only.
__global__ __launch_bounds__(TPB) void k_iluk_tcount(int64_t n, const int64_t *rp, const int32_t *ci, int64_t *cnt) {
    const int64_t r = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    if (r >= n) return;
    for (int64_t e = rp[r] + l; e < rp[r + 1]; e += 16) atomicAdd((unsigned long long *)&cnt[ci[e]], 1ull);
}
__global__ __launch_bounds__(TPB) void k_iluk_tfill(int64_t n, const int64_t *rp, const int32_t *ci,
                                                    const int64_t *trp, int32_t *cursor, int32_t *tci) {
    const int64_t r = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    if (r >= n) return;
    for (int64_t e = rp[r] + l; e < rp[r + 1]; e += 16) {
        const int32_t j = ci[e];
        tci[trp[j] + atomicAdd(&cursor[j], 1)] = (int32_t)r;
    }
}
void launch_iluk_transpose_count(int64_t n, const int64_t *rp, const int32_t *ci, int64_t *cnt, hipStream_t st) {
    if (n > 0) k_iluk_tcount<<<blocks_for(n * 16, TPB), TPB, 0, st>>>(n, rp, ci, cnt);
}
void launch_iluk_transpose_fill(int64_t n, const int64_t *rp, const int32_t *ci, const int64_t *trp, int32_t *cursor,
                                int32_t *tci, hipStream_t st) {
    if (n > 0) k_iluk_tfill<<<blocks_for(n * 16, TPB), TPB, 0, st>>>(n, rp, ci, trp, cursor, tci);
}

// ---------------------------------------------------------------- search ----
// ints of one search's table and queue (the queue holds at most slots / 2 vertices)
__host__ __device__ static inline int64_t iluk_table_ints(int slots) { return (int64_t)slots + slots / 2 + 64; }
int64_t iluk_search_table_ints(int slots) { return iluk_table_ints(slots); }

__device__ __forceinline__ unsigned iluk_hash(int32_t t, int bits) { return ((uint32_t)t * 2654435761u) >> (32 - bits); }

// One search by one wave; tab (slots) and q (slots / 2 + 64) in LDS or global memory, ctr in LDS.
// Returns false when the visited set outgrew the table (nothing emitted).
template <bool FILL>
__device__ __forceinline__ bool iluk_row(const IlukSearch &a, const int64_t i, int *tab, int *q, int *ctr) {
    const int lane = threadIdx.x;
    const int slots = 1 << a.slot_bits, mask = slots - 1, cap = slots >> 1;
    for (int s = lane; s < slots; s += 64) tab[s] = -1;
    __syncthreads();
    if (lane == 0) {
        tab[iluk_hash((int32_t)i, a.slot_bits)] = (int32_t)i;
        q[0] = (int32_t)i;
        ctr[0] = 1;  // queue tail
        ctr[1] = 1;  // vertices in the table
    }
    __syncthreads();
    int qs = 0, qe = 1;
    bool over = false;
    // the frontier [qs, qe) holds the vertices < i at depth d (i itself at depth 0)
    for (int d = 0; d <= a.levels && qs < qe && !over; ++d) {
        for (int f = qs; f < qe && !over; ++f) {
            const int64_t v = q[f];
            const int64_t e1 = a.rp[v + 1];
            for (int64_t e = a.rp[v]; e < e1; e += 64) {
                bool full = false;
                if (e + lane < e1) {
                    const int32_t t = a.ci[e + lane];
                    unsigned h = iluk_hash(t, a.slot_bits);
                    bool fresh = false;
                    for (;;) {  // ends: the table never holds more than cap + 64 < slots vertices
                        const int old = atomicCAS(&tab[h], -1, t);
                        if (old == -1) { fresh = true; break; }
                        if (old == t) break;
                        h = (h + 1) & mask;
                    }
                    if (fresh) {
                        if (atomicAdd(&ctr[1], 1) >= cap) full = true;
                        else if ((int64_t)t < i && d < a.levels) q[atomicAdd(&ctr[0], 1)] = t;
                    }
                }
                if (__ballot(full) != 0ull) {
                    over = true;
                    break;
                }
            }
        }
        __syncthreads();
        qs = qe;
        qe = ctr[0];
        __syncthreads();
    }
    if (over) return false;
    // the entries: every vertex > i in the table
    int64_t base = 0;
    if (FILL && !a.transposed) {
        const int64_t d = a.orp[i] + a.lcnt[i];
        if (lane == 0) a.oci[d] = (int32_t)i;
        base = d + 1;
    }
    int total = 0;
    for (int s0 = 0; s0 < slots; s0 += 64) {
        // (an atomic load: a table in global memory was written by atomics, past the CU's cache)
        const int32_t t = __hip_atomic_load(&tab[s0 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool keep = (int64_t)t > i;
        if (!a.transposed) {
            const unsigned long long m = __ballot(keep);
            if (FILL && keep) a.oci[base + total + __popcll(m & ((1ull << lane) - 1ull))] = t;
            total += __popcll(m);
        } else if (keep) {
            if (FILL) a.oci[a.orp[t] + atomicAdd(&a.cursor[t], 1)] = (int32_t)i;
            else atomicAdd(&a.lcnt[t], 1);
        }
    }
    if (!FILL && !a.transposed && lane == 0) a.ucnt[i] = total;
    return true;
}

// every row, tables in LDS; the count pass lists the rows whose search outgrew the table
template <bool FILL>
__global__ __launch_bounds__(64) void k_iluk_search(IlukSearch a) {
    extern __shared__ int iluk_lds[];
    __shared__ int ctr[2];
    const int64_t i = blockIdx.x;
    const bool ok = iluk_row<FILL>(a, i, iluk_lds, iluk_lds + (1 << a.slot_bits), ctr);
    if (!FILL && !ok && threadIdx.x == 0) a.ovf_rows[atomicAdd(a.ovf_n, 1)] = (int32_t)i;
}
// the listed rows, one table in global memory per workgroup; a search that outgrows this table
// too sets fail (the host refuses)
template <bool FILL>
__global__ __launch_bounds__(64) void k_iluk_search_gmem(IlukSearch a, int64_t nlist, int *gtab) {
    __shared__ int ctr[2];
    int *tab = gtab + (int64_t)blockIdx.x * iluk_table_ints(1 << a.slot_bits);
    for (int64_t r = blockIdx.x; r < nlist; r += gridDim.x) {
        const int64_t i = a.ovf_rows[r];
        if (!iluk_row<FILL>(a, i, tab, tab + (1 << a.slot_bits), ctr) && threadIdx.x == 0) atomicMax(a.fail, 1);
        __syncthreads();
    }
}

void launch_iluk_search(const IlukSearch &a, bool fill, hipStream_t st) {
    if (a.n <= 0) return;
    const size_t lds = sizeof(int) * (size_t)iluk_table_ints(1 << a.slot_bits);
    if (fill) k_iluk_search<true><<<(unsigned)a.n, 64, lds, st>>>(a);
    else k_iluk_search<false><<<(unsigned)a.n, 64, lds, st>>>(a);
}
void launch_iluk_search_gmem(const IlukSearch &a, bool fill, int64_t nlist, int grid, int *gtab, hipStream_t st) {
    if (nlist <= 0) return;
    if (fill) k_iluk_search_gmem<true><<<(unsigned)grid, 64, 0, st>>>(a, nlist, gtab);
    else k_iluk_search_gmem<false><<<(unsigned)grid, 64, 0, st>>>(a, nlist, gtab);
}

// --------------------------------------------------- lengths, sort, values ----
__global__ __launch_bounds__(TPB) void k_iluk_len(int64_t n, const int32_t *lcnt, const int32_t *ucnt, int64_t *len) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i > n) return;
    len[i] = i == n ? 0 : (int64_t)lcnt[i] + ucnt[i] + 1;
}
void launch_iluk_row_len(int64_t n, const int32_t *lcnt, const int32_t *ucnt, int64_t *len, hipStream_t st) {
    k_iluk_len<<<blocks_for(n + 1, TPB), TPB, 0, st>>>(n, lcnt, ucnt, len);
}

// one wave per row: bitonic sort of the row's columns in LDS (padded to a power of two with
// INT_MAX); fail |= 2 where a sorted row is not strictly ascending
__global__ __launch_bounds__(64) void k_iluk_sort(const int64_t *rp, int32_t *ci, int32_t *fail) {
    extern __shared__ int iluk_lds[];
    const int lane = threadIdx.x;
    const int64_t r0 = rp[blockIdx.x];
    const int len = (int)(rp[blockIdx.x + 1] - r0);
    if (len < 2) return;
    int P = 2;
    while (P < len) P <<= 1;
    for (int k = lane; k < P; k += 64) iluk_lds[k] = k < len ? ci[r0 + k] : INT_MAX;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = lane; x < P; x += 64) {
                const int y = x ^ j;
                if (y > x) {
                    const int a = iluk_lds[x], b = iluk_lds[y];
                    if ((a > b) == ((x & k) == 0)) {
                        iluk_lds[x] = b;
                        iluk_lds[y] = a;
                    }
                }
            }
            __syncthreads();
        }
    bool bad = false;
    for (int k = lane; k < len; k += 64) {
        const int v = iluk_lds[k];
        ci[r0 + k] = v;
        bad |= k + 1 < len && iluk_lds[k + 1] <= v;
    }
    if (bad) atomicOr(fail, 2);
}
void launch_iluk_sort_rows(int64_t n, const int64_t *rp, int32_t *ci, int64_t max_row, int32_t *fail, hipStream_t st) {
    if (n <= 0) return;
    int64_t P = 2;
    while (P < max_row) P <<= 1;
    k_iluk_sort<<<(unsigned)n, 64, sizeof(int) * (size_t)P, st>>>(rp, ci, fail);
}

// the block's values into the filled pattern (dval zeroed before): 16 lanes per source row, a
// binary search per entry; fail |= 4 where an entry has no place (cannot happen: level 0)
__global__ __launch_bounds__(TPB) void k_iluk_scatter(int64_t n, const int64_t *srp, const int32_t *sci,
                                                      const double *sval, const int64_t *drp, const int32_t *dci,
                                                      double *dval, int32_t *fail) {
    const int64_t r = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    if (r >= n) return;
    const int64_t d0 = drp[r], d1 = drp[r + 1];
    for (int64_t e = srp[r] + l; e < srp[r + 1]; e += 16) {
        const int32_t j = sci[e];
        int64_t lo = d0, hi = d1;
        while (lo < hi) {
            const int64_t m = (lo + hi) >> 1;
            if (dci[m] < j) lo = m + 1; else hi = m;
        }
        if (lo < d1 && dci[lo] == j) dval[lo] = sval[e];
        else atomicOr(fail, 4);
    }
}
void launch_iluk_scatter(int64_t n, const int64_t *srp, const int32_t *sci, const double *sval, const int64_t *drp,
                         const int32_t *dci, double *dval, int32_t *fail, hipStream_t st) {
    if (n > 0) k_iluk_scatter<<<blocks_for(n * 16, TPB), TPB, 0, st>>>(n, srp, sci, sval, drp, dci, dval, fail);
}

}  // namespace pls
