// ilu0.hip -- ILU(0): diagonal search, SGS factors, the numeric factorization, the level
// tables and the level-scheduled triangular sweeps.
//
// Design rule (cdna_hip_programming.md):
//  * the ILU(0) factor and sweeps are level scheduled; the triangular factors
//    are stored in level order so each level streams a contiguous slice.
//
// Contraction: contract(on), except the factorization (ilu0_row, k_ilu0_level, k_ilu0_dep),
// which is bracketed contract(off) so it rounds like the CPU restatement.
#include "devutil.hpp"

#pragma clang fp contract(on)

namespace pls {

// ================================================================ ILU(0) ===
__global__ __launch_bounds__(TPB) void k_find_diag(int64_t n, const int64_t *rp, const int32_t *ci,
                                                   int64_t *diag, int32_t *fail) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int64_t p = lower_bound_i32(ci, rp[i], rp[i + 1], i);
    if (p < rp[i + 1] && (int64_t)ci[p] == i) {
        diag[i] = p;
    } else {
        diag[i] = -1;
        atomicMax(fail, 1);
    }
}
void launch_find_diag(int64_t n, const int64_t *rp, const int32_t *ci, int64_t *diag, int32_t *fail,
                      hipStream_t st) {
    if (n > 0) k_find_diag<<<grid_for(n, TPB), TPB, 0, st>>>(n, rp, ci, diag, fail);
}

// Symmetric Gauss-Seidel factors (see kernels.hpp): 1/a_ii first, then every
// strict-lower entry a_ij -> a_ij * (1/a_jj), the multiplier the ILU(0) IKJ
// loop forms (k_ilu0_level: mult = a_ij * dinv[j]).
__global__ __launch_bounds__(TPB) void k_sgs_dinv(int64_t n, const double *lu, const int64_t *diag, double *dinv,
                                                  int32_t *fail) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const double d = lu[diag[i]];
    if (d == 0.0) {
        atomicMax(fail, 2);
        dinv[i] = 0.0;
    } else {
        dinv[i] = 1.0 / d;
    }
}
__global__ __launch_bounds__(TPB) void k_sgs_scale(int64_t n, const int64_t *rp, const int32_t *ci, double *lu,
                                                   const int64_t *diag, const double *dinv) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    for (int64_t k = rp[i]; k < diag[i]; ++k) lu[k] = lu[k] * dinv[ci[k]];
}
void launch_sgs_factor(int64_t n, const int64_t *rp, const int32_t *ci, double *lu, const int64_t *diag,
                       double *dinv, int32_t *fail, hipStream_t st) {
    if (n <= 0) return;
    k_sgs_dinv<<<grid_for(n, TPB), TPB, 0, st>>>(n, lu, diag, dinv, fail);
    k_sgs_scale<<<grid_for(n, TPB), TPB, 0, st>>>(n, rp, ci, lu, diag, dinv);
}

// ILU(0) numeric factorization, one workgroup (ILU0_TPB threads) per row.
// The row is staged in LDS (values, columns and a column -> position hash);
// the upper parts of its pivot rows (rows r of earlier levels, final) and
// their 1/u_rr are staged in LDS too, in segments of at most ILU0_STAGE
// entries -- all four waves' loads in flight at once -- and every staged
// entry's position in the row is resolved while staging (the hash probes do
// not depend on the elimination).  Wave 0 then runs the IKJ elimination over
// the row's strict-lower entries in column order with the next pivot's
// positions and values prefetched, so a pivot step is one LDS round trip
// (rv[t] and the entries it updates) plus the update.  A pivot whose upper
// part alone exceeds the stage reads global memory.  Same operations in the
// same order as the CPU restatement (no contraction): bitwise the same
// factors whatever the path.
// DEP (k_ilu0_dep): one persistent launch -- rows are drawn from a counter in
// level order and each waits for its pivot rows' completion flags.  Pivot
// data written by other workgroups is read with agent-coherent (sc1) loads
// and the row's results are written with agent-coherent stores, so neither
// side needs the L2 write-back / invalidate of a release / acquire fence
// (one per row measured ~1.8x slower rows: every row's fence emptied the
// XCD's L2 for all the others).
static constexpr int ILU0_TPB = 256;
static constexpr int ILU0_STAGE = 8192;  // staged upper-part entries per segment (96 KiB)
static constexpr int64_t ILU0_SPIN_MAX = 1ll << 24;  // dependency polls before a row gives up (never expected)
static constexpr int ILU0_LDS = 163840 - 512;         // dynamic LDS budget (beside ilu0_ctl, ilu0_cnt)
__shared__ int32_t ilu0_ctl[4];                       // [0] drawn row (DEP), [1] abort
__shared__ int32_t ilu0_cnt[64];                      // per pivot chunk: staging waves done (DEP)

template <bool COH>
__device__ __forceinline__ double ilu0_ld(const double *p) {
    if (COH)
        return __longlong_as_double((long long)__hip_atomic_load(
            reinterpret_cast<uint64_t *>(const_cast<double *>(p)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return *p;
}
template <bool COH>
__device__ __forceinline__ void ilu0_st(double *p, double v) {
    if (COH)
        __hip_atomic_store(reinterpret_cast<uint64_t *>(p), (uint64_t)__double_as_longlong(v), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    else
        *p = v;
}

// stage pivots [ta, tb)'s upper parts (entries so[t] - base ..): POS their
// positions in the row (sc), VAL their values (sv); eight loads per thread in
// flight, entry q's pivot found by binary search over so
template <bool COH, bool POS, bool VAL>
__device__ __forceinline__ void ilu0_stage_part(int ta, int tb, int base, int cnt, const int64_t *__restrict__ rp,
                                                const int32_t *__restrict__ ci, const double *lu, int len, int hbits,
                                                const int32_t *rc, const int32_t *so, const int64_t *su, int32_t *sc,
                                                double *sv, const int32_t *hk, const int32_t *hp, int wbase = 0,
                                                int tid_ = -1, int nthr = ILU0_TPB) {
    // (entry base + q is written at wbase + q; threads tid_ of nthr, default all)
    const int tid = tid_ < 0 ? (int)threadIdx.x : tid_;
    const uint32_t hmask = (1u << hbits) - 1;
    for (int q0 = 0; q0 < cnt; q0 += 8 * nthr) {
        int64_t src[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int q = base + q0 + u * nthr + tid;
            int lo = ta, hi = tb;  // last t with so[t] <= q
            while (hi - lo > 1) {
                const int m = (lo + hi) >> 1;
                if (so[m] <= q) lo = m; else hi = m;
            }
            src[u] = q < base + cnt ? su[lo] + (q - so[lo]) : su[ta];
        }
        int32_t cv[8];
        double vv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (POS) cv[u] = ci[src[u]];
            if (VAL) vv[u] = ilu0_ld<COH>(lu + src[u]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int q = q0 + u * nthr + tid;
            if (q < cnt) {
                if (POS) {  // the column's position in the row (len: not in the pattern)
                    const int32_t j = cv[u];
                    int lo = len;
                    if (hbits > 0) {
                        uint32_t h = ((uint32_t)j * 2654435761u) >> (32 - hbits);
                        int32_t key = hk[h];
                        while (key != j && key != -1) {
                            h = (h + 1) & hmask;
                            key = hk[h];
                        }
                        if (key == j) lo = hp[h];
                    } else {
                        int a = 0, b = len;
                        while (a < b) {
                            const int m = (a + b) >> 1;
                            if (rc[m] < j) a = m + 1; else b = m;
                        }
                        if (a < len && rc[a] == j) lo = a;
                    }
                    sc[wbase + q] = lo;
                }
                if (VAL) sv[wbase + q] = vv[u];
            }
        }
    }
}

#pragma clang fp contract(off)
// returns false when the launch aborts (DEP: a dependency wait exceeded its bound)
template <bool DEP>
__device__ __forceinline__ bool ilu0_row(int64_t i, const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                         double *lu, const int64_t *__restrict__ diag, double *dinv, int32_t *fail,
                                         int max_row, int stage, int hbits, char *smem, int32_t *done,
                                         int32_t *abortf) {
    const int tid = threadIdx.x, lane = tid & 63;
    const bool w0 = tid < 64;
    const int64_t s = rp[i], e = rp[i + 1];
    const int len = (int)(e - s);
    // LDS: row values [max_row] | staged values [stage] | row cols [max_row] | staged positions [stage]
    //      | per-pivot staged offsets [max_row + 1] | per-pivot 1/u_rr [max_row] | per-pivot first
    //      upper entry [max_row] | hash keys, positions [2^hbits each]
    // (stage == 0: no staged arrays -- every pivot goes through global memory
    // and reads 1/u_rr there -- so rows of up to ~13.6k entries fit, ilu0_max_row)
    double *rv = reinterpret_cast<double *>(smem);
    double *sv = rv + max_row;
    int32_t *rc = reinterpret_cast<int32_t *>(sv + stage);
    int32_t *sc = rc + max_row;
    int32_t *so = sc + stage;
    double *sd = reinterpret_cast<double *>(((uintptr_t)(so + max_row + 1) + 7) & ~(uintptr_t)7);
    int64_t *su = reinterpret_cast<int64_t *>(sd + max_row);
    int32_t *hk = stage > 0 ? reinterpret_cast<int32_t *>(su + max_row) : so;
    int32_t *hp = hk + (hbits > 0 ? 1 << hbits : 0);
    const uint32_t hmask = (1u << hbits) - 1;
    auto hslot = [&](int32_t c) { return ((uint32_t)c * 2654435761u) >> (32 - hbits); };
    for (int t = tid; t < len; t += ILU0_TPB) {
        rv[t] = lu[s + t];  // (the row's own entries: written by no other row)
        rc[t] = ci[s + t];
    }
    if (hbits > 0) {
        for (int h = tid; h <= (int)hmask; h += ILU0_TPB) hk[h] = -1;
        __syncthreads();
        for (int t = tid; t < len; t += ILU0_TPB) {
            const int32_t c = rc[t];
            uint32_t h = hslot(c);
            while (atomicCAS(&hk[h], -1, c) != -1) h = (h + 1) & hmask;
            hp[h] = t;
        }
    }
    __syncthreads();
    const int dl = (int)(diag[i] - s);
    // pivot t's upper part (row rc[t]) goes to so[t] .. so[t + 1] (wave 0 scans)
    if (w0 && stage > 0) {
        int total = 0;
        for (int t0 = 0; t0 < dl; t0 += 64) {
            const int t = t0 + lane;
            int cnt = 0;
            int64_t u0 = 0;
            if (t < dl) {
                const int64_t r = rc[t];
                u0 = diag[r] + 1;
                cnt = (int)(rp[r + 1] - u0);
            }
            int inc = cnt;  // inclusive wave scan
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(inc, o);
                if (lane >= o) inc += v;
            }
            if (t < dl) {
                so[t] = total + inc - cnt;
                su[t] = u0;
            }
            total += __shfl(inc, 63);
        }
        if (lane == 0) so[dl] = total;
    }
    __syncthreads();
    // the staged entries' positions depend on the pattern only: with one segment
    // they are resolved before the wait (DEP), off the dependency chain
    const bool pre = DEP && stage > 0 && so[dl] <= stage;
    if (pre) ilu0_stage_part<DEP, true, false>(0, dl, 0, so[dl], rp, ci, lu, len, hbits, rc, so, su, sc, sv, hk, hp);
    if (DEP) {  // every pivot row (an earlier level: already drawn) finished
        if (w0) {
            int ab = 0;
            for (int t0 = 0; t0 < dl && !ab; t0 += 64) {
                const int t = t0 + lane;
                const int32_t k = t < dl ? rc[t] : -1;
                bool ok = k < 0;
                for (int64_t spins = 0;; ++spins) {
                    // (only the flags not yet seen are polled: 64 scattered loads per poll from
                    // ~250 waiting rows measured ~30x slower staging for every row)
                    if (!ok) ok = __hip_atomic_load(done + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
                    if (__all(ok)) break;
                    if ((spins & 63) == 63 && __hip_atomic_load(abortf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                        ab = 1;
                        break;
                    }
                    if (spins > ILU0_SPIN_MAX) {  // report instead of hanging: every row then stops
                        if (lane == 0) {
                            atomicMax(fail, 3);
                            __hip_atomic_store(abortf, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                        ab = 1;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(4);
                }
            }
            if (lane == 0) ilu0_ctl[1] = ab;
        }
        __syncthreads();
        if (ilu0_ctl[1]) return false;
    }
    if (stage > 0)
        for (int t = tid; t < dl; t += ILU0_TPB) sd[t] = ilu0_ld<DEP>(dinv + rc[t]);
    __syncthreads();
    // pivots in segments [ta, tb) whose upper parts fit the stage together; a
    // pivot whose part alone does not (or no stage) goes through global memory
    for (int ta = 0; ta < dl;) {
        int tb = ta;
        const int base = stage > 0 ? so[ta] : 0;
        if (stage > 0) {  // the last tb with so[tb] - base <= stage
            int hi = dl;
            while (tb < hi) {
                const int m = (tb + hi + 1) >> 1;
                if (so[m] - base <= stage) tb = m; else hi = m - 1;
            }
        }
        if (tb > ta && pre) {
            // DEP, one segment: waves 1-3 stage the values chunk by chunk (CH pivots)
            // while wave 0 eliminates, waiting only for the chunk it needs next
            // (values ~5 us, elimination ~9 us per row: the row's time after its
            // pivots finish is the dependency chain's step)
            const int CH = dl > 512 ? (dl + 63) / 64 : 8, nch = (dl + CH - 1) / CH;
            if (tid < 64) ilu0_cnt[tid] = 0;
            __syncthreads();
            if (!w0) {
                for (int cc = 0; cc < nch; ++cc) {
                    const int t0 = cc * CH, t1 = min(dl, t0 + CH);
                    ilu0_stage_part<DEP, false, true>(t0, t1, so[t0], so[t1] - so[t0], rp, ci, lu, len, hbits, rc, so,
                                                      su, sc, sv, hk, hp, so[t0], tid - 64, ILU0_TPB - 64);
                    if (lane == 0) __hip_atomic_fetch_add(ilu0_cnt + cc, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            } else {
                auto wait_chunk = [&](int cc) {
                    for (int64_t spins = 0;
                         __hip_atomic_load(ilu0_cnt + cc, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) <
                         ILU0_TPB / 64 - 1;
                         ++spins) {
                        if (spins > ILU0_SPIN_MAX) {  // never expected: report, do not hang
                            if (lane == 0) atomicMax(fail, 3);
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                    }
                };
                // software pipeline: pivot t computes while pivot t + 1's first entries
                // and pivot t + 2's offsets are in flight; rv[t] and the first update
                // target are read first, so the chain waits for one LDS round trip
                wait_chunk(0);
                int kn = so[0] + lane, en = so[1];
                int lon = kn < en ? sc[kn] : len;
                double vn = kn < en ? sv[kn] : 0.0, dn = sd[0];
                int s2a = dl > 1 ? so[1] : 0, s2b = dl > 1 ? so[2] : 0;  // pivot t + 1's range (next)
                for (int t = 0; t < dl; ++t) {
                    const int lo0 = lon, kc = kn, ec = en;
                    const double v0 = vn, dc = dn;
                    const double pc = rv[t];
                    const double r0 = rv[lo0 < len ? lo0 : t];
                    if (t + 1 < dl) {
                        if ((t + 1) % CH == 0) wait_chunk((t + 1) / CH);
                        kn = s2a + lane;
                        en = s2b;
                        lon = kn < en ? sc[kn] : len;
                        vn = kn < en ? sv[kn] : 0.0;
                        dn = sd[t + 1];
                        s2a = s2b;
                        s2b = t + 3 <= dl ? so[t + 3] : s2b;
                    }
                    if (pc != 0.0) {
                        const double mult = pc * dc;
                        if (lane == 0) rv[t] = mult;
                        if (lo0 < len) rv[lo0] = r0 - mult * v0;
                        for (int kk = kc + 64; kk < ec; kk += 64) {
                            const int lo = sc[kk];
                            if (lo < len) rv[lo] = rv[lo] - mult * sv[kk];
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
            __syncthreads();
            ta = tb;
            continue;
        }
        if (tb > ta) {
            const int cnt = so[tb] - base;
            if (pre)
                ilu0_stage_part<DEP, false, true>(ta, tb, base, cnt, rp, ci, lu, len, hbits, rc, so, su, sc, sv, hk, hp);
            else
                ilu0_stage_part<DEP, true, true>(ta, tb, base, cnt, rp, ci, lu, len, hbits, rc, so, su, sc, sv, hk, hp);
            __syncthreads();
            if (w0) {
                // (one wave: its LDS accesses complete in order, so no barrier between pivots;
                // pivot t + 1's first entries and 1/u_rr are read before pivot t's updates --
                // the staged arrays are not written here)
                int k0 = so[ta] - base + lane, e0 = so[ta + 1] - base;
                int lon = k0 < e0 ? sc[k0] : len;
                double vn = k0 < e0 ? sv[k0] : 0.0, dn = sd[ta];
                for (int t = ta; t < tb; ++t) {
                    const int lo0 = lon, kc = k0, ec = e0;
                    const double v0 = vn, dc = dn;
                    if (t + 1 < tb) {
                        k0 = so[t + 1] - base + lane;
                        e0 = so[t + 2] - base;
                        lon = k0 < e0 ? sc[k0] : len;
                        vn = k0 < e0 ? sv[k0] : 0.0;
                        dn = sd[t + 1];
                    }
                    // rv[t] and the first entry the pivot updates are read together (one LDS
                    // round trip per pivot on the chain): positions of pivot t's upper part
                    // are > t and distinct, so nothing writes rv[lo0] in between
                    const double pc = rv[t];
                    const double r0 = rv[lo0 < len ? lo0 : t];
                    if (pc != 0.0) {
                        const double mult = pc * dc;
                        if (lane == 0) rv[t] = mult;
                        if (lo0 < len) rv[lo0] = r0 - mult * v0;
                        for (int kk = kc + 64; kk < ec; kk += 64) {
                            const int lo = sc[kk];
                            if (lo < len) rv[lo] = rv[lo] - mult * sv[kk];
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
            __syncthreads();  // (the next segment overwrites the stage)
            ta = tb;
            continue;
        }
        const int t = ta++;
        if (w0) {
            const double pc = rv[t];
            if (pc != 0.0) {
                const int64_t r = rc[t];
                const double mult = pc * ilu0_ld<DEP>(dinv + r);
                if (lane == 0) rv[t] = mult;
                const int64_t us = diag[r] + 1, ue = rp[r + 1];
                for (int64_t kk = us + lane; kk < ue; kk += 64) {
                    const int32_t j = ci[kk];
                    int lo = len;
                    if (hbits > 0) {  // the column's position in the row (hash)
                        uint32_t h = hslot(j);
                        int32_t key = hk[h];
                        while (key != j && key != -1) {
                            h = (h + 1) & hmask;
                            key = hk[h];
                        }
                        if (key == j) lo = hp[h];
                    } else {  // search j in rc[t+1, len)
                        int a = t + 1, b = len;
                        while (a < b) {
                            const int m = (a + b) >> 1;
                            if (rc[m] < j) a = m + 1; else b = m;
                        }
                        if (a < len && rc[a] == j) lo = a;
                    }
                    if (lo < len) rv[lo] = rv[lo] - mult * ilu0_ld<DEP>(lu + kk);
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    for (int t = tid; t < len; t += ILU0_TPB) ilu0_st<DEP>(lu + s + t, rv[t]);
    if (tid == 0) {
        const double piv = rv[dl];
        if (piv == 0.0) atomicMax(fail, 2);
        ilu0_st<DEP>(dinv + i, piv == 0.0 ? 0.0 : 1.0 / piv);
    }
    if (DEP) {  // publish: the row's coherent stores complete, then its flag
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        if (tid == 0) __hip_atomic_store(done + i, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return true;
}

__global__ __launch_bounds__(ILU0_TPB) void k_ilu0_level(const int32_t *__restrict__ rows,
                                                         const int64_t *__restrict__ rp,
                                                         const int32_t *__restrict__ ci, double *__restrict__ lu,
                                                         const int64_t *__restrict__ diag, double *__restrict__ dinv,
                                                         int32_t *fail, int max_row, int stage, int hbits) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    (void)ilu0_row<false>(rows[blockIdx.x], rp, ci, lu, diag, dinv, fail, max_row, stage, hbits, smem, nullptr,
                          nullptr);
}

// all levels in one launch: ctr[0] draws rows (rows: level order, so every
// pivot row was drawn earlier -- by a running workgroup -- and the lowest
// unfinished drawn row always has its pivots done: no deadlock); ctr[1] =
// abort flag; done[n] zeroed by the caller
__global__ __launch_bounds__(ILU0_TPB) void k_ilu0_dep(int64_t n, const int32_t *__restrict__ rows,
                                                       const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                       double *lu, const int64_t *__restrict__ diag, double *dinv,
                                                       int32_t *fail, int max_row, int stage, int hbits,
                                                       int32_t *done, int32_t *ctr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    for (;;) {
        if (threadIdx.x == 0) {
            const int q = atomicAdd(ctr, 1);
            ilu0_ctl[0] = (q >= n || __hip_atomic_load(ctr + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ? -1 : q;
        }
        __syncthreads();
        const int q = ilu0_ctl[0];
        __syncthreads();
        if (q < 0) return;
        if (!ilu0_row<true>(rows[q], rp, ci, lu, diag, dinv, fail, max_row, stage, hbits, smem, done, ctr + 1))
            return;
        __syncthreads();
    }
}
#pragma clang fp contract(on)

// the LDS the factorization kernels take for rows of up to max_row entries, `stage` staged
// entries and a 2^hbits-slot column hash
static size_t ilu0_lds_bytes(int64_t max_row, int64_t stage, int hbits) {
    const int64_t m = max_row < 1 ? 1 : max_row;
    // the per-pivot arrays (offsets, 1/u_rr, first entries) exist only with a stage
    const int64_t extra = (stage > 0 ? (m + 1) * 4 + 8 + m * 16 : 0) + (hbits > 0 ? (int64_t)8 << hbits : 0);
    return (size_t)(((m * 12 + stage * 12 + extra) + 15) & ~(int64_t)15);
}
// hash slots (at least twice the longest row) and staged entries (the most one
// row needs, at most ILU0_STAGE) that fit the LDS; 0 = none.  stage_cap >= 0 (test
// knob pls.ilu0_stage) caps the staged entries: 0 stages none, every pivot goes
// through global memory; small values force the segmented path
static void ilu0_plan(int64_t max_row, int64_t max_staged, int stage_cap, int &stage, int &hbits) {
    hbits = 7;
    while ((int64_t)1 << hbits < 2 * max_row) ++hbits;
    if (ilu0_lds_bytes(max_row, 0, hbits) > ILU0_LDS) hbits = 0;
    stage = 0;
    int64_t want = std::min<int64_t>(ILU0_STAGE, std::max<int64_t>(256, (max_staged + 63) & ~(int64_t)63));
    if (stage_cap >= 0) want = std::min<int64_t>(want, stage_cap);
    for (int64_t st = want; st >= std::min<int64_t>(want, 256) && st > 0; st /= 2)
        if (ilu0_lds_bytes(max_row, st, hbits) <= ILU0_LDS) {
            stage = (int)st;
            break;
        }
}
// the longest row with no stage: row values and columns (12 bytes per entry)
int ilu0_max_row() { return (ILU0_LDS - 16) / 12; }
void launch_ilu0_dep(int64_t n, const int32_t *rows, const int64_t *rp, const int32_t *ci, double *lu,
                     const int64_t *diag, double *dinv, int32_t *fail, int64_t max_row, int64_t max_staged,
                     int stage_cap, int grid_cap, int32_t *done, int32_t *ctr, hipStream_t st) {
    if (n <= 0) return;
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void *)k_ilu0_dep, hipFuncAttributeMaxDynamicSharedMemorySize, ILU0_LDS);
        attr = true;
    }
    int stage = 0, hbits = 0;
    ilu0_plan(max_row, max_staged, stage_cap, stage, hbits);
    const size_t lds = ilu0_lds_bytes(max_row, stage, hbits);
    (void)hipMemsetAsync(done, 0, sizeof(int32_t) * n, st);
    (void)hipMemsetAsync(ctr, 0, sizeof(int32_t) * 2, st);
    // persistent: the workgroups that fit (4 per CU at most), never more than rows
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(4, 163840 / (int64_t)(lds + 512)));
    int64_t grid = std::min<int64_t>(n, 256 * per_cu);
    // (test knob pls.ilu_dep_grid; 1: one workgroup takes the rows in draw order -- a draw order
    // that is not a topological order of the pivot DAG would then stop at the bounded wait)
    if (grid_cap > 0) grid = std::min<int64_t>(grid, grid_cap);
    k_ilu0_dep<<<(unsigned)grid, ILU0_TPB, lds, st>>>(n, rows, rp, ci, lu, diag, dinv, fail,
                                                       (int)(max_row < 1 ? 1 : max_row), stage, hbits, done, ctr);
}
void launch_ilu0_level(int64_t nrows_level, const int32_t *rows, const int64_t *rp, const int32_t *ci, double *lu,
                       const int64_t *diag, double *dinv, int32_t *fail, int64_t max_row, int64_t max_staged,
                       int stage_cap, hipStream_t st) {
    // caller guarantees max_row <= ilu0_max_row(); LDS sized to the longest row (occupancy for short rows)
    if (nrows_level <= 0) return;
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void *)k_ilu0_level, hipFuncAttributeMaxDynamicSharedMemorySize, ILU0_LDS);
        attr = true;
    }
    int stage = 0, hbits = 0;
    ilu0_plan(max_row, max_staged, stage_cap, stage, hbits);
    k_ilu0_level<<<(unsigned)nrows_level, ILU0_TPB, ilu0_lds_bytes(max_row, stage, hbits), st>>>(
        rows, rp, ci, lu, diag, dinv, fail, (int)(max_row < 1 ? 1 : max_row), stage, hbits);
}

__global__ __launch_bounds__(TPB) void k_lvl_count(int64_t n, const int32_t *order, const int64_t *rp,
                                                   const int64_t *diag, int upper, int64_t *len) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r > n) return;
    if (r == n) { len[n] = 0; return; }
    const int64_t i = order[r];
    len[r] = upper ? (rp[i + 1] - diag[i] - 1) : (diag[i] - rp[i]);
}
__global__ __launch_bounds__(TPB) void k_lvl_fill(int64_t n, const int32_t *order, const int64_t *rp,
                                                  const int32_t *ci, const double *lu, const int64_t *diag, int upper,
                                                  const int64_t *orp, int32_t *oci, double *oval) {
    const int64_t r = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    if (r >= n) return;
    const int64_t i = order[r];
    const int64_t src = upper ? diag[i] + 1 : rp[i];
    const int64_t dst = orp[r], cnt = orp[r + 1] - dst;
    for (int64_t k = l; k < cnt; k += 16) {
        oci[dst + k] = ci[src + k];
        oval[dst + k] = lu[src + k];
    }
}
void launch_lvl_count(int64_t n, const int32_t *order, const int64_t *rp, const int64_t *diag, int upper,
                      int64_t *len, hipStream_t st) {
    k_lvl_count<<<grid_for(n + 1, TPB), TPB, 0, st>>>(n, order, rp, diag, upper, len);
}
void launch_lvl_fill(int64_t n, const int32_t *order, const int64_t *rp, const int32_t *ci, const double *lu,
                     const int64_t *diag, int upper, const int64_t *out_rp, int32_t *out_ci, double *out_val,
                     hipStream_t st) {
    if (n > 0)
        k_lvl_fill<<<grid_for(n * 16, TPB), TPB, 0, st>>>(n, order, rp, ci, lu, diag, upper, out_rp, out_ci,
                                                         out_val);
}

// level of a triangular sweep.  forward (dinv == null): y[i] = b[i] - sum
// backward: y[i] = (y[i] - sum) * dinv[r]
template <int LPR>
__global__ __launch_bounds__(TPB) void k_trsv_level(int64_t r0, int64_t r1, const int32_t *__restrict__ row_of,
                                                    const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                    const double *__restrict__ val, const double *__restrict__ dinv,
                                                    const double *b, double *y) {
    const int sub = threadIdx.x & (LPR - 1);
    const int64_t r = r0 + ((int64_t)blockIdx.x * TPB + threadIdx.x) / LPR;
    if (r >= r1) return;
    const int64_t i = row_of[r];
    const int64_t s = rp[r], e = rp[r + 1];
    double acc = row_dot<LPR, 2, false>(s, e, sub, ci, val, y);
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (sub == 0) {
        if (dinv) y[i] = (y[i] - acc) * dinv[r];
        else y[i] = b[i] - acc;
    }
}

void launch_trsv_level(int64_t r0, int64_t r1, const int32_t *row_of, const int64_t *rp, const int32_t *ci,
                       const double *val, const double *dinv_lvl, const double *b, double *y, int lpr,
                       hipStream_t st) {
    const int64_t rows = r1 - r0;
    if (rows <= 0) return;
    switch (lpr) {
        case 64: k_trsv_level<64><<<grid_for(rows, TPB / 64), TPB, 0, st>>>(r0, r1, row_of, rp, ci, val, dinv_lvl, b, y); break;
        case 32: k_trsv_level<32><<<grid_for(rows, TPB / 32), TPB, 0, st>>>(r0, r1, row_of, rp, ci, val, dinv_lvl, b, y); break;
        case 16: k_trsv_level<16><<<grid_for(rows, TPB / 16), TPB, 0, st>>>(r0, r1, row_of, rp, ci, val, dinv_lvl, b, y); break;
        case 8: k_trsv_level<8><<<grid_for(rows, TPB / 8), TPB, 0, st>>>(r0, r1, row_of, rp, ci, val, dinv_lvl, b, y); break;
        default: k_trsv_level<4><<<grid_for(rows, TPB / 4), TPB, 0, st>>>(r0, r1, row_of, rp, ci, val, dinv_lvl, b, y); break;
    }
}

// Block-Jacobi sweep: one workgroup per diagonal block walks that block's
// levels (rows stored block-major, level-ordered) with only a workgroup
// barrier between levels -- the blocks are independent, so no grid-wide sync
// and no per-level launch.  y is read/written through L1 by the workgroup's
// own waves only (workgroup-scope visibility via __syncthreads()).
template <int LPR>
__global__ __launch_bounds__(512) void k_trsv_blocks(const int64_t *__restrict__ blk_off,
                                                     const int64_t *__restrict__ lvl_ptr,
                                                     const int32_t *__restrict__ row_of,
                                                     const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                     const double *__restrict__ val, const double *__restrict__ dinv,
                                                     const double *b, double *y) {
    const int sub = threadIdx.x & (LPR - 1);
    const int grp = threadIdx.x / LPR;
    constexpr int NG = 512 / LPR;
    const int64_t l0 = blk_off[blockIdx.x], l1 = blk_off[blockIdx.x + 1];
    for (int64_t l = l0; l < l1; ++l) {
        const int64_t rs = lvl_ptr[l], re = lvl_ptr[l + 1];
        for (int64_t r = rs + grp; r < re; r += NG) {
            const int64_t i = row_of[r];
            const int64_t s = rp[r], e = rp[r + 1];
            double acc = row_dot<LPR, 2, false>(s, e, sub, ci, val, y);
#pragma unroll
            for (int o = LPR / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if (sub == 0) {
                if (dinv) y[i] = (y[i] - acc) * dinv[r];
                else y[i] = b[i] - acc;
            }
        }
        __syncthreads();
    }
}

void launch_trsv_blocks(int64_t nblocks, const int64_t *blk_off, const int64_t *lvl_ptr, const int32_t *row_of,
                        const int64_t *rp, const int32_t *ci, const double *val, const double *dinv_lvl,
                        const double *b, double *y, int lpr, hipStream_t st) {
    if (nblocks <= 0) return;
    switch (lpr) {
        case 64: k_trsv_blocks<64><<<(unsigned)nblocks, 512, 0, st>>>(blk_off, lvl_ptr, row_of, rp, ci, val, dinv_lvl, b, y); break;
        case 32: k_trsv_blocks<32><<<(unsigned)nblocks, 512, 0, st>>>(blk_off, lvl_ptr, row_of, rp, ci, val, dinv_lvl, b, y); break;
        case 16: k_trsv_blocks<16><<<(unsigned)nblocks, 512, 0, st>>>(blk_off, lvl_ptr, row_of, rp, ci, val, dinv_lvl, b, y); break;
        case 8: k_trsv_blocks<8><<<(unsigned)nblocks, 512, 0, st>>>(blk_off, lvl_ptr, row_of, rp, ci, val, dinv_lvl, b, y); break;
        default: k_trsv_blocks<4><<<(unsigned)nblocks, 512, 0, st>>>(blk_off, lvl_ptr, row_of, rp, ci, val, dinv_lvl, b, y); break;
    }
}

}  // namespace pls
