// sweep_lds.hip -- level-aligned SELL-64 triangular factors, the LDS stream layout and the
// block sweeps that run a block's levels in one workgroup: LDS, ring, ASM (gfx950).
#include "devutil.hpp"

namespace pls {

// Multiply-adds contract within a statement only, never across statements (the compiler's
// default for device code would fuse across them): the rounding of the recorded results.
#pragma clang fp contract(on)

// ================================================= level-aligned SELL-64 ====
// Triangular factors for the sweeps: rows grouped by (block, level), every
// group padded to whole 64-row slices, entry k of a slice's rows contiguous
// (sptr[s] + 64 k + lane).  Lane = row: coalesced val/col loads, no lane
// reduction, and the U entries a lane keeps in flight are independent of the
// level barrier.  Padding entries are discarded by a select (never multiplied
// into the sum), so uninitialised y entries cannot leak NaNs.
__global__ __launch_bounds__(TPB) void k_tri_fill(int64_t nslices, const int32_t *slot_row, const int32_t *slot_len,
                                                  const int64_t *rp, const int32_t *ci, const double *lu,
                                                  const int64_t *diag, const double *dinv, int upper,
                                                  const int64_t *sptr, int32_t *ocol, double *oval, double *odinv) {
    const int64_t sl = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (sl >= nslices) return;
    const int64_t slot = sl * 64 + lane;
    const int32_t i = slot_row[slot];
    const int32_t len = slot_len[slot];
    const int64_t base = sptr[sl];
    const int64_t L = (sptr[sl + 1] - base) >> 6;
    const int64_t src = (i < 0) ? 0 : (upper ? diag[i] + 1 : rp[i]);
    for (int64_t k = 0; k < L; ++k) {
        const int64_t pos = base + k * 64 + lane;
        if (k < len) {
            ocol[pos] = ci[src + k];
            oval[pos] = lu[src + k];
        } else {
            ocol[pos] = 0;
            oval[pos] = 0.0;
        }
    }
    if (odinv) odinv[slot] = (i < 0) ? 1.0 : dinv[i];
}

template <int U>
__device__ __forceinline__ void tri_slice(int64_t sl, int lane, const int64_t *__restrict__ sptr,
                                          const int32_t *__restrict__ slot_row, const int32_t *__restrict__ slot_len,
                                          const int32_t *__restrict__ col, const double *__restrict__ val,
                                          const double *__restrict__ sdinv, const double *b, double *y) {
    const int64_t slot = sl * 64 + lane;
    const int32_t i = slot_row[slot];
    const int32_t len = slot_len[slot];
    const int64_t base = sptr[sl];
    const int64_t L = (sptr[sl + 1] - base) >> 6;
    const int32_t *cp = col + base + lane;
    const double *vp = val + base + lane;
    double acc = 0.0;
    for (int64_t k0 = 0; k0 < L; k0 += U) {
        int32_t c[U];
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t kk = (k0 + u < L) ? k0 + u : L - 1;
            c[u] = cp[kk * 64];
            v[u] = vp[kk * 64];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double t = v[u] * y[(uint32_t)c[u]];
            acc += (k0 + u < len) ? t : 0.0;
        }
    }
    if (i >= 0) {
        if (sdinv) y[i] = (y[i] - acc) * sdinv[slot];
        else y[i] = b[i] - acc;
    }
}

// one workgroup per block: goff[blk]..goff[blk+1] groups, gslice[g] slices
__global__ __launch_bounds__(1024) void k_tri_blocks(const int64_t *__restrict__ goff,
                                                     const int64_t *__restrict__ gslice,
                                                     const int64_t *__restrict__ sptr, const int32_t *__restrict__ slot_row,
                                                     const int32_t *__restrict__ slot_len, const int32_t *__restrict__ col,
                                                     const double *__restrict__ val, const double *__restrict__ sdinv,
                                                     const double *b, double *y) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    const int64_t g0 = goff[blockIdx.x], g1 = goff[blockIdx.x + 1];
    for (int64_t g = g0; g < g1; ++g) {
        const int64_t s1 = gslice[g + 1];
        for (int64_t sl = gslice[g] + wave; sl < s1; sl += nw)
            tri_slice<4>(sl, lane, sptr, slot_row, slot_len, col, val, sdinv, b, y);
        __syncthreads();
    }
}

// one launch per group (global levels): slices [s0, s1)
__global__ __launch_bounds__(TPB) void k_tri_group(int64_t s0, int64_t s1, const int64_t *__restrict__ sptr,
                                                   const int32_t *__restrict__ slot_row,
                                                   const int32_t *__restrict__ slot_len, const int32_t *__restrict__ col,
                                                   const double *__restrict__ val, const double *__restrict__ sdinv,
                                                   const double *b, double *y) {
    const int lane = threadIdx.x & 63;
    const int64_t sl = s0 + (((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6);
    if (sl >= s1) return;
    tri_slice<4>(sl, lane, sptr, slot_row, slot_len, col, val, sdinv, b, y);
}

void launch_tri_fill(int64_t nslices, const int32_t *slot_row, const int32_t *slot_len, const int64_t *rp,
                     const int32_t *ci, const double *lu, const int64_t *diag, const double *dinv, int upper,
                     const int64_t *sptr, int32_t *ocol, double *oval, double *odinv, hipStream_t st) {
    if (nslices > 0)
        k_tri_fill<<<grid_for(nslices * 64, TPB), TPB, 0, st>>>(nslices, slot_row, slot_len, rp, ci, lu, diag, dinv,
                                                                upper, sptr, ocol, oval, odinv);
}
void launch_tri_blocks(int64_t nblocks, const int64_t *goff, const int64_t *gslice, const int64_t *sptr,
                       const int32_t *slot_row, const int32_t *slot_len, const int32_t *col, const double *val,
                       const double *sdinv, const double *b, double *y, hipStream_t st) {
    if (nblocks > 0)
        k_tri_blocks<<<(unsigned)nblocks, 1024, 0, st>>>(goff, gslice, sptr, slot_row, slot_len, col, val, sdinv, b, y);
}
// One level of a triangular sweep straight from the factored CSR: TRI_G lanes
// per row (entries dealt round robin, partial sums combined by lane shuffles),
// so a long row costs one or two dependent gather rounds instead of one per
// entry as with a lane per row.  upper = 0: y_i = b_i - sum_{k < diag} l_ik y_k;
// 1: y_i = dinv_i (b_i - sum_{k > diag} u_ik y_k) (b may alias y).
static constexpr int TRI_G = 16;
__global__ __launch_bounds__(TPB) void k_tri_csr_level(int64_t m, const int32_t *__restrict__ rows,
                                                       const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                       const double *__restrict__ val, const int64_t *__restrict__ diag,
                                                       const double *__restrict__ dinv, int upper, const double *b,
                                                       double *y) {
    const int64_t gid = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const int64_t r = gid / TRI_G;
    const int j = (int)(gid % TRI_G);
    if (r >= m) return;  // whole groups of TRI_G lanes (m rows x TRI_G lanes, TRI_G divides 64)
    const int64_t i = rows[r], d = diag[i];
    const int64_t lo = upper ? d + 1 : rp[i], hi = upper ? rp[i + 1] : d;
    double s = 0.0;
    for (int64_t k = lo + j; k < hi; k += TRI_G) s += val[k] * y[ci[k]];
#pragma unroll
    for (int off = TRI_G / 2; off >= 1; off >>= 1) s += __shfl_xor(s, off, TRI_G);
    if (j == 0) {
        const double v = b[i] - s;
        y[i] = upper ? v * dinv[i] : v;
    }
}
void launch_tri_csr_level(int64_t m, const int32_t *rows, const int64_t *rp, const int32_t *ci, const double *val,
                          const int64_t *diag, const double *dinv, int upper, const double *b, double *y,
                          hipStream_t st) {
    if (m > 0)
        k_tri_csr_level<<<grid_for(m * TRI_G, TPB), TPB, 0, st>>>(m, rows, rp, ci, val, diag, dinv, upper, b, y);
}
void launch_tri_group(int64_t s0, int64_t s1, const int64_t *sptr, const int32_t *slot_row, const int32_t *slot_len,
                      const int32_t *col, const double *val, const double *sdinv, const double *b, double *y,
                      hipStream_t st) {
    if (s1 > s0)
        k_tri_group<<<grid_for((s1 - s0) * 64, TPB), TPB, 0, st>>>(s0, s1, sptr, slot_row, slot_len, col, val, sdinv,
                                                                   b, y);
}

// Block-Jacobi ILU(0) apply with the block's solution resident in LDS: the
// truncated factors only reference rows of their own block, so one workgroup
// loads x[b0, b0+len) into LDS, runs every forward level then every backward
// level against LDS (gathers and updates never leave the CU), and writes the
// block of y once.  Blocks are launched heaviest-last-index first (the
// pressure blocks at the end of the fp ordering carry the most levels).
// ------------------------------------------------ LDS sweep stream layout --
// The block-Jacobi LDS kernel reads each level's slices as streams.  A block
// whose rows are long gives each row LPR = 2 or 4 lanes (8 or 16 in the
// y-resident variant; entries dealt round robin, partial sums combined with
// lane shuffles), so every lane's share fits the P entries the pipeline keeps
// in registers; short-row blocks keep LPR = 1.  Slice = 64 / LPR rows of one
// level.  Entry 0 of every lane is a header -- col = (row - b0) | (entries of
// this lane << SW_ROW_BITS) (row SW_ROW_PAD: padding; 14 bits hold the
// longest row, ilu0_max_row()), val = 1/U_ii (upper factor) -- entries 1..L the lane's factor
// entries with block-local columns.  The only metadata a level needs is where
// its slice starts, known 64 levels ahead (see sweep2), so loads are issued D
// levels before use without a dependent metadata hop.
// (SW_ROW_BITS, SW_ROW_PAD: devutil.hpp, the chain sweep reads the same headers)

__global__ __launch_bounds__(TPB) void k_lds_fill(int64_t nslices, const int32_t *s_start, const int32_t *s_n,
                                                  const int32_t *s_lpr, const int32_t *order, const int64_t *rp,
                                                  const int32_t *ci, const double *lu, const int64_t *diag,
                                                  const double *dinv, int upper, int64_t n, int64_t nb,
                                                  const int64_t *sptr2, int32_t *ocol, double *oval, int wide,
                                                  const int32_t *posof, const int32_t *row_lo, const int64_t *bstart) {
    const int64_t sl = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (sl >= nslices) return;
    const int lpr = s_lpr[sl];
    const int r = lane / lpr, sub = lane % lpr;
    const int64_t i = r < s_n[sl] ? order[s_start[sl] + r] : -1;
    const int64_t base = sptr2[sl], L = (sptr2[sl + 1] - base) >> 6;
    int64_t b0 = 0, src = 0, len = 0;
    if (i >= 0) {
        int64_t blen;
        block_of(i, n, nb, bstart, b0, blen);
        src = upper ? diag[i] + 1 : rp[i];
        len = upper ? rp[i + 1] - diag[i] - 1 : diag[i] - rp[i];
    }
    const int64_t mine = len > sub ? (len - sub + lpr - 1) / lpr : 0;
    // posof (ring sweep): rows and columns become block-local positions in the
    // triangle's level order
    const int32_t me = i >= 0 ? (posof ? posof[i] : (int32_t)(i - b0)) : -1;
    // a padding lane's entries (value 0) read the slice's first row: in the
    // ring sweep that position is in the LDS ring, never a global fallback
    const int32_t pad = posof ? posof[order[s_start[sl]]] : 0;
    if (row_lo) {
        // ring sweep: only the row's near entries (position >= row_lo[i], in the
        // LDS ring when the row runs), dealt round robin over its lanes; the far
        // ones are applied to the row's input when its chunk is loaded.  Lane-
        // major layout: entry k of this lane at base + lane * L + k.
        const int32_t lo = i >= 0 ? row_lo[i] : 0;
        const int64_t lb = base + (int64_t)lane * L;
        ocol[lb] = me;
        oval[lb] = (upper && i >= 0) ? dinv[i] : 0.0;
        int64_t k = 1, m = 0;
        for (int64_t j = 0; j < len; ++j) {
            const int32_t pc = posof[ci[src + j]];
            if (pc < lo) continue;
            if (m++ % lpr != sub) continue;
            ocol[lb + k] = pc;
            oval[lb + k] = lu[src + j];
            ++k;
        }
        for (; k < L; ++k) {
            ocol[lb + k] = i >= 0 ? me : pad;
            oval[lb + k] = 0.0;
        }
        return;
    }
    ocol[base + lane] = wide ? me : (i >= 0 ? me : SW_ROW_PAD) | (int32_t)(mine << SW_ROW_BITS);
    oval[base + lane] = (upper && i >= 0) ? dinv[i] : 0.0;
    for (int64_t k = 1; k < L; ++k) {
        const int64_t j = (k - 1) * lpr + sub, pos = base + k * 64 + lane;
        ocol[pos] = j < len ? (posof ? posof[ci[src + j]] : (int32_t)(ci[src + j] - b0)) : (wide && i >= 0 ? me : pad);
        oval[pos] = j < len ? lu[src + j] : 0.0;
    }
}
void launch_lds_fill(int64_t nslices, const int32_t *s_start, const int32_t *s_n, const int32_t *s_lpr,
                     const int32_t *order, const int64_t *rp, const int32_t *ci, const double *lu, const int64_t *diag,
                     const double *dinv, int upper, int64_t n, int64_t nb, const int64_t *sptr2, int32_t *ocol,
                     double *oval, hipStream_t st, bool wide, const int32_t *posof, const int32_t *row_lo,
                     const int64_t *bstart) {
    if (nslices > 0)
        k_lds_fill<<<grid_for(nslices * 64, TPB), TPB, 0, st>>>(nslices, s_start, s_n, s_lpr, order, rp, ci, lu, diag,
                                                                dinv, upper, n, nb, sptr2, ocol, oval, wide ? 1 : 0,
                                                                posof, row_lo, bstart);
}

// One sweep over a block's levels.  Pipeline: the loads of level g+2 are
// issued while level g computes; slots live in a ring of 3 register sets
// indexed by compile-time constants (a register copy with a load in flight
// would make the compiler drain vmcnt to 0 every level).  Slice starts for 64
// levels come from vector registers (lane l: level gbase + l) filled by one
// gather per 62 levels and read with v_readlane -- no scalar loads in the
// loop, whose lgkmcnt waits would be paid at every LDS access.
template <int P>
struct Sw2Slot {
    int32_t c[P + 1];
    double v[P + 1];
    int64_t base, L;  // L: entries incl. header; base < 0: this wave has no slice
    int l2;           // ring sweep: log2 of the slice's lanes per row (slice starts carry it in bits 0-2)
};

// Ring sweep (R): the block solution lives in level-order position space; the
// last RING_SLOTS positions sit in an LDS ring (slot p % RING_SLOTS), older
// ones (far dependencies) were subtracted from the row's input when its chunk
// loaded (from the position-ordered global copy ypos).  Positions are
// processed in chunks of at most RING_CHUNK (level-aligned): at a chunk's first
// level its inputs are loaded into their ring slots, after which every
// position >= lo_ok = chunk end - RING_SLOTS is still in the ring.
static constexpr int RING_SLOTS = 16384;
static constexpr int RING_CHUNK = 4096;
struct RingIn {
    const int64_t *cg, *cp;   // per chunk: first level (group) / [start, end) positions (cp[2k], cp[2k+1])
    const int32_t *src_idx;   // per position: index of its input value in src (block offset b0 included)
    const double *src;        // L: x; U: the L sweep's ypos
    const int64_t *frp;       // far dependencies per position (b0 + p): CSR row pointers
    const int32_t *fcol;      // ... their block-local positions
    const double *fval;       // ... factor values
};
struct Sw2Ctx {
    const int64_t *gslice, *sptr;
    const int32_t *col;
    const double *val;
    double *ys;
    int64_t g1, gbase;
    int64_t gv, sb, se;  // lane l: gslice[gbase+l], sptr[gslice+wave], sptr[gslice+wave+1] (-1: none)
    int lane, wave, nw;
    bool upper;
    // ring sweep only
    double *ring, *ypos;     // LDS ring; this sweep's position-ordered output (block offset applied)
    int64_t lo_ok, ck, cend, cnext, b0, ck0;
    RingIn rin;
    __device__ __forceinline__ void refill(int64_t g) {
        gbase = g;
        const int64_t k = g + lane;
        const int64_t kc = k < g1 ? k : g1;
        gv = gslice[kc];
        const int64_t gn = gslice[kc + 1 <= g1 ? kc + 1 : g1];
        const int64_t sl = gv + wave;
        const bool ok = k < g1 && sl < gn;
        sb = ok ? sptr[sl] : -1;
        se = ok ? sptr[sl + 1] : -1;
        // consume the loads here: otherwise every level's v_readlane of these
        // registers inherits the refill path's "load pending" state and the
        // compiler drains vmcnt to 0 at each level, exposing all prefetches
        asm volatile("" : "+v"(gv), "+v"(sb), "+v"(se));
    }
};

template <int P, bool R>
__device__ __forceinline__ void sw2_issue(Sw2Ctx &x, int64_t g, Sw2Slot<P> &s) {
    const int l = (int)(g - x.gbase);
    int64_t base = g < x.g1 ? readlane64(x.sb, l) : -1;
    int64_t next = base >= 0 ? readlane64(x.se, l) : 0;
    s.l2 = 0;
    if (R) {  // slice starts are multiples of 64 entries; bits 0-2: log2(lanes per row)
        s.l2 = base >= 0 ? (int)(base & 7) : 0;
        base = base >= 0 ? (base & ~(int64_t)63) : -1;
        next &= ~(int64_t)63;
    }
    const int64_t L = base >= 0 ? (next - base) >> 6 : 0;
    s.base = base;
    s.L = L;
    if (R) {
        // ring sweep: buffer loads through per-slot descriptors bounded to the
        // slice (0 bytes for an idle wave): entries past the slice and idle
        // waves' loads are range-checked away (no traffic, reads return 0),
        // and every path issues the same loads, which keeps the compiler's
        // vmcnt bookkeeping exact -- using this slot two levels later waits for
        // its own loads only (a branch around them made it wait for everything
        // in flight, the prefetch issued this level included)
        static_assert((P + 1) % 8 == 0, "the ring sweep's slot is one lane's first P + 1 entries (a multiple of 8)");
        const int64_t b = base >= 0 ? base : 0;
        const int nc = base >= 0 ? (int)(L * 64 * 4) : 0;
        const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void *)(x.col + b), (short)0, nc, 0x00020000);
        const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void *)(x.val + b), (short)0, 2 * nc, 0x00020000);
        const int off = x.lane * (int)L;  // lane-major, L a multiple of P + 1
#pragma unroll
        for (int q = 0; q < (P + 1) / 4; ++q) {
            const auto c4 = __builtin_amdgcn_raw_buffer_load_b128(rc, (off + 4 * q) * 4, 0, 0);
            s.c[4 * q + 0] = (int32_t)c4[0];
            s.c[4 * q + 1] = (int32_t)c4[1];
            s.c[4 * q + 2] = (int32_t)c4[2];
            s.c[4 * q + 3] = (int32_t)c4[3];
        }
#pragma unroll
        for (int q = 0; q < (P + 1) / 2; ++q) {
            const auto v4 = __builtin_amdgcn_raw_buffer_load_b128(rv, (off + 2 * q) * 8, 0, 0);
            s.v[2 * q + 0] = __builtin_bit_cast(double, ((uint64_t)v4[1] << 32) | v4[0]);
            s.v[2 * q + 1] = __builtin_bit_cast(double, ((uint64_t)v4[3] << 32) | v4[2]);
        }
        return;
    }
    if (base < 0) {  // wave idle at this level: no loads (they would only queue in the CU's memory pipe)
#pragma unroll
        for (int u = 0; u <= P; ++u) {
            s.c[u] = 0;
            s.v[u] = 0.0;
        }
        return;
    }
#pragma unroll
    for (int u = 0; u <= P; ++u) {
        const int64_t pos = base + (u < L ? u : 0) * 64 + x.lane;
        s.c[u] = __builtin_nontemporal_load(x.col + pos);
        s.v[u] = __builtin_nontemporal_load(x.val + pos);
    }
}

// W (wide, the y-resident sweep): header col = local row (-1: padding lane),
// a lane's padding entries point at its own row with value 0, so only the
// slice length masks entries and blocks may have up to 2^31 rows.
// the value of a dependency (block-local row, or position in the ring sweep)
template <bool R>
__device__ __forceinline__ double sw2_dep(const Sw2Ctx &x, int32_t c) {
    // ring sweep: every stream entry is a near dependency, in the LDS ring (no
    // global load in the level loop: vmcnt waits would drain the prefetches)
    if (R) return x.ring[c & (RING_SLOTS - 1)];
    return x.ys[c];
}

// index of entry k of a lane's stream: [k][lane] (LDS / y-resident sweeps) or,
// in the ring sweep, lane-major [lane][k] with L (a multiple of 8) entries per
// lane, so a slot's first 8 columns / values are 2 / 4 16-byte loads
template <bool R>
__device__ __forceinline__ int64_t sw2_at(int64_t base, int64_t L, int lane, int64_t k) {
    return R ? base + (int64_t)lane * L + k : base + k * 64 + lane;
}

// LPR = 0: lanes per row chosen per slice (ring sweep), 1 << l2
template <int LPR, bool W, bool R>
__device__ __forceinline__ void sw2_finish(const Sw2Ctx &x, int32_t h, double dv, double acc, int l2 = 0) {
    // the LPR partial sums of a row: quad_perm xor 1, xor 2, then row_half_mirror
    // and row_mirror -- after the quad steps every lane of a quad holds the same
    // value, so mirroring pairs exactly the sums xor 4 / xor 8 would (a + b =
    // b + a: bitwise the shuffle tree), without LDS round trips
    const int lg = LPR ? (LPR >= 32 ? 5 : LPR >= 16 ? 4 : LPR >= 8 ? 3 : LPR >= 4 ? 2 : LPR >= 2 ? 1 : 0) : l2;
    if (lg >= 1) acc += dpp_d<0xB1>(acc);
    if (lg >= 2) acc += dpp_d<0x4E>(acc);
    if (lg >= 3) acc += dpp_d<0x141>(acc);
    if (lg >= 4) acc += dpp_d<0x140>(acc);
    if (lg >= 5) acc += __shfl_xor(acc, 16);
    const int32_t li = W ? h : (h & SW_ROW_PAD);
    if ((x.lane & ((1 << lg) - 1)) == 0 && (W ? li >= 0 : li != SW_ROW_PAD)) {
        if (R) {  // li: the row's position; its input sits in its ring slot
            double *slot = x.ring + (li & (RING_SLOTS - 1));
            *slot = x.upper ? (*slot - acc) * dv : *slot - acc;  // to ypos in bulk at the next chunk
        } else {
            x.ys[li] = x.upper ? (x.ys[li] - acc) * dv : x.ys[li] - acc;
        }
    }
}

template <int LPR, bool W, bool R>
__device__ __forceinline__ void sw2_slice_inline(const Sw2Ctx &x, int64_t sl) {
    const int64_t enc = x.sptr[sl];
    const int64_t base = R ? (enc & ~(int64_t)63) : enc;
    const int64_t L = ((R ? (x.sptr[sl + 1] & ~(int64_t)63) : x.sptr[sl + 1]) - base) >> 6;
    const int32_t h = x.col[sw2_at<R>(base, L, x.lane, 0)];
    const double dv = x.val[sw2_at<R>(base, L, x.lane, 0)];
    const int32_t len = (int32_t)((uint32_t)h >> SW_ROW_BITS);
    double acc = 0.0;
    for (int64_t k = 1; k < L; ++k) {
        const int64_t pos = sw2_at<R>(base, L, x.lane, k);
        const int32_t cc = x.col[pos];
        const double vv = x.val[pos];
        if (W || k <= len) acc += __dmul_rn(vv, sw2_dep<R>(x, cc));
    }
    sw2_finish<LPR, W, R>(x, h, dv, acc, R ? (int)(enc & 7) : 0);
}

// ring sweep: results of positions [p0, p1) from the ring to ypos (they stay in
// the ring for RING_SLOTS - RING_CHUNK >= RING_CHUNK more positions)
__device__ __forceinline__ void ring_flush(Sw2Ctx &x, int64_t p0, int64_t p1) {
    for (int64_t t = p0 + threadIdx.x; t < p1; t += blockDim.x) x.ypos[t] = x.ring[t & (RING_SLOTS - 1)];
}

// ring sweep: at the first level of a chunk, the previous chunk's results to
// ypos, then this chunk's inputs into the ring
__device__ __forceinline__ void ring_chunk(Sw2Ctx &x, int64_t g) {
    if (g != x.cnext) return;
    if (x.ck > x.ck0) ring_flush(x, x.rin.cp[2 * x.ck - 2], x.rin.cp[2 * x.ck - 1]);
    const int64_t c0 = x.rin.cp[2 * x.ck], c1 = x.rin.cp[2 * x.ck + 1];
    for (int64_t t = c0 + threadIdx.x; t < c1; t += blockDim.x) {
        double v = x.rin.src[x.rin.src_idx[x.b0 + t]];
        // far dependencies (older than the ring keeps, final before this chunk),
        // eight at a time: their column / value loads, then their eight ypos
        // gathers, are all in flight before the subtractions, which run in the
        // stream's order (one entry at a time, every load waited for in turn,
        // was ~2 global latencies per far entry -- most of the N=24 sweep's
        // skeleton time)
        const int64_t e0 = x.rin.frp[x.b0 + t], e1 = x.rin.frp[x.b0 + t + 1];
        for (int64_t e = e0; e < e1; e += 8) {
            int32_t fc[8];
            double fv[8], yv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t k = e + u < e1 ? e + u : e0;
                fc[u] = x.rin.fcol[k];
                fv[u] = x.rin.fval[k];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) yv[u] = x.ypos[fc[u]];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (e + u < e1) v -= fv[u] * yv[u];
        }
        x.ring[t & (RING_SLOTS - 1)] = v;
    }
    __syncthreads();
    x.lo_ok = c1 - RING_SLOTS;
    ++x.ck;
    x.cnext = x.ck < x.cend ? x.rin.cg[x.ck] : INT64_MAX;
}

template <int P, int LPR, bool W, bool R, int D = 2>
__device__ __forceinline__ void sw2_level(Sw2Ctx &x, int64_t g, const Sw2Slot<P> &cur, Sw2Slot<P> &ahead) {
    if (R) ring_chunk(x, g);
    if (g + D >= x.gbase + 64) x.refill(g);
    sw2_issue<P, R>(x, g + D, ahead);
    if (cur.base >= 0) {
        const int32_t h = cur.c[0];
        const int32_t len = W ? (int32_t)cur.L - 1 : (int32_t)((uint32_t)h >> SW_ROW_BITS);
        double acc = 0.0, d[P + 1];
        // every dependency read issued before the first is consumed (they are
        // independent; consuming in turn would serialise the LDS / L1 round trips)
        if (R) {
            // ring sweep: entries past the slice were range-checked to col 0 /
            // value 0 and padding entries carry value 0 on a written position,
            // so no masking: 0 * (a finite ring value) adds nothing
#pragma unroll
            for (int u = 1; u <= P; ++u) d[u] = sw2_dep<R>(x, cur.c[u]);
#pragma unroll
            for (int u = 1; u <= P; ++u) acc += __dmul_rn(cur.v[u], d[u]);  // no FMA: the other sweeps' rounding
        } else {
#pragma unroll
            for (int u = 1; u <= P; ++u) d[u] = sw2_dep<R>(x, u <= len ? cur.c[u] : 0);
#pragma unroll
            for (int u = 1; u <= P; ++u) {
                const double t = __dmul_rn(cur.v[u], d[u]);
                acc += (u <= len) ? t : 0.0;
            }
        }
        for (int64_t k0 = P + 1; k0 < cur.L; k0 += 8) {  // lanes with more than P entries: chunks of 8
            int32_t cc[8];
            double vv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t k = k0 + u < cur.L ? k0 + u : cur.L - 1;
                cc[u] = __builtin_nontemporal_load(x.col + sw2_at<R>(cur.base, cur.L, x.lane, k));
                vv[u] = __builtin_nontemporal_load(x.val + sw2_at<R>(cur.base, cur.L, x.lane, k));
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const double t = __dmul_rn(vv[u], sw2_dep<R>(x, k0 + u <= len ? cc[u] : 0));
                acc += (k0 + u <= len) ? t : 0.0;
            }
        }
        sw2_finish<LPR, W, R>(x, h, cur.v[0], acc, cur.l2);
        // levels with more slices than waves: the rest inline
        const int l = (int)(g - x.gbase);
        const int64_t s0 = readlane64(x.gv, l), s1 = readlane64(x.gv, l + 1);
        for (int64_t sl = s0 + x.wave + x.nw; sl < s1; sl += x.nw) sw2_slice_inline<LPR, W, R>(x, sl);
    }
    __syncthreads();
}

// D > 2: D levels of factor data in flight (D + 1 register slots, indexed by
// compile-time constants in the unrolled loop) -- for narrow levels under
// concurrent HBM traffic, where a load's latency exceeds two levels' time
template <int P, int LPR, bool W, int D>
__device__ __forceinline__ void sweep2_deep(Sw2Ctx &x, int64_t g0) {
    x.refill(g0);
    Sw2Slot<P> s[D + 1];
#pragma unroll
    for (int k = 0; k < D; ++k) sw2_issue<P, false>(x, g0 + k, s[k]);
    for (int64_t g = g0;;) {
#pragma unroll
        for (int k = 0; k <= D; ++k) {
            sw2_level<P, LPR, W, false, D>(x, g, s[k], s[(k + D) % (D + 1)]);
            if (++g >= x.g1) return;
        }
    }
}

template <int P, int LPR, bool W, bool R, int D = 2>
__device__ __forceinline__ void sweep2(Sw2Ctx &x, int64_t g0) {
    if (D != 2 && !R) {
        sweep2_deep<P, LPR, W, D>(x, g0);
        return;
    }
    x.refill(g0);
    Sw2Slot<P> s0, s1, s2;
    sw2_issue<P, R>(x, g0, s0);
    sw2_issue<P, R>(x, g0 + 1, s1);
    for (int64_t g = g0;;) {
        sw2_level<P, LPR, W, R>(x, g, s0, s2);
        if (++g >= x.g1) break;
        sw2_level<P, LPR, W, R>(x, g, s1, s0);
        if (++g >= x.g1) break;
        sw2_level<P, LPR, W, R>(x, g, s2, s1);
        if (++g >= x.g1) break;
    }
}

// Round-robin sweep for deep, narrow level DAGs (about one slice per level:
// FE rows in their natural order, e.g. the classical AMG's hybrid Gauss-Seidel
// chunks).  sweep2 gives every level to all waves and keeps two levels of
// factor data in flight, so with one slice per level one wave works, the rest
// idle at the barrier, and memory latency is exposed (footing N=128 smoother:
// ~0.77 us per level, 970 levels per 2,405-row chunk).  Here wave w owns the
// levels g0 + w, g0 + w + nw, ... and loads its next level's slice before
// computing the current one, so its data has nw levels' time to arrive.  A
// level's extra slices (rare) run inline.  Per-row sums are sweep2's (same
// entries, same order): results are bitwise those of sweep2.
// S > 1 (levels of a few slices: the pressure blocks of the headline's fp
// block, ~2 slices per level): groups of S waves own the levels round robin,
// wave k of a group the level's slice k, so data has nw / S levels to arrive.
template <int P, int LPR, bool W>
__device__ __forceinline__ void sweep_rr(Sw2Ctx &x, int64_t g0, int S = 1) {
    const int64_t g1 = x.g1;
    const int ng = x.nw / S, w = x.wave / S, ks = x.wave % S;  // level groups; this wave's group / slice
    const int nw = ng;
    const int64_t nown = g1 - g0 > w ? (g1 - g0 - w + nw - 1) / nw : 0;  // own levels of this wave
    int64_t jb = 0, ms0 = 0, ms1 = 0, mb = -1, me = -1;  // lane l: own level jb + l (first slice, end, entry range)
    auto refill = [&](int64_t j0) {
        jb = j0;
        const int64_t g = g0 + w + (j0 + x.lane) * nw;
        if (j0 + x.lane < nown) {
            ms0 = x.gslice[g];
            ms1 = x.gslice[g + 1];
            mb = ms1 > ms0 + ks ? x.sptr[ms0 + ks] : -1;
            me = ms1 > ms0 + ks ? x.sptr[ms0 + ks + 1] : -1;
        } else {
            ms0 = ms1 = 0;
            mb = me = -1;
        }
        asm volatile("" : "+v"(ms0), "+v"(ms1), "+v"(mb), "+v"(me));
    };
    auto issue = [&](int64_t j, Sw2Slot<P> &sl) {
        const int l = (int)(j - jb);
        const int64_t base = j < nown ? readlane64(mb, l) : -1;
        const int64_t next = base >= 0 ? readlane64(me, l) : 0;
        sl.base = base;
        sl.L = base >= 0 ? (next - base) >> 6 : 0;
        sl.l2 = 0;
#pragma unroll
        for (int u = 0; u <= P; ++u) {
            const int64_t pos = (base >= 0 ? base : 0) + (u < sl.L ? u : 0) * 64 + x.lane;
            sl.c[u] = base >= 0 ? __builtin_nontemporal_load(x.col + pos) : 0;
            sl.v[u] = base >= 0 ? __builtin_nontemporal_load(x.val + pos) : 0.0;
        }
    };
    auto compute = [&](int64_t j, const Sw2Slot<P> &cur) {
        if (cur.base < 0) return;
        const int32_t h = cur.c[0];
        const int32_t len = W ? (int32_t)cur.L - 1 : (int32_t)((uint32_t)h >> SW_ROW_BITS);
        double acc = 0.0, d[P + 1];
#pragma unroll
        for (int u = 1; u <= P; ++u) d[u] = sw2_dep<false>(x, u <= len ? cur.c[u] : 0);
#pragma unroll
        for (int u = 1; u <= P; ++u) {
            const double t = __dmul_rn(cur.v[u], d[u]);  // sweep2's rounding (no contraction)
            acc += (u <= len) ? t : 0.0;
        }
        for (int64_t k0 = P + 1; k0 < cur.L; k0 += 8) {
            int32_t cc[8];
            double vv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t k = k0 + u < cur.L ? k0 + u : cur.L - 1;
                cc[u] = __builtin_nontemporal_load(x.col + cur.base + k * 64 + x.lane);
                vv[u] = __builtin_nontemporal_load(x.val + cur.base + k * 64 + x.lane);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const double t = __dmul_rn(vv[u], sw2_dep<false>(x, k0 + u <= len ? cc[u] : 0));
                acc += (k0 + u <= len) ? t : 0.0;
            }
        }
        sw2_finish<LPR, W, false>(x, h, cur.v[0], acc);
        const int l = (int)(j - jb);
        const int64_t s0 = readlane64(ms0, l), s1 = readlane64(ms1, l);
        for (int64_t sl = s0 + ks + S; sl < s1; sl += S) sw2_slice_inline<LPR, W, false>(x, sl);
    };
    Sw2Slot<P> A, B;
    refill(0);
    issue(0, A);
    int64_t j = 0;
    for (int64_t g = g0; g < g1; ++g) {
        if ((g - g0) % nw == w) {
            if (j + 1 - jb >= 64) {  // keep the current level's metadata: refill from j
                refill(j);
            }
            // compute first: its wait covers only the slot loaded nw levels ago, not
            // the loads issued now for the next own level
            if ((j & 1) == 0) {
                compute(j, A);
                issue(j + 1, B);
            } else {
                compute(j, B);
                issue(j + 1, A);
            }
            ++j;
        }
        __syncthreads();
    }
}

template <int P, bool W, bool R = false, int D = 2>
__device__ __forceinline__ void sweep_block(int64_t g0, int64_t g1, int lpr, int lane, int wave, int nw, bool upper,
                                            const int64_t *__restrict__ gslice, const int64_t *__restrict__ sptr,
                                            const int32_t *__restrict__ col, const double *__restrict__ val,
                                            double *ys, double *ring = nullptr, double *ypos = nullptr,
                                            int64_t b0 = 0, int64_t ck0 = 0, int64_t ck1 = 0, RingIn rin = {},
                                            int rr = 0) {
    if (g0 >= g1) return;
    Sw2Ctx x{gslice, sptr, col, val, ys, g1, 0, 0, 0, 0, lane, wave, nw, upper,
             ring, ypos, 0, ck0, ck1, ck0 < ck1 ? rin.cg[ck0] : INT64_MAX, b0, ck0, rin};
    if (!R && rr) {  // deep, narrow levels: round-robin over groups of rr waves (a power of two <= nw)
        const int S = rr <= nw ? rr : nw;
        if (W) {
            if (lpr == 16) sweep_rr<P, 16, W>(x, g0, S);
            else if (lpr == 8) sweep_rr<P, 8, W>(x, g0, S);
            else if (lpr == 4) sweep_rr<P, 4, W>(x, g0, S);
            else if (lpr == 2) sweep_rr<P, 2, W>(x, g0, S);
            else sweep_rr<P, 1, W>(x, g0, S);
        } else {
            if (lpr == 4) sweep_rr<P, 4, W>(x, g0, S);
            else if (lpr == 2) sweep_rr<P, 2, W>(x, g0, S);
            else sweep_rr<P, 1, W>(x, g0, S);
        }
        return;
    }
    if (R) {  // ring sweep: lanes per row per slice
        sweep2<P, 0, true, true>(x, g0);
        if (ck1 > ck0) ring_flush(x, rin.cp[2 * ck1 - 2], rin.cp[2 * ck1 - 1]);  // the last chunk
        return;
    }
    if (W) {  // the y-resident sweep: 8 / 16 lanes for long rows
        if (lpr == 16) sweep2<P, 16, W, R, D>(x, g0);
        else if (lpr == 8) sweep2<P, 8, W, R, D>(x, g0);
        else if (lpr == 4) sweep2<P, 4, W, R, D>(x, g0);
        else if (lpr == 2) sweep2<P, 2, W, R, D>(x, g0);
        else sweep2<P, 1, W, R, D>(x, g0);
        return;
    }
    if (lpr == 4) sweep2<P, 4, W, R, D>(x, g0);
    else if (lpr == 2) sweep2<P, 2, W, R, D>(x, g0);
    else sweep2<P, 1, W, R, D>(x, g0);
}

static constexpr int SW_P = 7;  // factor entries per lane kept in registers per pipeline slot
// the ring sweep's slot and workgroup (measured: 512 threads with 15-entry
// slots, which hold the wider N=20 levels without in-level reloads, were
// slower at both N=12 (93 vs 138 it/s) and N=20 (16.6 vs 23.2))
static constexpr int RING_P = 7, RING_TPB = 1024;

// GMEM: the block solution lives in y itself (global memory) instead of LDS --
// blocks longer than the LDS holds, with the wide slice headers (W).  All waves of the workgroup share the CU's
// vector L1, so y written by one wave before __syncthreads() is seen by the
// others after it (workgroup-scope coherence, no cache maintenance needed).
// D: levels of factor data in flight (2; deeper with fewer threads: TPBMAX)
template <bool GMEM, int D = 2, int TPBMAX = 1024>
__global__ __launch_bounds__(TPBMAX) void k_ilu_blocks_lds(int64_t n, int64_t nblocks, const int64_t *__restrict__ Lgoff,
                                                         const int64_t *__restrict__ Lgslice,
                                                         const int64_t *__restrict__ Lsptr,
                                                         const int32_t *__restrict__ Lcol,
                                                         const double *__restrict__ Lval,
                                                         const int32_t *__restrict__ Llpr,
                                                         const int64_t *__restrict__ Ugoff,
                                                         const int64_t *__restrict__ Ugslice,
                                                         const int64_t *__restrict__ Usptr,
                                                         const int32_t *__restrict__ Ucol,
                                                         const double *__restrict__ Uval,
                                                         const int32_t *__restrict__ Ulpr, const double *x,
                                                         double *y, int64_t *__restrict__ prof, int rr,
                                                         const int64_t *__restrict__ bstart, int64_t blk_hi) {
    extern __shared__ __attribute__((aligned(16))) double lds_y[];
    // blocks [blk_hi - gridDim.x, blk_hi), the last (heaviest) first
    const int64_t blk = blk_hi - 1 - (int64_t)blockIdx.x;
    int64_t b0, len;
    block_range(blk, n, nblocks, bstart, b0, len);
    double *ys = GMEM ? y + b0 : lds_y;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    int64_t t0 = 0, t1 = 0;
    if (prof) t0 = wall_clock64();
    if (!GMEM || x != y)
        for (int64_t t = threadIdx.x; t < len; t += blockDim.x) ys[t] = x[b0 + t];
    __syncthreads();
    sweep_block<SW_P, GMEM, false, D>(Lgoff[blk], Lgoff[blk + 1], Llpr[blk], lane, wave, nw, false, Lgslice, Lsptr, Lcol,
                                      Lval, ys, nullptr, nullptr, 0, 0, 0, {}, rr);
    if (prof) t1 = wall_clock64();
    sweep_block<SW_P, GMEM, false, D>(Ugoff[blk], Ugoff[blk + 1], Ulpr[blk], lane, wave, nw, true, Ugslice, Usptr, Ucol,
                                      Uval, ys, nullptr, nullptr, 0, 0, 0, {}, rr);
    if (!GMEM)
        for (int64_t t = threadIdx.x; t < len; t += blockDim.x) y[b0 + t] = ys[t];
    if (prof && threadIdx.x == 0) {  // diagnostics (option pls.sweep_profile): 100 MHz wall clock
        int64_t *p = prof + blk * 8;
        p[0] = t0;
        p[1] = t1;
        p[2] = wall_clock64();
        p[3] = Lgoff[blk + 1] - Lgoff[blk];
        p[4] = Ugoff[blk + 1] - Ugoff[blk];
        p[5] = len;
        p[6] = Lgslice[Lgoff[blk + 1]] - Lgslice[Lgoff[blk]];
        p[7] = Llpr[blk] * 10 + Ulpr[blk];
    }
}

// The ring sweep (whole FE blocks in a bandwidth-reducing order: deep, narrow
// level DAGs whose dependencies are recent in level order): per block, the L
// sweep in L's level-order positions (inputs x[ordL]), outputs to yL (position
// order); the U sweep in U's positions (inputs yL[mapUL]), outputs to yU; then
// y[ordU[p]] = yU[p].  Dependency reads hit the LDS ring unless older than
// RING_SLOTS - RING_CHUNK positions (then yL / yU in global memory, written by
// this workgroup: workgroup-scope coherence as in the y-resident sweep), and
// those "far" dependencies are known at setup: they are taken out of the
// factor streams and subtracted from the row's input when its chunk loads.
__global__ __launch_bounds__(RING_TPB) void k_ilu_blocks_ring(
    int64_t n, int64_t nblocks, const int64_t *__restrict__ Lgoff, const int64_t *__restrict__ Lgslice,
    const int64_t *__restrict__ Lsptr, const int32_t *__restrict__ Lcol, const double *__restrict__ Lval,
    const int32_t *__restrict__ Llpr, const int64_t *__restrict__ Ugoff, const int64_t *__restrict__ Ugslice,
    const int64_t *__restrict__ Usptr, const int32_t *__restrict__ Ucol, const double *__restrict__ Uval,
    const int32_t *__restrict__ Ulpr, const int64_t *__restrict__ Lcoff, const int64_t *__restrict__ Lcg,
    const int64_t *__restrict__ Lcp, const int64_t *__restrict__ Ucoff, const int64_t *__restrict__ Ucg,
    const int64_t *__restrict__ Ucp, const int32_t *__restrict__ ordL, const int32_t *__restrict__ mapUL,
    const int32_t *__restrict__ ordU, const int64_t *__restrict__ Lfrp, const int32_t *__restrict__ Lfcol,
    const double *__restrict__ Lfval, const int64_t *__restrict__ Ufrp, const int32_t *__restrict__ Ufcol,
    const double *__restrict__ Ufval, const double *x, double *y, double *yL, double *yU,
    const int64_t *__restrict__ bstart) {
    extern __shared__ __attribute__((aligned(16))) double ring[];
    const int64_t blk = nblocks - 1 - (int64_t)blockIdx.x;
    int64_t b0, len;
    block_range(blk, n, nblocks, bstart, b0, len);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    sweep_block<RING_P, true, true>(Lgoff[blk], Lgoff[blk + 1], Llpr[blk], lane, wave, nw, false, Lgslice, Lsptr, Lcol,
                                  Lval, nullptr, ring, yL + b0, b0, Lcoff[blk], Lcoff[blk + 1],
                                  RingIn{Lcg, Lcp, ordL, x, Lfrp, Lfcol, Lfval});
    __syncthreads();
    sweep_block<RING_P, true, true>(Ugoff[blk], Ugoff[blk + 1], Ulpr[blk], lane, wave, nw, true, Ugslice, Usptr, Ucol,
                                  Uval, nullptr, ring, yU + b0, b0, Ucoff[blk], Ucoff[blk + 1],
                                  RingIn{Ucg, Ucp, mapUL, yL, Ufrp, Ufcol, Ufval});
    __syncthreads();
    for (int64_t t = threadIdx.x; t < len; t += blockDim.x) y[ordU[b0 + t]] = yU[b0 + t];
}

void launch_ilu_blocks_ring(int64_t n, int64_t nblocks, const int64_t *Lgoff, const int64_t *Lgslice,
                            const int64_t *Lsptr, const int32_t *Lcol, const double *Lval, const int32_t *Llpr,
                            const int64_t *Ugoff, const int64_t *Ugslice, const int64_t *Usptr, const int32_t *Ucol,
                            const double *Uval, const int32_t *Ulpr, const int64_t *Lcoff, const int64_t *Lcg,
                            const int64_t *Lcp, const int64_t *Ucoff, const int64_t *Ucg, const int64_t *Ucp,
                            const int32_t *ordL, const int32_t *mapUL, const int32_t *ordU, const int64_t *Lfrp,
                            const int32_t *Lfcol, const double *Lfval, const int64_t *Ufrp, const int32_t *Ufcol,
                            const double *Ufval, const double *x, double *y, double *yL, double *yU, hipStream_t st,
                            int tpb, const int64_t *bstart) {
    if (tpb < 64 || tpb > RING_TPB || (tpb & 63)) tpb = RING_TPB;
    static bool configured = false;
    const int bytes = RING_SLOTS * 8;
    if (!configured) {
        (void)hipFuncSetAttribute((const void *)k_ilu_blocks_ring, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        configured = true;
    }
    k_ilu_blocks_ring<<<(unsigned)nblocks, tpb, bytes, st>>>(n, nblocks, Lgoff, Lgslice, Lsptr, Lcol, Lval, Llpr,
                                                               Ugoff, Ugslice, Usptr, Ucol, Uval, Ulpr, Lcoff, Lcg, Lcp,
                                                               Ucoff, Ucg, Ucp, ordL, mapUL, ordU, Lfrp, Lfcol, Lfval,
                                                               Ufrp, Ufcol, Ufval, x, y, yL, yU, bstart);
}
int ilu_ring_slots() { return RING_SLOTS; }
int ilu_ring_lane_entries() { return RING_P; }
int ilu_ring_chunk() { return RING_CHUNK; }

int ilu_lds_max_rows() { return 163840 / 8; }
int ilu_gmem_max_rows() { return 0x7FFFFFFF; }
int ilu_lds_lane_entries() { return SW_P; }

void launch_ilu_blocks_lds(int64_t n, int64_t nblocks, const int64_t *Lgoff, const int64_t *Lgslice,
                           const int64_t *Lsptr, const int32_t *Lcol, const double *Lval, const int32_t *Llpr,
                           const int64_t *Ugoff, const int64_t *Ugslice, const int64_t *Usptr, const int32_t *Ucol,
                           const double *Uval, const int32_t *Ulpr, const double *x, double *y, hipStream_t st,
                           int64_t *prof, bool gmem, int tpb, int rr, const int64_t *bstart, int64_t max_len,
                           int64_t blk_lo, int64_t blk_hi, int depth) {
    // tpb: threads per workgroup, 64 .. 1024 (narrow levels: fewer waves, cheaper barriers)
    if (tpb < 64 || tpb > 1024 || (tpb & 63)) tpb = 1024;
    // block subset [blk_lo, blk_hi) (blk_hi < 0: every block)
    if (blk_hi < 0) {
        blk_lo = 0;
        blk_hi = nblocks;
    }
    if (blk_lo < 0 || blk_hi > nblocks || blk_lo >= blk_hi) return;
    const unsigned grid = (unsigned)(blk_hi - blk_lo);
    static bool configured = false;
    if (!configured) {
        (void)hipFuncSetAttribute((const void *)k_ilu_blocks_lds<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)163840);
        configured = true;
    }
    if (gmem) {
        k_ilu_blocks_lds<true><<<grid, tpb, 0, st>>>(n, nblocks, Lgoff, Lgslice, Lsptr, Lcol, Lval, Llpr, Ugoff, Ugslice,
                                                     Usptr, Ucol, Uval, Ulpr, x, y, prof, rr, bstart, blk_hi);
        return;
    }
    const size_t bytes = (size_t)(max_len > 0 ? max_len : n / nblocks + 1) * 8;
    if ((depth == 3 || depth == 4) && rr == 0) {  // 3 / 4 levels in flight on up to 16 waves (pls.sweep_depth)
        static bool conf34 = false;
        if (!conf34) {
            (void)hipFuncSetAttribute((const void *)k_ilu_blocks_lds<false, 3, 1024>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)163840);
            (void)hipFuncSetAttribute((const void *)k_ilu_blocks_lds<false, 4, 1024>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)163840);
            conf34 = true;
        }
        if (depth == 3)
            k_ilu_blocks_lds<false, 3, 1024><<<grid, tpb, bytes, st>>>(n, nblocks, Lgoff, Lgslice, Lsptr, Lcol, Lval,
                                                                       Llpr, Ugoff, Ugslice, Usptr, Ucol, Uval, Ulpr,
                                                                       x, y, prof, rr, bstart, blk_hi);
        else
            k_ilu_blocks_lds<false, 4, 1024><<<grid, tpb, bytes, st>>>(n, nblocks, Lgoff, Lgslice, Lsptr, Lcol, Lval,
                                                                       Llpr, Ugoff, Ugslice, Usptr, Ucol, Uval, Ulpr,
                                                                       x, y, prof, rr, bstart, blk_hi);
        return;
    }
    if (depth == 6 && tpb <= 512 && rr == 0) {  // 6 levels in flight, at most 8 waves (register room)
        static bool conf6 = false;
        if (!conf6) {
            (void)hipFuncSetAttribute((const void *)k_ilu_blocks_lds<false, 6, 512>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)163840);
            conf6 = true;
        }
        k_ilu_blocks_lds<false, 6, 512><<<grid, tpb, bytes, st>>>(n, nblocks, Lgoff, Lgslice, Lsptr, Lcol, Lval, Llpr,
                                                                 Ugoff, Ugslice, Usptr, Ucol, Uval, Ulpr, x, y, prof,
                                                                 rr, bstart, blk_hi);
        return;
    }
    k_ilu_blocks_lds<false><<<grid, tpb, bytes, st>>>(n, nblocks, Lgoff, Lgslice, Lsptr, Lcol, Lval, Llpr, Ugoff,
                                                        Ugslice, Usptr, Ucol, Uval, Ulpr, x, y, prof, rr, bstart, blk_hi);
}

// Additive Schwarz over LDS-resident subdomains (PCASM, asm.cpp): k_ilu_blocks_lds<false> with the
// gather and the restricted scatter in the workgroup.  Block blk's extended rows are
// [bstart[blk], bstart[blk + 1]); extended row e is global row gidx[e], own[e] = 1 where the block
// owns it.  Load: ys[t] = x[gidx[e]], 0.0 where the type masks the input and the row is not
// owned.  The sweeps are sweep_block's, with k_ilu_blocks_lds's arguments: the same bits.  Store:
// direct -- owned rows to y[gidx[e]] (every global row has exactly one owner: no race, no
// atomics); else every row to y[e], the extended vector that k_asm_combine sums.  x must not be
// y when direct: another workgroup reads the overlap rows this one overwrites (PCASM copies x).
// gidx and own lie inside [0, n) / the extended range by construction (k_asm_grow).
__global__ __launch_bounds__(1024) void k_asm_blocks_lds(
    int64_t nblocks, const int64_t *__restrict__ bstart, const int64_t *__restrict__ Lgoff,
    const int64_t *__restrict__ Lgslice, const int64_t *__restrict__ Lsptr, const int32_t *__restrict__ Lcol,
    const double *__restrict__ Lval, const int32_t *__restrict__ Llpr, const int64_t *__restrict__ Ugoff,
    const int64_t *__restrict__ Ugslice, const int64_t *__restrict__ Usptr, const int32_t *__restrict__ Ucol,
    const double *__restrict__ Uval, const int32_t *__restrict__ Ulpr, const int32_t *__restrict__ gidx,
    const uint8_t *__restrict__ own, int mask_in, int direct, const double *__restrict__ x, double *__restrict__ y,
    int rr) {
    extern __shared__ __attribute__((aligned(16))) double lds_y[];
    const int64_t blk = nblocks - 1 - (int64_t)blockIdx.x;
    const int64_t b0 = bstart[blk], len = bstart[blk + 1] - b0;
    double *ys = lds_y;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    for (int64_t t = threadIdx.x; t < len; t += blockDim.x) {
        const int64_t e = b0 + t;
        ys[t] = (mask_in && !own[e]) ? 0.0 : x[gidx[e]];
    }
    __syncthreads();
    sweep_block<SW_P, false, false, 2>(Lgoff[blk], Lgoff[blk + 1], Llpr[blk], lane, wave, nw, false, Lgslice, Lsptr,
                                       Lcol, Lval, ys, nullptr, nullptr, 0, 0, 0, {}, rr);
    sweep_block<SW_P, false, false, 2>(Ugoff[blk], Ugoff[blk + 1], Ulpr[blk], lane, wave, nw, true, Ugslice, Usptr,
                                       Ucol, Uval, ys, nullptr, nullptr, 0, 0, 0, {}, rr);
    for (int64_t t = threadIdx.x; t < len; t += blockDim.x) {
        const int64_t e = b0 + t;
        if (!direct) y[e] = ys[t];
        else if (own[e]) y[gidx[e]] = ys[t];
    }
}

void launch_asm_blocks_lds(int64_t nblocks, const int64_t *bstart, int64_t max_len, const int64_t *Lgoff,
                           const int64_t *Lgslice, const int64_t *Lsptr, const int32_t *Lcol, const double *Lval,
                           const int32_t *Llpr, const int64_t *Ugoff, const int64_t *Ugslice, const int64_t *Usptr,
                           const int32_t *Ucol, const double *Uval, const int32_t *Ulpr, const int32_t *gidx,
                           const uint8_t *own, int mask_in, int direct, const double *x, double *y, int tpb, int rr,
                           hipStream_t st) {
    if (nblocks <= 0) return;
    if (tpb < 64 || tpb > 1024 || (tpb & 63)) tpb = 1024;
    static bool configured = false;
    if (!configured) {
        (void)hipFuncSetAttribute((const void *)k_asm_blocks_lds, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)163840);
        configured = true;
    }
    const size_t bytes = (size_t)max_len * 8;  // (PCASM: max_len <= ilu_lds_max_rows(), the inner sweep is Lds)
    k_asm_blocks_lds<<<(unsigned)nblocks, tpb, bytes, st>>>(nblocks, bstart, Lgoff, Lgslice, Lsptr, Lcol, Lval, Llpr,
                                                            Ugoff, Ugslice, Usptr, Ucol, Uval, Ulpr, gidx, own,
                                                            mask_in, direct, x, y, rr);
}

}  // namespace pls
