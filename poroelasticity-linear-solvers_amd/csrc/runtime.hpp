// runtime.hpp -- host runtime of libpls.so: device memory, options database,
// operators, preconditioners, Krylov solvers, the block preconditioner and
// AAR.  Every vector operation is a HIP kernel on one stream over
// device-resident vectors.  GMRES / FGMRES run their loop on the host and read
// back the handful of scalars the PETSc algorithm branches on per iteration
// (Hessenberg column, norms); CG and BiCGStab keep their scalar recurrences on
// the device and read back (done, its, reason) once per batch of iterations,
// with host-driven loops for the monitor and the time limit (ksp.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <map>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "comm.hpp"
#include "kernels.hpp"

namespace pls {

struct Error : std::runtime_error {
    explicit Error(const std::string &m) : std::runtime_error(m) {}
};

#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess)                                                                       \
            throw ::pls::Error(std::string(#x) + " failed: " + hipGetErrorString(e_) + " at " +    \
                               __FILE__ + ":" + std::to_string(__LINE__));                          \
    } while (0)

// ------------------------------------------------------------ device buffer --
template <class T>
struct DBuf {
    T *p = nullptr;
    size_t n = 0;
    DBuf() = default;
    explicit DBuf(size_t count) { alloc(count); }
    DBuf(const DBuf &) = delete;
    DBuf &operator=(const DBuf &) = delete;
    DBuf(DBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DBuf &operator=(DBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~DBuf() { release(); }
    void alloc(size_t count) {
        release();
        n = count;
        if (count) HIPCHK(hipMalloc((void **)&p, sizeof(T) * count));
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    T *get() const { return p; }
};

// ------------------------------------------------------------------ context --
struct Ctx {
    hipStream_t st = nullptr;
    Comm *comm = nullptr;   // global reductions (CommSelf unless distributed)
    DBuf<double> partial;   // reduction partials (NB_MAX (4096) x 136 at first; ensure_partial grows it)
    int64_t partial_n = 0;
    int64_t hscal_n = 0;    // doubles in the pinned host mirror
    DBuf<double> dscal;     // device scalars
    double *hscal = nullptr;  // pinned host mirror
    bool sell_d16 = true;     // build SpMV layouts as SELL-64/D16 where every row fits
    int d16_wide_lpr = 8;     // lanes per row of D16 slices with wide rows (option pls.d16_wide_lpr)
    int d16_unroll = 4;       // D16 SpMV 8-entry groups per lane in flight (option pls.d16_unroll)
    int d16_xcd = 0;          // D16 SpMV workgroup -> slice order: 1 XCD-contiguous ranges (option pls.d16_xcd)
    int d16_share = -1;       // shared delta streams: -1 where they pay (see below), 0 never, 1 always (pls.d16_share)
    int64_t d16_share_min_bytes = 268435456;  // ... -1: only layouts above this size (pls.d16_share_min_bytes)
    int64_t d16_share_built = 0;              // D16 layouts built with a shared delta stream so far
    int reuse_wide = -1;      // coupling reuse on rows of several lanes: -1 wherever the reuse is eligible, 0 never (pls.reuse_wide)
    int d16_unroll_single = 8;  // ... of the fp32-value kernel: 1, 2, 4 or 8 (option pls.d16_unroll_single)
    int d16_segs = D16_SEG;   // minimum D16 segment bases per lane (option pls.d16_segs; 8 where needed)
    int d16_sigma = 1024;         // SELL-C-sigma window (rows sorted by length; 0: never) (pls.d16_sigma)
    double d16_sigma_pad = 0.15;  // ... used when the plain plan pads more than this fraction (pls.d16_sigma_pad)
    int d16_sorted_lpr = 2;       // lanes per row of sorted slices with 32+ entries per row (pls.d16_sorted_lpr)
    bool spmv_b3 = false;         // row-triple layout for FE vector fields (pls.spmv_b3; measured slower)
    int spmv_rcm = -1;            // RCM-relabelled SpMV layout: -1 where the plain plan pads (FE), 0 never, 1 always
    int sweep_chain = -1;         // LDS-resident ILU / Gauss-Seidel blocks swept by one wave (k_ilu_blocks_chain):
                                  // -1 where the level DAG is deep and narrow, 0 never, 1 whenever rows fit
    int sweep_window = -1;        // ... in 64-row windows with inverted window triangles (k_ilu_blocks_window):
                                  // -1 where the chain sweep would be chosen, 0 never, 1 whenever rows fit
    int ilu_factor_dep = 1;       // ILU(0) factorization in one dependency-driven launch: 1 narrow levels, 2 always, 0 never
    int ilu_view = 0;             // print every ILU / Gauss-Seidel PC's sweep choice to stderr (pls.ilu_view)
    int ilu0_stage_cap = -1;      // test knob (pls.ilu0_stage): staged entries of the ILU(0) factorization, -1 default
    int ilu_dep_grid = 0;         // test knob (pls.ilu_dep_grid): k_ilu0_dep's persistent grid capped (0: none)
    int window_depth = 2;         // window sweep: windows of data in flight, 2 or 3 (pls.window_depth)
    int window_ring = -1;         // ... its ring variant for blocks longer than LDS (pls.window_ring: -1 where the
                                  // window sweep's level test holds, 0 off, 1 also forced on LDS-resident blocks)
    int window_kpw = 0;           // window sweep: stream records per wave (pls.window_kpw: 0 by the rows, 8 forced)
    int window_mixed = -1;        // ... its L triangle by levels (pls.window_mixed: -1 where L has no more levels
                                  // than windows, 0 off, 1 forced)
    int sweep_swin = 0;           // blocks too long for LDS: the super-window sweep (k_ilu_blocks_swin, experimental,
                                  // measured slower than the ring sweep): 0 never (default, capi), -1 where the ring
                                  // sweep would run, 1 whenever the block is y-resident
    double amg_csr_below = 16.0;  // AMG operators with fewer entries per row than this stay CSR (pls.amg_csr_below)
    bool halo_overlap = true;     // distributed SpMV: interior slices overlap the halo exchange (pls.halo_overlap)
    hipStream_t st_comm = nullptr;  // stream of the overlapped halo exchange (created on first use)
    hipEvent_t ev_x = nullptr, ev_halo = nullptr;
    DBuf<char> scan_tmp;
    size_t scan_tmp_bytes = 0;
    DBuf<double> rcm_x;  // x in RCM order for RCM-relabelled SpMV layouts (grown at layout build)
    // a redundant PC's gathered block: the rows each rank owns (contiguous, rank
    // order; empty when not) -- the classical AMG builds hypre's np = G hierarchy
    std::vector<int64_t> rank_rows;
    Ctx();
    ~Ctx();
    void sync() { HIPCHK(hipStreamSynchronize(st)); }
    void ensure_scan(int64_t n);
    // room for `cols` reductions of n entries (CGS: one partial per column and block) and
    // for `cols` + 2 doubles in the host mirror; setup only (frees the old buffers)
    void ensure_partial(int64_t n, int64_t cols);
    // every launch that writes `partial` / `hscal` takes its pointer from these:
    // they throw Error when the request exceeds the room (the round-3 fault was a
    // silent overrun of `partial` by a 453-column CGS block)
    double *partials(int64_t n, int64_t cols);
    double *host_scalars(int64_t count);
    // pls.debug_bounds: a canary region behind `partial` (checked by check_bounds,
    // which throws Error when it was written); pls.debug_partial_cap /
    // pls.debug_no_grow / pls.debug_unguarded reproduce the round-3 overrun in tests
    bool debug_bounds = false, debug_no_grow = false, debug_unguarded = false;
    static constexpr int64_t CANARY = 1 << 16;
    void set_debug(bool bounds, int64_t cap, bool no_grow, bool unguarded);
    void check_bounds();
    // deterministic reductions returning host values (synchronising)
    double dot(int64_t n, const double *x, const double *y);
    double norm2(int64_t n, const double *x);
};

// ------------------------------------------------------------------ matrix --
struct DevSELL {
    int64_t nslices = 0, stored = 0;  // stored = padded entries
    bool d16 = false;                 // SELL-64/D16: 16-bit column deltas (dl, seg) instead of col
    DBuf<int64_t> sptr;
    DBuf<int32_t> col;
    DBuf<double> val;
    DBuf<uint16_t> dl;
    // shared delta stream (pls.d16_share; kernels.hip): dl holds one pack per class and 8-entry
    // group, dstored deltas in all, addressed through dptr (nslices + 1) and cls (nslices * 64);
    // both empty and dstored == stored: one pack per lane
    DBuf<int64_t> dptr;
    DBuf<uint8_t> cls;
    int64_t dstored = 0, shared_slices = 0;  // stored deltas; slices with fewer than 64 classes
    DBuf<int32_t> seg, slpr;  // D16: segment bases per lane, lanes per row per slice
    DBuf<int64_t> sfirst;     // D16: first row of each slice (nslices + 1)
    int64_t wide_slices = 0;  // D16 slices with 8 lanes per row
    // SELL-C-sigma: slice positions hold rows sorted by length inside windows of
    // sigma rows (rowmap[position] = row); empty when rows keep their order
    DBuf<int32_t> rowmap;
    int64_t nrows_mapped = 0;
    // SELL/B3 (FE vector fields): row triples with one shared column list, lane =
    // triple; the D16 part above then holds only the other rows (through rowmap)
    int64_t b3_nslices = 0, b3_ntrip = 0, b3_stored = 0;
    DBuf<int64_t> b3ptr;
    DBuf<int32_t> b3map, b3col;
    DBuf<double> b3val;
    int nsegs = D16_SEG;      // D16 segment bases per lane: 4, or 8 when halo columns need them
    // distributed products: slices without / with ghost columns (the first
    // run while the halo exchange is in flight)
    DBuf<int32_t> s_in, s_halo;
    int64_t n_in = 0, n_halo = 0;
    // RCM-relabelled columns (FE matrices, pls.spmv_rcm): the product reads
    // xp = x[xperm] (Ctx::rcm_x) so a slice's gathers stay local
    int64_t nperm = 0;
    DBuf<int32_t> xperm;
    // Compressed-operator GMRES (pls_gmres_operator single): the D16 values once more, rounded to
    // fp32, val32[base + (k / 4) * 256 + lane * 4 + k % 4] (build_low; empty until a KSP asks)
    DBuf<float> val32;
    D16Streams streams() const { return {sptr.p, sfirst.p, slpr.p, dl.p, seg.p, nsegs, dptr.p, cls.p}; }  // (D16 layouts)
    bool has_low() const { return d16 && !b3_nslices && val32.p != nullptr; }
    int64_t low_stream_bytes() const { return has_low() ? stored * 4 : 0; }
    int64_t bytes_low() const { return bytes() - stored * 4; }  // bytes one low product streams (D16 only)
    int64_t bytes() const {  // bytes one product streams from the matrix
        return (d16 ? stored * 8 + dstored * 2 + (cls.p ? nslices * 72 + 8 : 0) + nslices * (64 * 4 * nsegs + 20) + 8 +
                          nrows_mapped * 4
                    : stored * 12 + (nslices + 1) * 8) +
               b3_stored * 28 + b3_ntrip * 4 + (b3_nslices + 1) * 8 + nperm * 20;
    }
};

// Halo of a distributed matrix: columns >= nlocal are ghosts (entries owned by
// other ranks, ordered owner-major); before each product the owned entries
// other ranks need are packed and exchanged into `ghost`.
struct Halo {
    int64_t nlocal = 0, nghost = 0, nsend = 0;
    // block-global index of every local column (owned [0, nlocal), then the
    // ghosts); for a diagonal block also of every local row (host, setup only)
    std::vector<int64_t> l2g;
    DBuf<int32_t> send_idx;
    DBuf<double> sendbuf, ghost;
    std::vector<int64_t> scnt, soff, rcnt, roff;
};

struct DevCSR {
    int64_t nrows = 0, ncols = 0, nnz = 0;
    std::shared_ptr<Halo> halo;     // distributed matrices only
    DBuf<int64_t> rp;
    DBuf<int32_t> ci;
    DBuf<double> val;
    int64_t max_row = 0;
    std::unique_ptr<DevSELL> sell;  // SpMV layout (built on demand)
    int tag = 0;                    // 1: outer operator A
    bool rcm_auto = true;           // pls.spmv_rcm -1 may relabel this matrix (not AMG level operators)
};
// Build the SELL-64 copy used by every SpMV with this matrix.
void build_sell(DevCSR &M, Ctx &c);

void upload_csr(DevCSR &M, int64_t nrows, int64_t ncols, const int64_t *rp, const int32_t *ci, const double *val,
                Ctx &c);
// Extract rows [r0, r1) with a column window (see WindowSpec), columns shifted.
void extract_csr(const DevCSR &src, int64_t r0, int64_t r1, WindowSpec w, int64_t cshift, int64_t ncols,
                 DevCSR &dst, Ctx &c);
// Distributed D16 matrices: split the slices into interior / halo lists (the
// product overlaps the halo exchange with the interior slices).  build_sell
// calls it for matrices with a halo.
void classify_halo_slices(DevCSR &M, Ctx &c);
// low: the D16 kernel over the layout's fp32 value stream (build_low first), x and sums fp64
void spmv(const DevCSR &M, const double *x, double *y, Ctx &c, double alpha = 1.0, double beta = 0.0,
          const double *z = nullptr, bool low = false);
// The fp32 value stream of a D16 layout, from its fp64 stream on the device (a no-op when it
// exists).  Throws, naming `who` and the condition, when the layout is not SELL-64/D16, has a B3
// part, or holds a finite value whose fp32 rounding is infinite.
void build_low(DevSELL &S, Ctx &c, const std::string &who);
// qout (plain D16 layouts): also qout[row] = the raw row sum, before alpha and beta, for the
// rows of lane-per-row slices (launch_d16_spmv's D16_AUX_STORE)
void spmv_slices(const DevCSR &M, const double *x, double *y, Ctx &c, double alpha, double beta, const double *z,
                 const int32_t *slist, int64_t count, size_t lds_reserve = 0, double *qout = nullptr,
                 const D16Wide &W = D16Wide());
void spmv_store_sums(const DevCSR &M, const double *x, double *y, Ctx &c, double alpha, double beta, const double *z,
                     double *qout, const D16Wide &W = D16Wide());
// true when M's layout is the plain D16 one (no halo, RCM relabelling, row triples or row map)
bool plain_d16(const DevCSR &M);

// Host copy of a CSR matrix (setup-time algebra: fieldsplit blocks, AMG hierarchy).
// std::allocator whose value-initialisation is default-initialisation: a
// resize(n) of a host matrix array leaves it unwritten (its writer fills it,
// on as many threads as it likes) instead of zeroing GBs on one thread
// Arrays of 2 MB and more are mapped on their own with MADV_HUGEPAGE (the
// boxes run transparent huge pages in madvise mode): the setup's random
// accesses over GB-sized host matrices (the Galerkin product's P rows, the
// first pass's lambda array) otherwise miss the TLB on 4 KB pages, and a
// first touch costs one fault per 4 KB.
void *huge_alloc(size_t bytes);
void huge_free(void *p, size_t bytes);
static constexpr size_t HUGE_ALLOC_MIN = (size_t)2 << 20;
template <class T>
struct NoInitAlloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = NoInitAlloc<U>;
    };
    NoInitAlloc() = default;
    template <class U>
    NoInitAlloc(const NoInitAlloc<U> &) noexcept {}
    T *allocate(size_t n) {
        if (n * sizeof(T) >= HUGE_ALLOC_MIN) return static_cast<T *>(huge_alloc(n * sizeof(T)));
        return std::allocator<T>::allocate(n);
    }
    void deallocate(T *p, size_t n) noexcept {
        if (n * sizeof(T) >= HUGE_ALLOC_MIN) huge_free(p, n * sizeof(T));
        else std::allocator<T>::deallocate(p, n);
    }
    template <class U>
    void construct(U *p) noexcept {
        ::new ((void *)p) U;
    }
    template <class U, class... Args>
    void construct(U *p, Args &&...args) {
        ::new ((void *)p) U(std::forward<Args>(args)...);
    }
};
template <class T>
using hvec = std::vector<T, NoInitAlloc<T>>;

struct HostCSR {
    int64_t nrows = 0, ncols = 0;
    hvec<int64_t> rp{0};
    hvec<int32_t> ci;
    hvec<double> v;
};
HostCSR download(const DevCSR &M, Ctx &c);
void upload(const HostCSR &H, DevCSR &M, Ctx &c);

// ----------------------------------------------------------------- options --
struct Options {
    std::map<std::string, std::string> kv;
    void parse(const char *text);
    bool has(const std::string &k) const { return kv.count(k) > 0; }
    std::string str(const std::string &k, const std::string &d) const;
    double num(const std::string &k, double d) const;
    int64_t integer(const std::string &k, int64_t d) const;
    bool flag(const std::string &k, bool d) const;
};

// -------------------------------------------------------------- timer pool --
enum TimerCat { T_PC_TOTAL = 0, T_PC_SOLID, T_PC_FLUID, T_PC_PRESS, T_PC_ALLOC, T_SOLVER, T_SPMV, T_NCAT };
struct Timers {
    // an interval on any stream, outside the begin / end nesting (see add)
    struct Span { hipEvent_t a = nullptr, b = nullptr; };
    double acc[T_NCAT] = {0};
    int64_t spmv_calls = 0;
    bool enabled = true;
    std::vector<hipEvent_t> pool;
    struct Pending { int cat; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<int> open_stack;
    std::vector<hipEvent_t> open_ev;
    size_t next = 0;
    hipStream_t st = nullptr;
    ~Timers();
    hipEvent_t ev();
    void begin(int cat);
    void end(int cat);
    void flush();  // call after a stream sync
    void reset() { for (double &a : acc) a = 0; spmv_calls = 0; }
    // Non-nesting intervals: mark(s) records an event of the pool on stream s; add(cat, span)
    // counts the time between two marks into cat at the next flush.  A span is valid until
    // that flush (`flushes` tells: the pool's events are handed out again after it).
    hipEvent_t mark(hipStream_t s);
    void add(int cat, Span sp) { if (enabled && sp.a && sp.b) pending.push_back({cat, sp.a, sp.b}); }
    int64_t flushes = 0;
};

// ------------------------------------------- coupling reuse (outer product) --
// Right-preconditioned GMRES forms w = A z directly after z = M^-1 v.  The 2-way block PC has
// then just multiplied its coupling block P_fp,s with z_s; where that block is A's own
// (rows [ns, n) x columns [0, ns), bitwise), the PC's launches also store their raw row sums
// q, and the outer product runs over `reduced` -- A without those entries on the reuse rows
// -- starting each such row's sum from q.  Same chain of operations per row as the full
// product, so the same bits ("Coupling reuse").  Owned by the handle; the block PC
// writes q and the spans, MatOp consumes them.
struct Coupling {
    bool eligible = false;     // decided at setup and after every matrix update
    std::string why;           // ... and why not
    DevSELL reduced;           // second D16 layout of the outer operator (A's slice plan)
    int64_t reuse_rows = 0;
    std::vector<uint8_t> reuse;  // per row (internal order): 1 on the reuse rows (empty: not eligible)
    DBuf<double> q;            // n: raw sums on the reuse rows; zero wherever the reduced launch reads it else
    // Wide reuse rows: rows of wlpr > 1 lanes in A's plan and in M's (pls.reuse_wide).  qw holds
    // the raw sum of every lane of the rows [wlo, whi) of A, (row - wlo) * wlpr + lane of the row;
    // zeroed once: a lane without s-entries, and a row of the range that is wide in A only, read
    // the zero.  wide(shift): the launch argument in the row numbering of A (0) or of M (ns).
    DBuf<double> qw;
    int64_t wide_rows = 0, wlo = 0, whi = 0;
    int wlpr = 0;
    D16Wide wide(int64_t shift) const {
        D16Wide W;
        if (eligible && wide_rows > 0) W = D16Wide{qw.p, wlo - shift, whi - shift, wlpr};
        return W;
    }
    const double *fresh_for = nullptr;  // the z the PC returned last, while q belongs to it
    std::vector<Timers::Span> spans;    // the PC's coupling launches of that application
    int64_t spans_flush = -1;
    int64_t n_reduced = 0, n_full = 0;  // outer products since the last reset
};
// Decide the layout-level conditions and build `reduced` and q: both layouts plain D16, A's
// coupling entries bitwise those of M (device comparison).  Returns false with R.why set.
bool build_coupling(const DevCSR &A, int64_t ns, const DevCSR &M, Coupling &R, Ctx &c);

// --------------------------------------------------------------- operators --
struct PC;
struct Op {
    int64_t n = 0;
    virtual ~Op() = default;
    virtual void apply(const double *x, double *y, Ctx &c) = 0;
    // y = A x for the x that pc.apply() has just returned: an operator that shares work with
    // that application (MatOp with a Coupling) may continue it
    virtual void apply_after(const PC &pc, const double *x, double *y, Ctx &c) { apply(x, y, c); }
    // r = b - A x (r is neither x nor b); a matrix does it in the product's launch
    virtual void residual(const double *x, const double *b, double *r, Ctx &c);
    // Compressed-operator GMRES: y = A^ x with the operator's low-precision copy (MatOp: the
    // stored values rounded to fp32 once; x, y and every sum fp64), and its apply_after
    virtual bool has_low() const { return false; }
    virtual void apply_low(const double *x, double *y, Ctx &c);
    virtual void apply_after_low(const PC &pc, const double *x, double *y, Ctx &c);
};
struct MatOp : Op {
    const DevCSR *M;
    Timers *timers = nullptr;
    explicit MatOp(const DevCSR *m) : M(m) { n = m->nrows; }
    Ctx *ctx_for_build = nullptr;
    Coupling *coupling = nullptr;  // the outer operator's (counts its products; reduced ones where eligible)
    void apply(const double *x, double *y, Ctx &c) override;
    void apply_after(const PC &pc, const double *x, double *y, Ctx &c) override;
    void residual(const double *x, const double *b, double *r, Ctx &c) override;
    // low: a KSP with pls_gmres_operator single uses this operator (enable_low: the layout and its
    // fp32 stream now, with the refusals; after a matrix update the streams are rebuilt on demand)
    bool low = false;
    void enable_low(Ctx &c, const std::string &who);
    bool has_low() const override { return low; }
    void apply_low(const double *x, double *y, Ctx &c) override;
    void apply_after_low(const PC &pc, const double *x, double *y, Ctx &c) override;
    int64_t low_bytes() const;  // bytes of the fp32 streams held: the layout's and the coupling's reduced one
private:
    // the bodies of apply / apply_low and apply_after / apply_after_low: timers, spans, fresh_for
    // and the coupling's counters; lo picks the value stream and its unroll knob
    void product(const double *x, double *y, Ctx &c, bool lo);
    void product_after(const PC &pc, const double *x, double *y, Ctx &c, bool lo);
};

// --------------------------------------------------------- preconditioners --
struct PC {
    std::string type;
    int64_t n = 0;
    virtual ~PC() = default;
    virtual void apply(const double *x, double *y, Ctx &c) = 0;
    // apply() may run on two streams at once (no per-application device state)
    virtual bool reentrant() const { return false; }
    // apply() runs a KSP of its own (fieldsplit, the block PC): iterations a
    // device-resident outer loop enqueues past its end would count as inner solves
    virtual bool holds_ksp() const { return false; }
    // the coupling product that belongs to the y apply() returned last (null: none)
    virtual Coupling *coupling_product() const { return nullptr; }
    // the PC that does the work (a redundant PC: the one applied on the gathered block)
    virtual const PC *unwrapped() const { return this; }
};
struct PCNone : PC {
    explicit PCNone(int64_t n_) { type = "none"; n = n_; }
    bool reentrant() const override { return true; }
    void apply(const double *x, double *y, Ctx &c) override;
};
struct PCJacobi : PC {
    DBuf<double> dinv;
    PCJacobi(const DevCSR &M, Ctx &c);
    bool reentrant() const override { return true; }
    void apply(const double *x, double *y, Ctx &c) override;
};
// Exact LU of a block small enough for a dense inverse (dense.hip): K^-1 is
// formed once (blocked Gauss-Jordan, no pivoting, like the sparse path) and
// applied as one dense GEMV.  Chosen for -pc_type lu when n <= pls.lu_dense_max.
struct PCDenseLU : PC {
    int64_t ld = 0;
    DBuf<double> inv;
    DBuf<int32_t> rowperm;  // threshold pivoting's row order (empty: none); inv = (Pi M)^-1
    int32_t piv_stats[3] = {0, 0, 0};  // rows exchanged, pivots below u x column max, zero columns
    // u: MUMPS's relative pivot threshold CNTL(1) (pls.lu_pivot_threshold, default 0.01; 0 = no pivoting)
    PCDenseLU(const DevCSR &M, Ctx &c, double u = 0.0);
    bool reentrant() const override { return true; }
    void apply(const double *x, double *y, Ctx &c) override;
};
// Exact LU of a banded block past the dense-inverse size (band.hip): 64 x 64
// tiles, right-looking factorization without pivoting, flag-chained sweeps.
// Not reentrant (the sweeps share the granules, the ticket and t).
struct PCBandLU : PC {
    int64_t nb = 0, bl = 0, bu = 0;
    DBuf<double> T, Dl, Du, Gl, Gu, t;  // Gl / Gu: near-tile products (band.hip)
    DBuf<int32_t> fail;
    DBuf<uint64_t> G, ticket;  // G: 128 tagged granules per tile row (the sweeps' hand-off)
    uint64_t sweeps = 0;  // launched sweeps (ticket base = sweeps * band_sweep_tickets(nb))
    int64_t plen = 0;     // SPIKE partition length in tile rows (0: one chain per triangle)
    DBuf<double> Wl, Wu;  // SPIKE spikes of L and U (nb x bl, nb x bu tiles)
    DBuf<double> spike_tmp;  // tail partial sums
    // spike_plen: -1 auto (~16 partitions), 0 off, > 0 partition length in tile rows
    PCBandLU(const DevCSR &M, int64_t kl, int64_t ku, Ctx &c, int64_t spike_plen = -1);
    void apply(const double *x, double *y, Ctx &c) override;
    int32_t check_fail(Ctx &c);  // synchronising: the fail word (2: a sweep spin gave up)
};
// Lower / upper bandwidth of a square CSR matrix with sorted rows.
// Eigenvalues of the leading m x m of an upper Hessenberg matrix (column-major, H[i + j * ldh];
// entries below the subdiagonal are not read), m <= 64: shifted QR in complex arithmetic, no
// LAPACK.  Returns nonzero when it fails to converge (or m is out of range).
int hessenberg_eigenvalues(int m, const double *H, int ldh, double *re, double *im);
void csr_bandwidths(const DevCSR &M, int64_t &kl, int64_t &ku, Ctx &c);
// -pc_type lu / cholesky (MUMPS in the reference): dense inverse up to
// pls.lu_dense_max rows, else the sparse (nested dissection, multifrontal) LU;
// pls.lu_path dense|sparse|band|envelope forces one.
std::unique_ptr<PC> make_lu(const DevCSR &M, const Options &o, Ctx &c);
// Sparse LU by nested dissection + multifrontal factorization (sparse_lu.cpp)
std::unique_ptr<PC> make_sparse_lu(const DevCSR &M, const Options &o, Ctx &c);
void sparse_lu_analyze(const HostCSR &A, const Options &o, double *stats, int64_t nstats, int32_t *perm = nullptr,
                       int32_t *front_of = nullptr, int32_t *parent = nullptr);
std::unique_ptr<PC> make_pc(const std::string &type, const DevCSR &M, const Options &o, const std::string &prefix,
                            Ctx &c);
// Smoothed-aggregation AMG (amg.cpp; -pc_type gamg, and hypre with pls.hypre sa).
std::unique_ptr<PC> make_amg(const DevCSR &M, const Options &o, const std::string &prefix, bool hypre, Ctx &c);
// Classical AMG as the reference configures BoomerAMG (boomeramg.cpp; -pc_type hypre).
std::unique_ptr<PC> make_boomeramg(const DevCSR &M, const Options &o, const std::string &prefix, Ctx &c);
// hypre's np = G hierarchy on a sharded block (M: this rank's rows; global: the gathered block)
std::unique_ptr<PC> make_boomeramg_dist(const DevCSR &M, const HostCSR &global, const std::vector<int64_t> &rank_rows,
                                        const Options &o, const std::string &prefix, Ctx &c);
void boomeramg_host_level(const HostCSR &A, const Options &o, const std::string &prefix, int64_t level,
                          int64_t &nlevels, int64_t &n, int64_t &nc, std::vector<int8_t> &cf, HostCSR &P);
// pls_get_boomeramg_relax's values when pc is the BoomerAMG stand-in (else false): stats[0] relax
// type 0-3, [1] smoothed levels, [2] Chebyshev order, [3] levels on the fused step, [4] fused and
// [5] elementwise step launches of the last application; lambda[l < cap] the levels' estimates
// throws, naming the key, when <prefix>pc_hypre_boomeramg_relax_type_all is not the default:
// the refusal of a sharded block (PCRedundant and make_boomeramg_dist share it)
void boomeramg_refuse_sharded_relax(const Options &o, const std::string &prefix);
bool boomeramg_relax_info(const PC *pc, int64_t stats[6], double *lambda, int32_t cap);

// ---------------------------------------------------------------------- KSP --
struct BcColumns;  // bccols.hpp: the Dirichlet-column split a KSP may own (pls_bc_columns)

enum Reason {
    CONVERGED_ITERATING = 0, CONVERGED_RTOL = 2, CONVERGED_ATOL = 3, CONVERGED_ITS = 4,
    DIVERGED_NULL = -2, DIVERGED_ITS = -3, DIVERGED_DTOL = -4, DIVERGED_BREAKDOWN = -5,
    DIVERGED_INDEFINITE_PC = -8, DIVERGED_NANORINF = -9, DIVERGED_INDEFINITE_MAT = -10,  // petscksp.h
    DIVERGED_TIME_LIMIT = -100  // libpls diagnostic (pls.solver_time_limit), not a PETSc reason
};

struct KSP {
    std::string prefix, type = "gmres";
    double rtol = 1e-5, atol = 1e-50, dtol = 1e4;
    int64_t maxit = 10000, restart = 30;
    bool right = false;
    std::string norm = "preconditioned";
    Op *A = nullptr;
    PC *pc = nullptr;
    // <prefix>pls_bc_columns lift | drop: K' and C of the block this KSP was given;
    // null with keep.  In front of the PC and the operator, which are built from K' and go first.
    std::unique_ptr<BcColumns> bc;
    std::unique_ptr<PC> owned_pc;
    std::unique_ptr<Op> owned_op;
    int64_t n = 0;
    // results
    int its = 0, reason = 0;
    double rnorm = 0;
    std::vector<double> history;
    bool keep_history = true;
    bool monitor = false;
    // pls.ksp_stats: iteration totals printed when the KSP is destroyed (diagnostics)
    bool stats = false;
    double time_limit = 0;  // seconds (pls.solver_time_limit, the outer solver only; 0: none)
    double t_start = 0;
    int64_t stat_its = 0, stat_max = 0, stat_solves = 0, stat_div = 0;  // stat_div: solves with reason < 0
    int64_t stat_last_neg = 0;  // the most recent negative reason
    KSP();  // (out of line, as the destructor: bc's type is complete in ksp.cpp only)
    KSP(const KSP &) = delete;
    ~KSP();
    // work
    DBuf<double> V, w, t1, t2, t3, t4;
    int64_t ldv = 0;  // column stride of the Krylov basis V
    DBuf<double> Z;   // FGMRES: the preconditioned basis Z_k = M^-1 V_k (restart columns, stride ldv)
    DBuf<double> t5, t6, t7;  // BiCGStab: with t1..t4, its seven work vectors
    DBuf<unsigned> bcticket;  // ... the tickets of its single-launch reductions
    bool bcgs_device = true;  // pls.bcgs_device: BiCGStab's recurrence on the device
    bool bcgs_fused = true;   // pls.bcgs_fused_reduce: the last block to arrive finishes each sum (one rank only)
    DBuf<double> dh;  // device Hessenberg column / coefficients (and a second CGS pass's column behind it)
    // GMRES orthogonalisation (gmres, fgmres): ksp_gmres_modifiedgramschmidt, ksp_gmres_cgs_refinement_type
    enum Orthog { CGS_NEVER = 0, CGS_IFNEEDED = 1, CGS_ALWAYS = 2, MGS = 3 };
    int orthog = CGS_NEVER;
    bool mgs_fused = false;      // pls.gmres_mgs_fused: the last block to arrive finishes each MGS sum (one rank only)
    DBuf<double> mgs_part;       // MGS: one row of partials ...
    DBuf<unsigned> mgs_ticket;   // ... and the ticket of its single-launch reductions
    int64_t stat_orth_steps = 0, stat_orth_second = 0;  // Arnoldi steps orthogonalised, second CGS passes
    // Compressed-basis GMRES (gmres, fgmres; <prefix>pls_gmres_basis single): the basis in fp32 (Vf, ldv a
    // multiple of 128 floats), w (cbw) and the promoted newest basis vector (cbv), which the operator and the
    // PC read, in fp64.  A cycle ends when the estimate has fallen by basis_drop from its start (rule a), and an
    // estimate that meets the tolerance ends the cycle only: the next cycle's true residual decides (rule b).
    bool basis_single = false;
    double basis_drop = 1e-6;  // <prefix>pls_gmres_basis_drop (0: rule a off)
    DBuf<float> Vf;
    DBuf<double> cbw, cbv;
    int allocated_single = -1;  // the mode the work vectors were allocated for
    bool vf_canary = false;     // pls.debug_bounds: Ctx::CANARY guard bytes behind Vf (check_basis_bounds)
    int64_t stat_cb_forced = 0, stat_cb_confirm = 0, stat_cb_failed = 0;  // rule (a) cycle ends, rule (b)
                                                                          // confirmations, those that failed
    // Compressed-operator GMRES (<prefix>pls_gmres_operator single, with the fp32 basis only): the
    // Arnoldi step's product through A->apply_low / apply_after_low; cycle-start residuals, the
    // guesses' products and everything else through the fp64 operator
    bool operator_single = false;
    int64_t stat_co_low = 0, stat_co_double = 0;  // low / fp64 products in solves
    int64_t basis_bytes() const { return basis_single ? (int64_t)(Vf.n * sizeof(float)) : (int64_t)(V.n * sizeof(double)); }
    // GMRES: keep the Hessenberg columns of the first cycle as Arnoldi made them (the cycle
    // rotates its own copy in place): hess[i + j * (restart + 1)], column j = step j (double basis only)
    bool keep_hess = false;
    std::vector<double> hess;
    // richardson, chebyshev (left, zero initial guess, no inner products unless a norm is asked for)
    double rich_scale = 1.0;        // ksp_richardson_scale
    bool poly_fuse_jacobi = true;   // pls.poly_fuse_jacobi: PCJacobi's product inside the update kernel
    bool cheb_explicit = false;     // ksp_chebyshev_eigenvalues emin,emax given
    double cheb_emin = 0.0, cheb_emax = 0.0;  // the bounds in use (cheb_ready)
    double cheb_raw[2] = {0.0, 0.0};          // the estimate's smallest / largest real part (NaN when explicit)
    double cheb_tr[4] = {0.0, 0.1, 0.0, 1.1};  // ksp_chebyshev_esteig a,b,c,d
    int64_t cheb_steps = 10;                   // ksp_chebyshev_esteig_steps
    bool cheb_ready = false;  // bounds set (explicit: at creation; estimated: at the first solve)
    std::unique_ptr<KSP> cheb_est;  // the GMRES that runs the estimate's Arnoldi steps
    DBuf<double> cgS, cghist;  // device-resident CG: scalar state, residual history
    DBuf<int64_t> cgI;
    bool cg_device = true;     // pls.cg_device: CG's recurrences on the device (no read-back per iteration)
    int64_t allocated_k = -1;
    // The initial guess.  ksp_initial_guess_nonzero (the outer KSP only): x0 is the
    // incoming x.  ksp_guess_type fischer (KSPGuess, model 2): x0 = X B^T b over up to guess_size stored
    // column pairs with B = A X orthonormal, the space updated after every solve.  Either way the solve runs
    // in correction form -- a zero-guess solve of A d = b - A x0 by the type's own loop, x = x0 + d -- with
    // KSPConvergedDefault's rnorm0 taken from b (guess_rnorm0) instead of the first residual.
    bool guess_nonzero = false, guess_fischer = false;
    int64_t guess_size = 10;           // ksp_guess_fischer_model 2,<size>
    double guess_tol = 0.0;            // ksp_guess_fischer_tol
    int64_t guess_m = 0, guess_ldv = 0;  // columns stored now; their stride (a multiple of 64 doubles)
    DBuf<double> gX, gB;               // the space, allocated at the first solve (2 x guess_size x guess_ldv)
    DBuf<double> gx0, gr0, gy, gd;     // x0, r0 = b - A x0, y = A x (and scratch), the projections' scalars
    bool guess_canary = false;         // pls.debug_bounds: Ctx::CANARY guard doubles behind gX and gB
    int64_t stat_guess_formed = 0, stat_guess_skipped = 0, stat_guess_resets = 0;
    double guess_last_reduction = NAN;  // ||b - A x0|| / ||b|| of the most recent solve (NaN before the first)
    double guess_rnorm0 = 0.0;          // > 0 while a guessed solve runs: rnorm0 of the convergence test
    bool guess_timing = false;          // pls.ksp_guess_timing: HIP-event time of what the guess adds to a solve
                                        // (forming x0, r0 and its norms; x = x0 + d and the space's update)
    double guess_seconds = 0.0;         // ... of the most recent solve
    void guess_reset();                 // empties the space and counts a reset (the operator changed)
    void set_type_defaults();
    void resolve_side_norm(const std::string &side, const std::string &nt);
    void solve(const double *b, double *x, Ctx &c);
    // a PREONLY solve whose PC was applied by the caller (BlockPC's fp pipeline): its bookkeeping
    void note_preonly() {
        history.clear();
        its = 1;
        reason = CONVERGED_ITS;
        stat_its += 1;
        stat_max = std::max<int64_t>(stat_max, 1);
        ++stat_solves;
    }
  private:
    void ensure_work(Ctx &c);
    void run(const double *b, double *x, Ctx &c);  // the type's own solve, from a zero guess
    // the wrapper around run() when a guess is in use, and the Fischer space's two operations
    void solve_guessed(const double *b, double *x, Ctx &c);
    void ensure_guess(Ctx &c);
    void guess_form(const double *b, double *x0, Ctx &c);
    void guess_update(const double *x, Ctx &c);
    void check_guess_bounds(Ctx &c);
    hipEvent_t guess_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    void solve_gmres(const double *b, double *x, Ctx &c);  // gmres and fgmres, over V or (basis_single) Vf
    // one Arnoldi step: w orthogonalised against the first k columns of the basis B (V.p or
    // Vf.p); the Hessenberg column's k entries into h (host), ||w||^2 returned
    template <class T>
    double gmres_orthogonalise(int k, const T *B, double *w, double *h, Ctx &c);
    void check_basis_bounds(Ctx &c);
    void solve_cg(const double *b, double *x, Ctx &c);
    void solve_cg_dev(const double *b, double *x, Ctx &c);
    void solve_bcgs(const double *b, double *x, Ctx &c);
    void solve_bcgs_dev(const double *b, double *x, Ctx &c);
    void solve_richardson(const double *b, double *x, Ctx &c);
    void solve_chebyshev(const double *b, double *x, Ctx &c);
    void chebyshev_estimate(Ctx &c);
    // richardson / chebyshev: z = B r through the PC, or (returns true) left to the update kernel
    // with PCJacobi's dinv; rn(r) of the norm type in use; out = a pm1 + b pk + c (B r)
    const double *poly_dinv() const;
    double poly_norm(const double *r, double *z, Ctx &c);
    void poly_step(double a, const double *pm1, double b, const double *pk, double cz, const double *r, double *z,
                   bool z_done, double *out, Ctx &c);
    // what the host and the device driver of a type share: the start (false: ended at iteration 0) and the end
    bool cg_begin(const double *b, double *x, Ctx &c, double &beta);
    bool bcgs_begin(const double *b, double *x, Ctx &c, double &rho0);
    void bcgs_end(double *x, Ctx &c);
    void bcgs_K(const double *in, double *out, Ctx &c);
    // the device-resident loops (CG, BiCGStab): may this solve run one, its parameters, its
    // initial state, and the driver around enqueue(i)
    bool device_loop_allowed() const;
    CgParams cg_params() const;
    void reset_state(const std::vector<double> &s0, bool tickets, Ctx &c);
    template <class Enqueue>
    void device_loop(Ctx &c, Enqueue enqueue);
    int record(int it, double r, bool test = true);  // history, monitor, rnorm; the convergence test's reason
    int converged(int it, double r);
    double rnorm0 = 0, ttol = 0;
};

// PCFIELDSPLIT with two splits given as index sets of the matrix rows
// (reference lib/Preconditioner.py:102-118: split 0 = is_p, split 1 = is_f in
// fp-local numbering).  Types additive, multiplicative, schur (fact diag /
// lower / upper / full; Schur preconditioning matrix selfp or a11; Schur KSP
// operator S = A11 - A10 A00^-1 A01 applied implicitly with the split-0 KSP).
struct PCFieldSplit : PC {
    std::string ftype, fact;
    double scale = -1.0;
    int64_t n0 = 0, n1 = 0;
    DBuf<int32_t> is0, is1;
    DevCSR A00, A01, A10, A11, Sp;
    std::unique_ptr<KSP> k0, k1;
    DBuf<double> x0, x1, y0, y1, t0, t1;
    PCFieldSplit(const DevCSR &M, const std::vector<int32_t> &is0, const std::vector<int32_t> &is1, const Options &o,
                 const std::string &prefix, Ctx &c);
    void apply(const double *x, double *y, Ctx &c) override;
    bool holds_ksp() const override { return true; }
};

// PCREDUNDANT: a sharded diagonal block (Halo::l2g) gathered on every rank,
// factory(global block, single-rank context) builds the PC applied redundantly.
// Sharded diagonal block -> the global host CSR on every rank (PCRedundant's
// gather; rank_rows: the ranks' row counts when contiguous in rank order)
HostCSR gather_block(const DevCSR &M, Ctx &c, const std::string &prefix, std::vector<int64_t> &srcslot,
                     int64_t &maxloc, std::vector<int64_t> &rank_rows);
// a single-rank context with c's layout options (own stream)
std::unique_ptr<Ctx> layout_ctx(const Ctx &c);
// local rows with global columns owned in contiguous rank ranges cst -> distributed DevCSR with halo
void upload_dist(const HostCSR &L, const std::vector<int64_t> &cst, DevCSR &M, Ctx &c);
// (a block gather_block already produced, consumed by make_redundant instead of gathering again)
struct GatheredBlock {
    HostCSR G;
    std::vector<int64_t> srcslot, rank_rows;
    int64_t maxloc = 0;
};
std::unique_ptr<PC> make_redundant(const std::string &type, const DevCSR &M, Ctx &c,
                                   const std::function<std::unique_ptr<PC>(const DevCSR &, Ctx &)> &factory,
                                   const std::string &prefix, GatheredBlock *pre = nullptr);
// Configure a KSP from programmatic defaults + options (setFromOptions order).
std::unique_ptr<KSP> make_ksp(const std::string &prefix, const Options &o, const DevCSR *Amat, const DevCSR *Pmat,
                              const std::string &default_ksp, const std::string &default_pc, Ctx &c,
                              double rtol = 1e-5, double atol = 1e-50, double dtol = 1e4, int64_t maxit = 10000,
                              int64_t restart = 30, PC *external_pc = nullptr);

}  // namespace pls

#include "ilu.hpp"  // PCILU: ilu, bjacobi, the envelope lu, the AMG's Gauss-Seidel chunks
