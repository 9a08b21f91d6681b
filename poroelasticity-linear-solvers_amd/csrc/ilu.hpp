// ilu.hpp -- PCILU, the block ILU(0) / Gauss-Seidel preconditioner, and the
// device tables of its sweep kernels (ilu.cpp).  runtime.hpp includes it at its end.
#pragma once
#include "runtime.hpp"

namespace pls {

// Level-aligned SELL-64 strict triangular factor (see sweep_lds.hip).
struct TriSELL {
    int64_t nslices = 0, ngroups = 0, nblocks = 0;
    bool blockwise = false;
    DBuf<int64_t> sptr, gslice, goff;
    DBuf<int32_t> slot_row, slot_len, col;
    DBuf<double> val, sdinv;
    std::vector<int64_t> gslice_h;
    void apply(const double *b, double *y, Ctx &c) const;
};
// LDS-kernel stream layout of a blockwise TriSELL (header entry per lane,
// block-local columns; levels/groups shared with the TriSELL).
struct LdsTri {
    DBuf<int64_t> sptr, gslice;  // slices differ from the TriSELL's (lanes per row); groups/goff are shared
    DBuf<int32_t> col, lpr;      // lpr: lanes per row, per block
    DBuf<double> val;
};
// Ring sweep tables of one triangle (sweep_lds.hip, k_ilu_blocks_ring)
struct RingTri {
    DBuf<int64_t> coff, cg, cp;  // chunks per block / first level / [start, end) positions
    DBuf<int32_t> ord;           // position -> row (the triangle's level order)
    DBuf<int64_t> frp;           // far dependencies per position (CSR over b0 + p)
    DBuf<int32_t> fcol;          // ... block-local positions
    DBuf<double> fval;           // ... factor values
    int64_t nfar = 0;
};
// Chain-sweep stream of one triangle (kernels.hip, k_ilu_blocks_chain)
struct ChainTri {
    DBuf<int64_t> base, soff, nsl;  // per block: first entry, first slice, slice count
    DBuf<int32_t> sz, lpr;          // per slice: size | (8 entries per lane); per block: lanes per row
    DBuf<int32_t> col;
    DBuf<double> val;
};
// Window-sweep tables of one triangle (kernels.hip, k_ilu_blocks_window)
struct WinTri {
    DBuf<int64_t> woff;  // per window: off-window stream offsets (nwin + 1)
    // rec: per stream entry (value, block-local column) as 3 words -- one
    // 12-byte load each; tinv: per window the 64 x 64 inverse of its diagonal
    // block, column pairs [k / 2][lane][k % 2]
    DBuf<int32_t> rec;
    DBuf<double> tinv;
    int64_t nwin = 0;
};
// Super-window sweep tables of one triangle (kernels.hip, k_ilu_blocks_swin):
// blocks too long for LDS, in windows of 64 rows grouped into super-windows
// whose window inverses and near streams fit LDS (see build_swin_tri)
struct SwinTri {
    DBuf<int64_t> bsw;         // per block: first super-window (nblocks + 1), in processing order
    DBuf<int64_t> sw;          // per super-window: first window (global), windows, first row, end row (block-local)
    DBuf<int64_t> wnear, wfar;  // per window: near / far SELL offsets (nwin + 1)
    DBuf<int32_t> ncol, fcol;  // near: row - super-window's first row (LDS index); far: block-local row
    DBuf<double> nval, fval;
    DBuf<double> tinv;  // per window the packed triangle of the window inverse (2080 doubles)
    int64_t lds_bytes = 0, nwin = 0, nsw = 0;
};

// ILU(0) of the block-Jacobi truncation of M (nblocks == 1: plain ILU(0)).
// Factorization: level scheduled, one wave per row.  Sweeps: one of ten
// kernels (Sweep), chosen once at setup (choose_sweep) -- one launch per
// global level, or one workgroup per block walking the block's own levels,
// windows or chain.
struct PCILU : PC {
    // the kernel that serves apply(), in pls.ilu_view's words (sweep_kind())
    enum class Sweep {
        Levels,            // SELL-64 level slices: a launch per global level, or (>= 64 blocks) a workgroup per block
        LevelsCsr,         // a launch per global level straight from the factored CSR, 16 lanes per row
        Lds,               // one workgroup per block, the block solution in LDS (k_ilu_blocks_lds)
        Gmem,              // ... in y itself (blocks too long for LDS)
        Ring,              // ... y-resident in level-order position space, an LDS ring of recent values
        Chain,             // one wave per block, 16-lane steps in order (deep, narrow level DAGs)
        Window,            // 64-row windows with explicit inverses of the windows' triangles, LDS-resident
        WindowRing,        // ... y-resident, an LDS ring of the recent rows
        LevelsWindowRing,  // L by the y-resident level sweep, U by ring windows (pls.window_mixed)
        Swin               // super-windows (pls.sweep_swin): blocks too long for LDS
    };
    struct Config {
        // the same pipeline on the profile (envelope) pattern of M -- row i spans the
        // contiguous columns [first nonzero of row i, max column of rows <= i], which
        // contains every fill entry of LU without pivoting, so the "ILU" of that
        // pattern is the exact LU factorization (PCLU)
        bool exact_lu = false;
        bool allow_lds = true;  // block solution resident in LDS when it fits (pls.ilu_lds)
        int force_lpr = 0;      // lanes per row of the workgroup sweeps (pls.sweep_lpr; 0: by the longest row)
        // pls.ilu_gmem: 0 auto, 1 force the y-resident workgroup sweep (also on
        // blocks that fit LDS), -1 never, -2 never and per-level CSR kernels
        // (long rows, wide levels: the AMG's Gauss-Seidel triangles) instead of
        // the SELL-64 level slices
        int gmem_mode = 0;
        int ring_mode = 1;  // pls.ilu_ring: the ring sweep where every level fits one chunk
        // no ILU(0) -- the factors are symmetric Gauss-Seidel's (I + L D^-1, D + U;
        // launch_sgs_factor), so apply() is one hybrid symmetric GS sweep from 0 with
        // the blocks as hypre's thread chunks (boomeramg.cpp)
        bool sgs = false;
        // explicit block starts (nblocks + 1 entries from 0 to n) instead of PETSc's bjacobi sizes
        const std::vector<int64_t> *bounds = nullptr;
        int tpb_override = -1;    // pls.sweep_tpb: threads per workgroup (-1: as few waves as the widest level needs)
        int lds_depth = 2;        // levels of factor data in flight in the LDS sweep (pls.sweep_depth 2 / 3 / 4)
        bool rr = false;          // round-robin level sweep (deep DAGs of ~one slice per level; pls.sweep_rr)
        std::string profile_tag;  // non-empty: dump per-block sweep timings once (pls.sweep_profile)
        // levels of fill (<prefix>pc_factor_levels, <prefix>sub_pc_factor_levels for bjacobi's blocks): the
        // ILU(k) pattern of the truncated block replaces the block's own before the factorization (iluk.hip)
        int levels = 0;
        std::string levels_key;  // the option that set it (error messages)
        // test knob (pls.iluk_lds_slots): hash table slots of a symbolic search in LDS, a power of two
        // in [256, 8192]; 0: by the block's longest row.  Rows that need more go through global memory
        int iluk_lds_slots = 0;
        // pls.ilu_lds, pls.ilu_gmem and pls.ilu_ring, and of the sweep tuning options those
        // a site honours (reads): pls.sweep_tpb and pls.sweep_rr (Tuning), pls.sweep_depth /
        // <prefix>pls_sweep_depth (Depth), pls.sweep_lpr and pls.sweep_profile (LprProfile)
        // Levels / SubLevels: the levels of fill of an ilu / of bjacobi's blocks
        enum Reads : unsigned { Tuning = 1, Depth = 2, LprProfile = 4, Levels = 8, SubLevels = 16 };
        static Config from_options(const Options &o, const std::string &prefix, unsigned reads);
    };
    PCILU(const DevCSR &M, int64_t nblocks, Ctx &c, const Config &cfg);
    bool reentrant() const override { return profile_tag.empty(); }
    void apply(const double *x, double *y, Ctx &c) override;
    const char *sweep_kind() const;  // which apply kernel serves this PC (pls.ilu_view)
    // one workgroup per block, and not the ring sweep (what pls.sweep_rr needs)
    bool block_sweep_not_ring() const { return sweep >= Sweep::Lds && sweep != Sweep::Ring; }
    // the plain LDS sweep can run a subset of its blocks (the 2-way PC's
    // pressure-first pipeline, blockpc.cpp BlockPC::apply_fp_pipeline): levels (L + U) and
    // first row of every block, host copies made at setup
    std::vector<int64_t> block_levels_h, block_start_h, block_maxsl_h;  // maxsl: most slices of any level
    bool can_apply_blocks() const { return sweep == Sweep::Lds && profile_tag.empty() && !exact && !sgs; }
    // rr_group > 0: the round-robin sweep with groups of that many waves per level (a power of two)
    // tpb > 0: threads per workgroup for this launch; depth: levels of factor data in flight (2, or 6 with tpb <= 512)
    void apply_blocks(const double *x, double *y, Ctx &c, int64_t b_lo, int64_t b_hi, int rr_group = 0, int tpb = 0,
                      int depth = 2, int64_t *prof = nullptr);  // prof: nblocks x 8 wall-clock records (diagnostics)

    Sweep sweep = Sweep::Levels;
    int64_t nblocks = 1, max_len = 0, nlev_L = 0, nlev_U = 0;  // max_len: longest block
    bool exact = false, sgs = false;  // Config::exact_lu, Config::sgs
    // Config::levels where it applies, the truncated block's entries before the fill (after: F.nnz,
    // longest row F.max_row), rows whose symbolic search left LDS (pls_get_ilu_fill, pls.ilu_view)
    int levels = 0;
    int64_t nnz_block = 0, iluk_gmem_rows = 0;
    std::vector<int64_t> bstart_h;    // Config::bounds (empty: PETSc's bjacobi sizes)
    DBuf<int64_t> bstart;
    DevCSR F;  // truncated matrix, factored in place
    DBuf<int64_t> diag;  // positions of F's diagonal entries; their inverses
    DBuf<double> dinv;
    TriSELL Lf, Uf;  // Levels; the workgroup sweeps share their goff
    DBuf<int32_t> lrowsL, lrowsU;  // LevelsCsr: rows in level order, levels
    std::vector<int64_t> lptrL, lptrU;
    LdsTri Ls, Us;       // Lds, Gmem, Ring (LevelsWindowRing: Ls)
    int lds_tpb = 1024;  // ... threads per workgroup
    int lds_depth = 2;  // ... Config's lds_depth, rr (where the sweep can), profile_tag
    bool lds_rr = false;
    std::string profile_tag;
    RingTri Lr, Ur;       // Ring
    DBuf<int32_t> mapUL;  // ... U position -> index of the row's L-sweep value
    std::map<hipStream_t, std::pair<DBuf<double>, DBuf<double>>> ring_scratch;  // ... per stream: yL, yU
    ChainTri Lc, Uc;  // Chain
    WinTri Lw, Uw;    // Window, WindowRing, LevelsWindowRing
    // ... the rows' most off-window entries per triangle (4, 6 or 8 stream records per wave)
    int window_entries_L = 32, window_entries_U = 32;
    DBuf<int64_t> zgoff;   // LevelsWindowRing: no levels, the empty U of the level launch
    DBuf<int64_t> wstart;  // windows and super-windows: per block its first window
    SwinTri Lsw, Usw;      // Swin

    void fill_levels(Ctx &c, const Config &cfg);  // F <- its ILU(levels) pattern, zeros in the new places
    struct Setup;  // the constructor's steps share a host copy of the factors' pattern and the level orders
    void factor(const DevCSR &M, int64_t nb, Ctx &c, const Config &cfg, Setup &s);
    Sweep choose_sweep(Setup &s, const Ctx &c, const Config &cfg) const;
    void build_tables(Setup &s, Ctx &c, const Config &cfg);
    void print_profile(const DBuf<int64_t> &prof, Ctx &c);  // pls.sweep_profile
};

// PCASM on one rank (asm.cpp, asm.hip): bjacobi's contiguous ranges grown by `overlap` rounds of
// MatIncreaseOverlap_SeqAIJ, A_b = M[I_b, I_b] factored by ILU(levels).  The subdomain matrices
// are the diagonal blocks of one extended matrix E (sum |I_b| rows), which an inner PCILU with
// explicit block bounds factors and sweeps; apply() gathers x into the extended vector (input
// mask), runs the inner sweep and combines (output mask) -- or, where the inner sweep is the
// plain LDS one, runs all three in one launch (k_asm_blocks_lds).
struct PCASM : PC {
    enum Type { Restrict = 0, Basic = 1, Interpolate = 2, None = 3 };  // pls_get_asm_stats' numbering
    PCASM(const DevCSR &M, const Options &o, const std::string &prefix, Ctx &c);
    // scratch vectors are per stream (as PCILU::ring_scratch), so two streams may apply at once
    bool reentrant() const override { return inner->reentrant(); }
    void apply(const double *x, double *y, Ctx &c) override;
    const PC *unwrapped() const override { return inner.get(); }  // pls_get_ilu_fill reports the factors
    int64_t nblocks = 1, overlap = 1, ne = 0, largest = 0;  // ne: sum |I_b|
    Type atype = Restrict;
    bool fused = false;  // k_asm_blocks_lds serves apply()
    bool mask_in() const { return atype == Interpolate || atype == None; }
    bool mask_out() const { return atype == Restrict || atype == None; }
    std::vector<int64_t> ptr_h;  // nblocks + 1 offsets of the subdomains in the extended numbering
    DBuf<int64_t> ptr;
    DBuf<int32_t> gidx;   // global row of each extended row (the subdomains, each ascending)
    DBuf<uint8_t> own;    // 1 where the extended row's block owns the global row
    DBuf<int32_t> opos;   // per global row: its owned extended position
    DBuf<int64_t> tptr;   // per global row: its extended positions, ascending block order (CSR)
    DBuf<int32_t> tpos;
    std::unique_ptr<PCILU> inner;
    struct Scratch { DBuf<double> xe, ye, xc; };
    std::map<hipStream_t, Scratch> scratch;
};

}  // namespace pls
