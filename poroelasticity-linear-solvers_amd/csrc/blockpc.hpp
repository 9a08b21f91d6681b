// blockpc.hpp -- the block preconditioner (lib/Preconditioner.py): 2-way
// [s | fp] and 3-way [s | f | p] with its FS and DIFF sweeps.  It owns the
// sub-blocks of P / P_diff, their inner solvers, the work vectors, the second
// stream and its events, the 2-way pressure-first pipeline and the inner
// Anderson mixer (blockpc.cpp).
#pragma once
#include "anderson.hpp"
#include "dist.hpp"
#include "runtime.hpp"

namespace pls {

struct BlockPC : PC {
    // what setup() reads; nothing of it is referenced afterwards except `timers`
    struct Inputs {
        const DevCSR &P, &Pd;  // rows in field order [s | f | p] (2-way: [s | fp])
        bool have_Pd;
        const Dist &dist;      // row slabs (sharded handles: P's columns are global)
        bool distributed, three_way;
        int64_t ns, nf, np;
        const std::vector<int32_t> &fp_is_f, &fp_is_p;  // 2-way: f / p positions inside the sorted fp set
        const std::string &inner_ksp, &inner_pc;        // defaults of the inner solvers (options win)
        const Options &opt;
        Timers &timers;
        Ctx &ctx;
    };
    // Builds the sub-blocks and the inner solvers again; the mixer's history, the second
    // stream and the events persist from the first call.
    void setup(const Inputs &in);
    // BC positions inside the p sub-vector (the DIFF sweep zeroes them); before setup()
    void set_bcs(const std::vector<int32_t> &positions, int64_t np_);
    void apply(const double *x, double *y, Ctx &c) override;
    bool holds_ksp() const override { return true; }
    // every inner solver, the fp fieldsplit's two included
    std::vector<const KSP *> ksps() const;
    ~BlockPC() override;

    int pc_applies = 0;

    // Coupling reuse (runtime.hpp): the handle's record, set before the first apply.  Where it
    // is eligible the product with the coupling block stores its raw row sums there.
    Coupling *coupling = nullptr;
    // the block an outer operator may share (2-way, no mixer, one rank; after setup), else null
    const DevCSR *coupling_block() const {
        return (!three_way && mixer.order == 0 && !Mfp_s.halo && Mfp_s.sell) ? &Mfp_s : nullptr;
    }
    Coupling *coupling_product() const override {
        return coupling && coupling->eligible && coupling->fresh_for ? coupling : nullptr;
    }

  private:
    bool three_way = false;
    int64_t ns = 0, nf = 0, np = 0;
    Timers *timers = nullptr;
    std::unique_ptr<PCFieldSplit> fs_fp;  // fp_ fieldsplit PC (2-way, inexact inner PC)
    std::unique_ptr<PC> pc_red_fp;        // ... on a sharded fp block: gathered, redundant
    bool mixer_ready = false;
    int64_t nbcs = 0;
    DBuf<int32_t> dbcs;
    // sub-blocks (field-major)
    DevCSR Ks, Kf, Kp, Kpd, Kfp, Mfp_s, Ms_fp, Mf_p;
    std::unique_ptr<KSP> ksp_s, ksp_f, ksp_p, ksp_pd, ksp_fp;
    AndersonMixer mixer;
    // work
    DBuf<double> t_fp, t_s, t_f, xpd, yfpd, ysd;
    DBuf<double> t_s2, t_f2;     // DIFF-sweep temporaries (concurrent 3-way sweeps)
    std::unique_ptr<Ctx> ctx2;   // second stream: the DIFF sweep runs beside the FS sweep
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    bool concurrent_3way = false;
    // 2-way pressure-first pipeline (pls.fp_pipeline): the fp block's heavy
    // BJACOBI blocks (the pressure rows: ~5x the levels of the fluid blocks)
    // get their t = x_fp - P_fp,s y_s rows first and sweep on the second
    // stream while the fluid rows' product runs (same sums, same blocks)
    struct {
        bool on = false;
        int64_t b_split = 0, nb = 0, n_hi = 0, n_lo = 0;
        int rr = 0;  // the heavy blocks' sweep: round robin over groups of rr waves (0: every wave per level)
        size_t lds = 0;  // LDS the concurrent product's workgroups reserve (pls.fp_pipeline_lds)
        int tpb = 0, depth = 2;  // the heavy blocks' sweep: threads per workgroup, levels in flight
        int view = 0;            // pls.ilu_view (3: per-block start / end of both launches, once)
        bool profiled = false;
        // CU-masked streams (pls.fp_pipeline_cus R > 0): the heavy sweep on R
        // reserved CUs, the concurrent product on the others -- with every CU
        // open to both, the product's workgroups (dispatched first) kept the
        // sweep's from starting until the product drained (measured: the 11
        // sweep workgroups all started ~0.75 ms late)
        std::unique_ptr<Ctx> c_p, c_lo;
        hipEvent_t ev_lo = nullptr;
        int cus = 0;
        DBuf<int32_t> sl_hi, sl_lo;  // Mfp_s slices holding rows of the heavy blocks / the rest
        hipEvent_t ev_t = nullptr, ev_p = nullptr;
    } fpp;

    Ctx &second_stream();
    void extract_blocks(const Inputs &in);
    void make_fp_solver(const Inputs &in);
    void choose_concurrent_3way(const Inputs &in);
    void setup_fp_pipeline(const Inputs &in);
    void apply_fp_pipeline(const double *x, double *y, Ctx &c);
    void print_fp_profile(const DBuf<int64_t> &prof, Ctx &c);
};

}  // namespace pls
