// blockpc.cpp -- the block preconditioner (blockpc.hpp): setup of its
// sub-blocks and inner solvers, the 2-way and 3-way applies, the 2-way
// pressure-first pipeline.
#include "blockpc.hpp"
#include "bccols.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace pls {

static void ensure_event(hipEvent_t &e) {
    if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
}

Ctx &BlockPC::second_stream() {
    if (!ctx2) ctx2 = std::make_unique<Ctx>();
    return *ctx2;
}

BlockPC::~BlockPC() {
    for (hipEvent_t e : {ev_in, ev_out, fpp.ev_t, fpp.ev_p, fpp.ev_lo})
        if (e) (void)hipEventDestroy(e);
}

void BlockPC::set_bcs(const std::vector<int32_t> &positions, int64_t np_) {
    for (int32_t b : positions)
        if (b < 0 || b >= np_) throw Error("bcs_sub_pressure: position out of range of the p sub-vector");
    nbcs = (int64_t)positions.size();
    dbcs.alloc(std::max<int64_t>(nbcs, 1));
    if (nbcs) HIPCHK(hipMemcpy(dbcs.p, positions.data(), sizeof(int32_t) * nbcs, hipMemcpyHostToDevice));
}

std::vector<const KSP *> BlockPC::ksps() const {
    std::vector<const KSP *> all = {ksp_s.get(), ksp_f.get(), ksp_p.get(), ksp_pd.get(), ksp_fp.get()};
    const PCFieldSplit *fs = ksp_fp ? dynamic_cast<const PCFieldSplit *>(ksp_fp->pc) : nullptr;
    if (!fs) fs = fs_fp.get();
    if (fs) {
        all.push_back(fs->k0.get());
        all.push_back(fs->k1.get());
    }
    all.erase(std::remove(all.begin(), all.end(), nullptr), all.end());
    return all;
}

// ------------------------------------------------------------------ apply ---
void BlockPC::apply(const double *x, double *y, Ctx &c) {
    Timers &T = *timers;
    T.begin(T_PC_TOTAL);
    // coupling reuse: the product with Mfp_s also leaves its raw row sums for the outer A y
    // that follows (the handle decided eligibility: 2-way, no mixer, plain layouts)
    Coupling *R = coupling && coupling->eligible ? coupling : nullptr;
    if (R) {
        R->fresh_for = nullptr;
        R->spans.clear();
        R->spans_flush = T.flushes;
    }
    if (!three_way) {
        T.begin(T_PC_SOLID);
        ksp_s->solve(x, y, c);
        T.end(T_PC_SOLID);
        T.begin(T_PC_FLUID);
        if (fpp.on) {
            apply_fp_pipeline(x, y, c);
        } else {
            // t = x_fp - P_fp,s y_s   (Preconditioner.py:232-233, fused)
            if (R) {
                Timers::Span sp;
                sp.a = T.mark(c.st);
                spmv_store_sums(Mfp_s, y, t_fp.p, c, -1.0, 1.0, x + ns, R->q.p + ns, R->wide(ns));
                sp.b = T.mark(c.st);
                R->spans.push_back(sp);
            } else {
                spmv(Mfp_s, y, t_fp.p, c, -1.0, 1.0, x + ns);
            }
            ksp_fp->solve(t_fp.p, y + ns, c);
        }
        T.end(T_PC_FLUID);
    } else {
        const double *xs = x, *xf = x + ns, *xp = x + ns + nf;
        double *ys = y, *yf = y + ns, *yp = y + ns + nf;
        double *yfd = yfpd.p, *ypd = yfpd.p + nf;
        if (concurrent_3way) {
            // FS sweep on the main stream, DIFF sweep on the second; join before the combination
            Ctx &c2 = *ctx2;
            HIPCHK(hipEventRecord(ev_in, c.st));
            HIPCHK(hipStreamWaitEvent(c2.st, ev_in, 0));
            launch_copy(np, xp, xpd.p, c2.st);                     // :172-173 BC rows of x_p zeroed
            launch_zero_entries(nbcs, dbcs.p, xpd.p, c2.st);
            ksp_pd->solve(xpd.p, ypd, c2);                         // :174
            spmv(Mf_p, ypd, t_f2.p, c2, -1.0, 1.0, xf);            // :184-185
            ksp_f->solve(t_f2.p, yfd, c2);                         // :186
            spmv(Ms_fp, yfd, t_s2.p, c2, -1.0, 1.0, xs);           // :198-201
            ksp_s->solve(t_s2.p, ysd.p, c2);                       // :202
            HIPCHK(hipEventRecord(ev_out, c2.st));
            T.begin(T_PC_PRESS);
            ksp_p->solve(xp, yp, c);                               // :170
            T.end(T_PC_PRESS);
            T.begin(T_PC_FLUID);
            spmv(Mf_p, yp, t_f.p, c, -1.0, 1.0, xf);               // :180-181
            ksp_f->solve(t_f.p, yf, c);                            // :182
            T.end(T_PC_FLUID);
            T.begin(T_PC_SOLID);
            spmv(Ms_fp, yf, t_s.p, c, -1.0, 1.0, xs);              // :192-195
            ksp_s->solve(t_s.p, ys, c);                            // :196
            T.end(T_PC_SOLID);
            HIPCHK(hipStreamWaitEvent(c.st, ev_out, 0));
        } else {
            T.begin(T_PC_PRESS);
            ksp_p->solve(xp, yp, c);                               // :170
            launch_copy(np, xp, xpd.p, c.st);                      // :172-173 BC rows of x_p zeroed
            launch_zero_entries(nbcs, dbcs.p, xpd.p, c.st);
            ksp_pd->solve(xpd.p, ypd, c);                          // :174
            T.end(T_PC_PRESS);
            T.begin(T_PC_FLUID);
            spmv(Mf_p, yp, t_f.p, c, -1.0, 1.0, xf);               // :180-181
            ksp_f->solve(t_f.p, yf, c);                            // :182
            spmv(Mf_p, ypd, t_f.p, c, -1.0, 1.0, xf);              // :184-185
            ksp_f->solve(t_f.p, yfd, c);                           // :186
            T.end(T_PC_FLUID);
            T.begin(T_PC_SOLID);
            spmv(Ms_fp, yf, t_s.p, c, -1.0, 1.0, xs);              // :192-195 (y_f, y_p contiguous)
            ksp_s->solve(t_s.p, ys, c);                            // :196
            spmv(Ms_fp, yfd, t_s.p, c, -1.0, 1.0, xs);             // :198-201
            ksp_s->solve(t_s.p, ysd.p, c);                         // :202
            T.end(T_PC_SOLID);
        }
        // y = w1 y_FS + w2 y_DIFF (:207-212)
        launch_axpby(ns, 0.1, ysd.p, 1.0, ys, c.st);
        launch_axpby(nf + np, 0.1, yfd, 1.0, yf, c.st);
    }
    if (mixer.order > 0) mixer.next(y, c);                         // :248-249
    T.end(T_PC_TOTAL);
    pc_applies++;
    if (R) R->fresh_for = y;
}

// The 2-way fp solve as a pipeline: the heavy blocks' rows of t first, their
// sweep on the second stream while the other rows' product and sweep run here
// (a PREONLY solve).
void BlockPC::apply_fp_pipeline(const double *x, double *y, Ctx &c) {
    auto &F = fpp;
    Ctx &c2 = F.c_p ? *F.c_p : *ctx2;
    Ctx &clo = F.c_lo ? *F.c_lo : c;
    PCILU *pc = static_cast<PCILU *>(ksp_fp->pc);
    // pls.ilu_view 3: per-block start / end of both launches, once (diagnostics)
    DBuf<int64_t> prof;
    if (F.view >= 3 && !F.profiled) prof.alloc(F.nb * 8);
    // (coupling reuse: both launches store their raw row sums and are timed on their streams)
    Coupling *R = coupling && coupling->eligible ? coupling : nullptr;
    double *q = R ? R->q.p + ns : nullptr;
    const D16Wide W = R ? R->wide(ns) : D16Wide();
    Timers::Span sp_hi, sp_lo;
    if (R) sp_hi.a = timers->mark(c.st);
    spmv_slices(Mfp_s, y, t_fp.p, c, -1.0, 1.0, x + ns, F.sl_hi.p, F.n_hi, 0, q, W);
    if (R) sp_hi.b = timers->mark(c.st);
    HIPCHK(hipEventRecord(F.ev_t, c.st));
    HIPCHK(hipStreamWaitEvent(c2.st, F.ev_t, 0));
    pc->apply_blocks(t_fp.p, y + ns, c2, F.b_split, F.nb, F.rr, F.tpb, F.depth, prof.p);
    HIPCHK(hipEventRecord(F.ev_p, c2.st));
    if (F.c_lo) HIPCHK(hipStreamWaitEvent(clo.st, F.ev_t, 0));
    // (pls.fp_pipeline_lds: its workgroups reserve LDS they do not use)
    if (R) sp_lo.a = timers->mark(clo.st);
    spmv_slices(Mfp_s, y, t_fp.p, clo, -1.0, 1.0, x + ns, F.sl_lo.p, F.n_lo, F.lds, q, W);
    if (R) {
        sp_lo.b = timers->mark(clo.st);
        R->spans.push_back(sp_hi);
        R->spans.push_back(sp_lo);
    }
    if (F.c_lo) {
        HIPCHK(hipEventRecord(F.ev_lo, clo.st));
        HIPCHK(hipStreamWaitEvent(c.st, F.ev_lo, 0));
    }
    pc->apply_blocks(t_fp.p, y + ns, c, 0, F.b_split, 0, 0, 2, prof.p);
    HIPCHK(hipStreamWaitEvent(c.st, F.ev_p, 0));
    if (prof.p) print_fp_profile(prof, c);
    ksp_fp->note_preonly();
    c.check_bounds();  // (what KSP::solve does after a solve; pls.debug_bounds)
}

void BlockPC::print_fp_profile(const DBuf<int64_t> &prof, Ctx &c) {
    auto &F = fpp;
    F.profiled = true;
    std::vector<int64_t> hp(F.nb * 8);
    HIPCHK(hipMemcpyAsync(hp.data(), prof.p, sizeof(int64_t) * hp.size(), hipMemcpyDeviceToHost, c.st));
    c.sync();
    int64_t t0 = INT64_MAX;
    for (int64_t b = 0; b < F.nb; ++b) t0 = std::min(t0, hp[b * 8]);
    auto span = [&](int64_t b0, int64_t b1, const char *what) {
        int64_t s0 = INT64_MAX, s1 = 0, e1 = 0;
        double dsum = 0;
        for (int64_t b = b0; b < b1; ++b) {
            s0 = std::min(s0, hp[b * 8]);
            s1 = std::max(s1, hp[b * 8]);
            e1 = std::max(e1, hp[b * 8 + 2]);
            dsum += (hp[b * 8 + 2] - hp[b * 8]) * 0.01;
        }
        fprintf(stderr, "[pls fp pipeline] %s blocks [%lld, %lld): starts %+.1f .. %+.1f us, last end %+.1f us, "
                "mean duration %.1f us\n", what, (long long)b0, (long long)b1, (s0 - t0) * 0.01,
                (s1 - t0) * 0.01, (e1 - t0) * 0.01, dsum / std::max<int64_t>(1, b1 - b0));
    };
    span(F.b_split, F.nb, "heavy");
    span(0, F.b_split, "light");
}

// ------------------------------------------------------------------ setup ---
void BlockPC::setup(const Inputs &in) {
    Ctx &c = in.ctx;
    three_way = in.three_way;
    ns = in.ns;
    nf = in.nf;
    np = in.np;
    timers = &in.timers;
    type = "python";
    n = ns + nf + np;
    extract_blocks(in);
    // (PLS_SETUP_TRACE: wall time of the setup stages on stderr)
    const bool trace = std::getenv("PLS_SETUP_TRACE") != nullptr;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    c.sync();
    double t0 = now();
    auto stage = [&](const char *what) {
        if (!trace) return;
        c.sync();
        const double t1 = now();
        fprintf(stderr, "[setup] %s %.2f s\n", what, t1 - t0);
        t0 = t1;
    };
    stage("blocks extracted");
    // inner solvers (setup_elliptic_solver / setup_fieldsplit; options win)
    const Options &o = in.opt;
    ksp_s = make_ksp("s_", o, &Ks, &Ks, in.inner_ksp, in.inner_pc, c);
    stage("s block solver");
    if (three_way) {
        ksp_f = make_ksp("f_", o, &Kf, &Kf, in.inner_ksp, in.inner_pc, c);
        ksp_p = make_ksp("p_", o, &Kp, &Kp, in.inner_ksp, in.inner_pc, c);
        ksp_pd = make_ksp("diff_", o, &Kpd, &Kpd, in.inner_ksp, in.inner_pc, c);
    } else {
        make_fp_solver(in);
    }
    stage(three_way ? "f / p / diff block solvers" : "fp block solver");
    // the inner Anderson history lives as long as the preconditioner object
    // (lib/Preconditioner.py: created in __init__, not in setUp)
    if (!mixer_ready) {
        mixer.init((int)o.integer("pls.inner_accel_order", 0), n);
        mixer_ready = true;
    }
    t_fp.alloc(std::max<int64_t>(nf + np, 1));
    t_s.alloc(std::max<int64_t>(ns, 1));
    t_f.alloc(std::max<int64_t>(nf, 1));
    xpd.alloc(std::max<int64_t>(np, 1));
    yfpd.alloc(std::max<int64_t>(nf + np, 1));
    ysd.alloc(std::max<int64_t>(ns, 1));
    choose_concurrent_3way(in);
    setup_fp_pipeline(in);
}

// lib/Preconditioner.py:60-75 allocate_submatrices (field-major: contiguous ranges), and the
// SELL-64 copies of every matrix the PC multiplies with
void BlockPC::extract_blocks(const Inputs &in) {
    Ctx &c = in.ctx;
    const Dist &D = in.dist;
    const int64_t first[4] = {0, ns, ns + nf, ns + nf + np};  // local rows of field f: [first[f], first[f + 1])
    // rows [r0, r1) of M, the columns of the fields [f0, f1].  One rank: M's columns are the
    // local rows' numbering.  Sharded: they are global, and the block becomes distributed.
    auto block = [&](const DevCSR &M, int f_rows0, int f_rows1, int f0, int f1, DevCSR &dst) {
        const int64_t g0 = in.distributed ? D.off[f0] : first[f0];
        const int64_t g1 = in.distributed ? D.off[f1] + D.n[f1] : first[f1 + 1];
        WindowSpec w{};
        w.mode = 0;
        w.c0 = g0;
        w.c1 = g1;
        extract_csr(M, first[f_rows0], first[f_rows1 + 1], w, g0, g1 - g0, dst, c);
        if (in.distributed) make_dist(dst, D, f0, f1, c.comm, c);
    };
    block(in.P, 0, 0, 0, 0, Ks);
    if (!three_way) {
        block(in.P, 1, 2, 0, 0, Mfp_s);
        block(in.P, 1, 2, 1, 2, Kfp);
        build_sell(Mfp_s, c);
    } else {
        if (!in.have_Pd) throw Error("3-way preconditioner needs P_diff");
        block(in.P, 1, 1, 1, 1, Kf);
        block(in.P, 2, 2, 2, 2, Kp);
        block(in.Pd, 2, 2, 2, 2, Kpd);
        block(in.P, 0, 0, 1, 2, Ms_fp);
        block(in.P, 1, 1, 2, 2, Mf_p);
        build_sell(Ms_fp, c);
        build_sell(Mf_p, c);
    }
}

// The 2-way fp block's solver: LU, the fp_ fieldsplit (setup_fieldsplit), or what fp_pc_type names.
void BlockPC::make_fp_solver(const Inputs &in) {
    Ctx &c = in.ctx;
    const Options &o = in.opt;
    if (in.inner_pc == "lu") {
        ksp_fp = make_ksp("fp_", o, &Kfp, &Kfp, in.inner_ksp, "lu", c);
        return;
    }
    const std::string pt = o.str("fp_pc_type", "fieldsplit");
    if (pt != "fieldsplit") {
        ksp_fp = make_ksp("fp_", o, &Kfp, &Kfp, "gmres", pt, c);
        return;
    }
    // setup_fieldsplit (Preconditioner.py:102-118): setFieldSplitIS((None, is_p)) then
    // ((None, is_f)) -- split 0 = pressure, split 1 = fluid, fp-local positions
    PC *fs = nullptr;
    if (in.distributed) {
        // sharded fp block: the fieldsplit PC on the gathered block, redundantly.
        // Gathered order = the block's global order: synthetic shards are
        // field-major (split 0 = p = [nf, nf + np), split 1 = f = [0, nf));
        // caller-assembled ones (pls_create_dist, 2-way: one fp field) are
        // rank-major, each rank's rows its sorted f U p (PETSc's is_fp), so the
        // splits are every rank's fp_is_p / fp_is_f offset by its first row
        std::vector<int32_t> gf, gp;
        const Dist &D = in.dist;
        if (D.n[2] == 0) {
            Comm *cm = c.comm;
            const int G = cm->size;
            int64_t mine[2] = {(int64_t)in.fp_is_f.size(), (int64_t)in.fp_is_p.size()};
            std::vector<int64_t> cnts((size_t)2 * G);
            cm->allgather_host(mine, sizeof(mine), cnts.data());
            int64_t mx = 1;
            for (int64_t v : cnts) mx = std::max(mx, v);
            std::vector<int32_t> sendf(mx, -1), sendp(mx, -1), allf((size_t)mx * G), allp((size_t)mx * G);
            std::copy(in.fp_is_f.begin(), in.fp_is_f.end(), sendf.begin());
            std::copy(in.fp_is_p.begin(), in.fp_is_p.end(), sendp.begin());
            cm->allgather_host(sendf.data(), sizeof(int32_t) * mx, allf.data());
            cm->allgather_host(sendp.data(), sizeof(int32_t) * mx, allp.data());
            for (int q = 0; q < G; ++q) {
                const int64_t base = D.start[1][q];
                for (int64_t k = 0; k < cnts[2 * q]; ++k) gf.push_back((int32_t)(base + allf[(size_t)q * mx + k]));
                for (int64_t k = 0; k < cnts[2 * q + 1]; ++k) gp.push_back((int32_t)(base + allp[(size_t)q * mx + k]));
            }
        } else {
            for (int64_t i = 0; i < D.n[1]; ++i) gf.push_back((int32_t)i);
            for (int64_t i = 0; i < D.n[2]; ++i) gp.push_back((int32_t)(D.n[1] + i));
        }
        pc_red_fp = make_redundant("fieldsplit", Kfp, c, [&](const DevCSR &Gm, Ctx &sc) -> std::unique_ptr<PC> {
            return std::make_unique<PCFieldSplit>(Gm, gp, gf, o, "fp_", sc);
        }, "fp_");
        fs = pc_red_fp.get();
    } else {
        std::vector<int32_t> fpf = in.fp_is_f, fpp_ = in.fp_is_p;
        if (fpf.empty() && fpp_.empty()) {  // field-major fp block: [f | p]
            for (int64_t i = 0; i < nf; ++i) fpf.push_back((int32_t)i);
            for (int64_t i = 0; i < np; ++i) fpp_.push_back((int32_t)(nf + i));
        }
        fs_fp = std::make_unique<PCFieldSplit>(Kfp, fpp_, fpf, o, "fp_", c);
        fs = fs_fp.get();
    }
    ksp_fp = make_ksp("fp_", o, &Kfp, &Kfp, "gmres", "fieldsplit", c, 1e-5, 1e-50, 1e4, 10000, 30, fs);
}

// 3-way: the FS (p -> f -> s) and DIFF sweeps are independent until the
// final w1/w2 combination (Preconditioner.py:150-212); with PREONLY inner
// solves (no host round trips) the DIFF sweep runs on a second stream.
// Not with several ranks: two streams would interleave halo exchanges on
// one communicator.
void BlockPC::choose_concurrent_3way(const Inputs &in) {
    concurrent_3way = false;
    if (!three_way || in.distributed || !in.opt.flag("pls.concurrent_sweeps", true)) return;
    bool pre = true;
    for (KSP *k : {ksp_s.get(), ksp_f.get(), ksp_p.get(), ksp_pd.get()}) pre = pre && k && k->type == "preonly";
    // the s and f PCs serve both sweeps at once: they must be reentrant
    for (KSP *k : {ksp_s.get(), ksp_f.get()}) pre = pre && k->pc && k->pc->reentrant();
    // ... and so must their solves: a lifting KSP (pls_bc_columns lift) forms b' in one buffer of its own
    // (p_ and diff_ each solve on one stream only)
    for (KSP *k : {ksp_s.get(), ksp_f.get()}) pre = pre && !(k->bc && k->bc->lifting());
    if (!pre) return;
    second_stream();
    ensure_event(ev_in);
    ensure_event(ev_out);
    t_s2.alloc(std::max<int64_t>(ns, 1));
    t_f2.alloc(std::max<int64_t>(nf, 1));
    concurrent_3way = true;
}

// The 2-way PC's fp solve with PREONLY + BJACOBI(ILU(0)) on the LDS sweep:
// when the last blocks (the pressure rows of the field-major fp block) carry
// well over the median block's levels, their rows of t = x_fp - P_fp,s y_s are
// computed first and swept on a second stream beside the rest of the product
// (the headline N=59: 11 pressure blocks of 263 levels per triangle, ~500 us,
// against 56 for the fluid blocks).  Results are bitwise those of the plain
// path: the same per-row sums and per-block sweeps.  pls.fp_pipeline 0 turns
// it off.
void BlockPC::setup_fp_pipeline(const Inputs &in) {
    auto &F = fpp;
    Ctx &c = in.ctx;
    F.on = false;
    // pls.fp_pipeline: 1 always, 0 never, -1 (default) when the s block's PC is an
    // ILU / BJACOBI sweep too.  Measured (MI355X, N=59, same box, A/B x 3): the
    // BJACOBI headline 168.4 -> 169.8 it/s; with BoomerAMG on the s block 120 ->
    // 114 it/s -- with the CU-masked queues present every kernel of the V-cycle's
    // ~40 per iteration ran slower (small ones ~2-10x), which the pipeline's
    // ~90 us per iteration does not repay
    const int64_t mode = in.opt.integer("pls.fp_pipeline", -1);
    if (three_way || in.distributed || mode == 0) return;
    if (!ksp_fp || ksp_fp->type != "preonly" || mixer.order > 0) return;
    if (ksp_fp->monitor) return;  // -fp_ksp_monitor: the plain path's KSP::solve prints it
    if (ksp_fp->bc && ksp_fp->bc->lifting()) return;  // fp_pls_bc_columns lift: KSP::solve forms b' first
    if (mode < 0 && !(ksp_s && ksp_s->type == "preonly" && dynamic_cast<PCILU *>(ksp_s->pc))) return;
    PCILU *pc = dynamic_cast<PCILU *>(ksp_fp->pc);
    if (!pc || !pc->can_apply_blocks() || pc->nblocks < 8 || pc->block_levels_h.size() != (size_t)pc->nblocks) return;
    const DevCSR &M = Mfp_s;
    if (!M.sell || !M.sell->d16 || M.halo || M.sell->nperm || M.sell->b3_nslices || M.sell->nrows_mapped) return;
    const int64_t nb = pc->nblocks;
    std::vector<int64_t> lev(pc->block_levels_h);
    std::vector<int64_t> srt(lev);
    std::nth_element(srt.begin(), srt.begin() + nb / 2, srt.end());
    const int64_t med = srt[nb / 2];
    int64_t b = nb;
    while (b > 0 && lev[b - 1] >= 2 * med) --b;
    if (b == nb || nb - b > nb / 8 || b == 0) return;  // no heavy tail, or too much of the block
    const DevSELL &S = *M.sell;
    std::vector<int64_t> sf(S.nslices + 1);
    HIPCHK(hipMemcpyAsync(sf.data(), S.sfirst.p, sizeof(int64_t) * sf.size(), hipMemcpyDeviceToHost, c.st));
    c.sync();
    const int64_t r_split = pc->block_start_h[b];
    std::vector<int32_t> hi, lo;
    for (int64_t s = 0; s < S.nslices; ++s) (sf[s + 1] > r_split ? hi : lo).push_back((int32_t)s);
    F.sl_hi.alloc(std::max<size_t>(hi.size(), 1));
    F.sl_lo.alloc(std::max<size_t>(lo.size(), 1));
    if (!hi.empty())
        HIPCHK(hipMemcpyAsync(F.sl_hi.p, hi.data(), sizeof(int32_t) * hi.size(), hipMemcpyHostToDevice, c.st));
    if (!lo.empty())
        HIPCHK(hipMemcpyAsync(F.sl_lo.p, lo.data(), sizeof(int32_t) * lo.size(), hipMemcpyHostToDevice, c.st));
    c.sync();
    second_stream();
    ensure_event(F.ev_t);
    ensure_event(F.ev_p);
    // Experimental variants for the heavy sweep (both measured no faster, kept
    // opt-in): round-robin wave groups owning whole levels
    // (pls.fp_pipeline_rr g) and 6 levels of factor data in flight on 8 waves
    // (pls.fp_pipeline_depth 6, levels of <= 8 slices) -- meant for the
    // concurrent product's HBM traffic, which stretches a load's latency past
    // the plain sweep's two levels (the 11 pressure blocks: 1.24 ms beside the
    // unmasked product, ~0.5 ms alone)
    int64_t msl = 0;
    for (int64_t k = b; k < nb; ++k) msl = std::max(msl, pc->block_maxsl_h.empty() ? 16 : pc->block_maxsl_h[k]);
    // pls.fp_pipeline_rr (experimental, measured no faster): 0 / -1 off (default), or a forced group size
    const int64_t rr_opt = in.opt.integer("pls.fp_pipeline_rr", 0);
    if (rr_opt > 16 || (rr_opt > 0 && (rr_opt & (rr_opt - 1))))
        throw Error("pls.fp_pipeline_rr must be 0 (off) or a power of two <= 16");
    const bool deep = msl <= 8 && in.opt.integer("pls.fp_pipeline_depth", 2) == 6;
    F.rr = rr_opt > 0 ? (int)rr_opt : 0;
    F.tpb = deep && F.rr == 0 ? 512 : 0;
    F.depth = deep && F.rr == 0 ? 6 : 2;
    // the sweep holds max_len * 8 bytes of the CU's 160 KiB: reserve more than what is left
    const int64_t left = 163840 - pc->max_len * 8;
    const int64_t lds_opt = in.opt.integer("pls.fp_pipeline_lds", 0);
    F.lds = (size_t)(lds_opt >= 0 ? lds_opt : (left < 16384 ? ((left + 1024) & ~int64_t(1023)) : 0));
    // reserved CUs: the heavy blocks' count rounded up to a multiple of 8 (one per XCD)
    int ncu = 0, dev = 0;
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    const int64_t cus_opt = in.opt.integer("pls.fp_pipeline_cus", -1);
    const int want = (int)(cus_opt >= 0 ? cus_opt : (nb - b + 7) / 8 * 8);
    F.cus = (want >= nb - b && want <= ncu / 4) ? want : 0;
    F.c_p.reset();
    F.c_lo.reset();
    if (F.cus > 0) {
        const uint32_t words = (uint32_t)((ncu + 31) / 32);
        std::vector<uint32_t> mp(words, 0), ml(words, 0);
        // which mask bits: pls.fp_pipeline_cu_layout 0 -- bits [0, R) (one per XCD in turn
        // if the driver deals bits round robin over the XCDs), 1 -- R / 8 consecutive
        // bits at the start of every 1/8 of the mask (XCD-major bit order)
        const int64_t layout = in.opt.integer("pls.fp_pipeline_cu_layout", 0);
        for (int k = 0; k < ncu; ++k) {
            const int per = ncu / 8;
            const bool res = layout == 1 ? (k % per) < F.cus / 8 : k < F.cus;
            (res ? mp : ml)[k / 32] |= 1u << (k % 32);
        }
        // (a driver without CU masking: plain streams, F.cus = 0)
        auto masked = [&](const std::vector<uint32_t> &m) -> std::unique_ptr<Ctx> {
            auto cx = std::make_unique<Ctx>();
            hipStream_t s = nullptr;
            if (hipExtStreamCreateWithCUMask(&s, words, m.data()) != hipSuccess) {
                (void)hipGetLastError();
                return nullptr;
            }
            HIPCHK(hipStreamDestroy(cx->st));
            cx->st = s;
            cx->d16_unroll = c.d16_unroll;
            cx->d16_xcd = c.d16_xcd;
            return cx;
        };
        F.c_p = masked(mp);
        F.c_lo = F.c_p ? masked(ml) : nullptr;
        if (!F.c_p || !F.c_lo) {
            F.c_p.reset();
            F.c_lo.reset();
            F.cus = 0;
        }
        ensure_event(F.ev_lo);
    }
    F.b_split = b;
    F.nb = nb;
    F.n_hi = (int64_t)hi.size();
    F.n_lo = (int64_t)lo.size();
    F.view = c.ilu_view;
    F.on = true;
    if (c.ilu_view)
        fprintf(stderr, "[pls fp pipeline] blocks [%lld, %lld) first (levels >= %lld, median %lld), rows from %lld, "
                "slices %lld + %lld, round-robin groups %d (most slices per level %lld), product LDS reserve %zu, "
                "sweep tpb %d depth %d, reserved CUs %d\n", (long long)b, (long long)nb,
                (long long)(2 * med), (long long)med, (long long)r_split, (long long)F.n_hi, (long long)F.n_lo, F.rr,
                (long long)msl, F.lds, F.tpb, F.depth, F.cus);
}

}  // namespace pls
