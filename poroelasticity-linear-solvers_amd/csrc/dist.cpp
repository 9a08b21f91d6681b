// dist.cpp -- row-slab distribution (dist.hpp): Dist, make_dist, shard_rows.
#include "dist.hpp"

#include <algorithm>

namespace pls {

void Dist::slab(int64_t N, int size, int r, int64_t &lo, int64_t &len) {
    const int64_t q = N / size, rem = N % size;
    lo = r * q + std::min<int64_t>(r, rem);
    len = q + (r < rem ? 1 : 0);
}

void Dist::init_counts(const std::vector<int64_t> counts[3], int r, int s) {
    rank = r;
    size = s;
    int64_t o = 0, lo_ = 0;
    for (int f = 0; f < 3; ++f) {
        start[f].assign(s + 1, 0);
        for (int q = 0; q < s; ++q) start[f][q + 1] = start[f][q] + counts[f][q];
        n[f] = start[f][s];
        off[f] = o;
        o += n[f];
        lo[f] = start[f][r];
        len[f] = counts[f][r];
        loff[f] = lo_;
        lo_ += len[f];
    }
    nloc = lo_;
}

void Dist::init(const int64_t nf[3], int r, int s) {
    std::vector<int64_t> counts[3];
    for (int f = 0; f < 3; ++f) {
        counts[f].resize(s);
        for (int q = 0; q < s; ++q) {
            int64_t l0, l1;
            slab(nf[f], s, q, l0, l1);
            counts[f][q] = l1;
        }
    }
    init_counts(counts, r, s);
}

void make_dist(DevCSR &M, const Dist &D, int f0, int f1, Comm *comm, Ctx &c) {
    int64_t gsize = 0, nlocal = 0;
    int64_t cs_off[3] = {0, 0, 0}, l_off[3] = {0, 0, 0};
    for (int f = f0; f <= f1; ++f) {
        cs_off[f] = gsize;
        l_off[f] = nlocal;
        gsize += D.n[f];
        nlocal += D.len[f];
    }
    std::vector<int32_t> own(gsize, -1);
    for (int f = f0; f <= f1; ++f)
        for (int64_t i = 0; i < D.len[f]; ++i) own[cs_off[f] + D.lo[f] + i] = (int32_t)(l_off[f] + i);
    DBuf<int32_t> down(std::max<int64_t>(gsize, 1));
    DBuf<uint8_t> dflag(std::max<int64_t>(gsize, 1));
    HIPCHK(hipMemcpyAsync(down.p, own.data(), sizeof(int32_t) * gsize, hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemsetAsync(dflag.p, 0, gsize, c.st));
    launch_flag_ghosts(M.nnz, M.ci.p, down.p, dflag.p, c.st);
    std::vector<uint8_t> flag(gsize);
    HIPCHK(hipMemcpyAsync(flag.data(), dflag.p, gsize, hipMemcpyDeviceToHost, c.st));
    c.sync();
    std::vector<std::vector<int64_t>> need(D.size);
    std::vector<int32_t> gmap(own);
    int64_t pos = 0;
    auto H = std::make_shared<Halo>();
    H->rcnt.assign(D.size, 0);
    H->roff.assign(D.size, 0);
    for (int q = 0; q < D.size; ++q) {
        H->roff[q] = pos;
        if (q == D.rank) continue;
        for (int f = f0; f <= f1; ++f) {
            int64_t lo, len;
            D.range(f, q, lo, len);
            for (int64_t i = 0; i < len; ++i) {
                const int64_t g = cs_off[f] + lo + i;
                if (flag[g]) {
                    gmap[g] = (int32_t)(nlocal + pos++);
                    need[q].push_back(g);
                }
            }
        }
        H->rcnt[q] = (int64_t)need[q].size();
    }
    H->nlocal = nlocal;
    H->nghost = pos;
    H->l2g.resize(nlocal + pos);
    for (int f = f0; f <= f1; ++f)
        for (int64_t i = 0; i < D.len[f]; ++i) H->l2g[l_off[f] + i] = cs_off[f] + D.lo[f] + i;
    for (int q = 0, k = 0; q < D.size; ++q)
        for (int64_t g : need[q]) H->l2g[nlocal + k++] = g;
    std::vector<std::vector<int64_t>> asked;
    comm->alltoallv_i64(need, asked);
    std::vector<int32_t> sidx;
    H->scnt.assign(D.size, 0);
    H->soff.assign(D.size, 0);
    for (int q = 0; q < D.size; ++q) {
        H->soff[q] = (int64_t)sidx.size();
        for (int64_t g : asked[q]) {
            if (g < 0 || g >= gsize || own[g] < 0) throw Error("halo plan: peer asked for a column this rank does not own");
            sidx.push_back(own[g]);
        }
        H->scnt[q] = (int64_t)asked[q].size();
    }
    H->nsend = (int64_t)sidx.size();
    H->send_idx.alloc(std::max<int64_t>(H->nsend, 1));
    if (H->nsend) HIPCHK(hipMemcpyAsync(H->send_idx.p, sidx.data(), sizeof(int32_t) * H->nsend, hipMemcpyHostToDevice, c.st));
    H->sendbuf.alloc(std::max<int64_t>(H->nsend, 1));
    H->ghost.alloc(std::max<int64_t>(H->nghost, 1));
    DBuf<int32_t> dgmap(std::max<int64_t>(gsize, 1));
    HIPCHK(hipMemcpyAsync(dgmap.p, gmap.data(), sizeof(int32_t) * gsize, hipMemcpyHostToDevice, c.st));
    launch_remap_cols(M.nnz, M.ci.p, dgmap.p, c.st);
    launch_sort_rows(M.nrows, M.rp.p, M.ci.p, M.val.p, c.st);
    HIPCHK(hipGetLastError());
    c.sync();
    M.ncols = nlocal + H->nghost;
    M.halo = H;
    M.sell.reset();
    build_sell(M, c);
}

// Multi-rank drop-in from caller matrices: the reference runs under
// `mpirun -np 8` (paper-scripts/robustness_2d.sh:29) where every rank holds the
// MPIAIJ rows it owns (A.getValuesCSR() of lib/Solver.py:151's operator: local
// rows, global columns) and the index sets of the dofs it owns
// (lib/IndexSet.py:38-49).  PETSc's createSubMatrix (lib/Preconditioner.py:
// 61-74) then gives every field block the row ownership of the rank-local IS
// entries; the same here: field f of rank q is the contiguous internal range
// start[f][q] .. start[f][q+1] (3-way fields s, f, p; 2-way s and
// fp = sorted(f U p), PETSc's is_fp), columns renumbered to that field-major
// global order; make_dist then builds the halo plan as for synthetic shards.
ShardedRows shard_rows(const pls_csr *A, const pls_csr *P, const pls_csr *Pdiff, int64_t row_start, const int32_t *is_s,
                       int64_t ns, const int32_t *is_f, int64_t nf, const int32_t *is_p, int64_t np, bool three_way,
                       Comm *cm, Ctx &c) {
    ShardedRows out;
    const int G = cm->size, r = cm->rank;
    const int64_t nloc = ns + nf + np;
    if (A->nrows != nloc || P->nrows != nloc || (Pdiff && Pdiff->nrows != nloc))
        throw Error("pls_create_dist: local matrices must have ns + nf + np rows (this rank's rows)");
    // this rank's rows are [row_start, row_start + nloc) of the caller's numbering
    std::vector<char> seen(nloc, 0);
    auto check_local = [&](const int32_t *is, int64_t m, const char *name) {
        for (int64_t i = 0; i < m; ++i) {
            const int64_t l = (int64_t)is[i] - row_start;
            if (l < 0 || l >= nloc) throw Error(std::string(name) + ": index not owned by this rank");
            if (i && is[i] <= is[i - 1]) throw Error(std::string(name) + ": must be sorted ascending and unique");
            if (seen[l]) throw Error(std::string(name) + ": overlaps another field");
            seen[l] = 1;
        }
    };
    check_local(is_s, ns, "is_s");
    check_local(is_f, nf, "is_f");
    check_local(is_p, np, "is_p");
    // internal local order and the field counts the Dist sees
    std::vector<int64_t> order(is_s, is_s + ns);  // caller global indices in internal local order
    int64_t cnt[3] = {ns, nf, np};
    if (three_way) {
        order.insert(order.end(), is_f, is_f + nf);
        order.insert(order.end(), is_p, is_p + np);
    } else {
        std::vector<int64_t> fp(is_f, is_f + nf);
        fp.insert(fp.end(), is_p, is_p + np);
        std::sort(fp.begin(), fp.end());
        std::vector<char> isf(nloc, 0);
        for (int64_t i = 0; i < nf; ++i) isf[is_f[i] - row_start] = 1;
        for (size_t t = 0; t < fp.size(); ++t) (isf[fp[t] - row_start] ? out.fp_is_f : out.fp_is_p).push_back((int32_t)t);
        order.insert(order.end(), fp.begin(), fp.end());
        cnt[1] = nf + np;
        cnt[2] = 0;
    }
    // every rank's field counts -> ownership ranges of the internal numbering
    std::vector<int64_t> all((size_t)3 * G);
    cm->allgather_host(cnt, sizeof(int64_t) * 3, all.data());
    std::vector<int64_t> counts[3];
    int64_t maxloc = 0;
    for (int f = 0; f < 3; ++f) counts[f].resize(G);
    for (int q = 0; q < G; ++q) {
        int64_t t = 0;
        for (int f = 0; f < 3; ++f) t += (counts[f][q] = all[(size_t)q * 3 + f]);
        maxloc = std::max(maxloc, t);
    }
    out.dist.init_counts(counts, r, G);
    const Dist &D = out.dist;
    const int64_t nglob = D.n[0] + D.n[1] + D.n[2];
    if (A->ncols != nglob || P->ncols != nglob || (Pdiff && Pdiff->ncols != nglob))
        throw Error("pls_create_dist: matrix columns must span the global system (sum of every rank's rows)");
    // caller global index -> internal global index, from every rank's order
    std::vector<int64_t> mine(maxloc, -1), every((size_t)maxloc * G);
    std::copy(order.begin(), order.end(), mine.begin());
    cm->allgather_host(mine.data(), sizeof(int64_t) * maxloc, every.data());
    std::vector<int32_t> cmap(nglob, -1);
    for (int q = 0; q < G; ++q) {
        int64_t k = 0;
        for (int f = 0; f < 3; ++f)
            for (int64_t i = 0; i < counts[f][q]; ++i, ++k) {
                const int64_t g = every[(size_t)q * maxloc + k];
                if (g < 0 || g >= nglob || cmap[g] >= 0) throw Error("pls_create_dist: index sets do not partition 0..n-1");
                cmap[g] = (int32_t)(D.off[f] + D.start[f][q] + i);
            }
    }
    // local rows in internal order, columns in the internal global numbering
    auto upload = [&](const pls_csr *M, DevCSR &dst) {
        std::vector<int64_t> rp(nloc + 1, 0);
        for (int64_t i = 0; i < nloc; ++i) {
            const int64_t o = order[i] - row_start;
            rp[i + 1] = rp[i] + (M->row_ptr[o + 1] - M->row_ptr[o]);
        }
        std::vector<int32_t> ci(rp[nloc]);
        std::vector<double> v(rp[nloc]);
        std::vector<std::pair<int32_t, double>> row;
        for (int64_t i = 0; i < nloc; ++i) {
            const int64_t o = order[i] - row_start;
            row.clear();
            for (int64_t k = M->row_ptr[o]; k < M->row_ptr[o + 1]; ++k) {
                const int32_t cc = M->col[k];
                if (cc < 0 || cc >= nglob) throw Error("pls_create_dist: column index out of range");
                row.emplace_back(cmap[cc], M->val[k]);
            }
            std::sort(row.begin(), row.end(), [](auto &a, auto &b) { return a.first < b.first; });
            for (size_t t = 0; t < row.size(); ++t) {
                ci[rp[i] + t] = row[t].first;
                v[rp[i] + t] = row[t].second;
            }
        }
        upload_csr(dst, nloc, nglob, rp.data(), ci.data(), v.data(), c);
    };
    upload(A, out.A);
    upload(P, out.P);
    if (Pdiff) {
        upload(Pdiff, out.Pd);
        out.have_Pd = true;
    }
    out.perm.resize(nloc);
    for (int64_t i = 0; i < nloc; ++i) out.perm[i] = order[i] - row_start;
    return out;
}

}  // namespace pls
