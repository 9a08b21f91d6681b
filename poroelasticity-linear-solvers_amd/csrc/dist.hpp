// dist.hpp -- row-slab distribution (dist.cpp): which rows of every field a
// rank owns, local matrices turned into distributed ones (halo plan), and a
// rank's share of a caller-assembled system brought into the internal order.
#pragma once
#include "runtime.hpp"

namespace pls {

// Row slabs per field (the analogue of PETSc MPIAIJ ownership ranges): rank r
// owns rows [lo_f, lo_f + len_f) of every field f; local layout [s_r | f_r | p_r].
// Synthetic systems use PETSc's split (the first n % size ranks one row
// more); caller matrices (pls_create_dist) bring their own per-rank counts --
// the rows each rank's index sets select, as PETSc's createSubMatrix keeps them.
struct Dist {
    int rank = 0, size = 1;
    int64_t n[3] = {0, 0, 0}, off[3] = {0, 0, 0}, lo[3] = {0, 0, 0}, len[3] = {0, 0, 0}, loff[3] = {0, 0, 0};
    int64_t nloc = 0;
    std::vector<int64_t> start[3];  // start[f][q]: first row of field f owned by rank q (size + 1 entries)
    static void slab(int64_t N, int size, int r, int64_t &lo, int64_t &len);
    void range(int f, int q, int64_t &lo_, int64_t &len_) const {
        lo_ = start[f][q];
        len_ = start[f][q + 1] - lo_;
    }
    // counts[f][q] = rows of field f on rank q
    void init_counts(const std::vector<int64_t> counts[3], int r, int s);
    void init(const int64_t nf[3], int r, int s);
};

// Turn a local-row matrix whose columns are indices into the column space of
// fields [f0, f1] (0 = first column of field f0) into a distributed matrix:
// owned columns -> local index (my slabs of those fields, field order), other
// referenced columns -> ghosts nlocal + position (owner-major, then global),
// plus the halo plan.  Builds the SELL-64 copy.
void make_dist(DevCSR &M, const Dist &D, int f0, int f1, Comm *comm, Ctx &c);

// A rank's share of a caller-assembled system (pls_create_dist), uploaded:
// local rows in the internal order, columns in the internal global numbering.
struct ShardedRows {
    Dist dist;
    std::vector<int64_t> perm;              // internal local row -> the caller's local row
    std::vector<int32_t> fp_is_f, fp_is_p;  // 2-way: f / p positions inside the rank's sorted fp set
    DevCSR A, P, Pd;
    bool have_Pd = false;
};
ShardedRows shard_rows(const pls_csr *A, const pls_csr *P, const pls_csr *Pdiff, int64_t row_start, const int32_t *is_s,
                       int64_t ns, const int32_t *is_f, int64_t nf, const int32_t *is_p, int64_t np, bool three_way,
                       Comm *cm, Ctx &c);

}  // namespace pls
