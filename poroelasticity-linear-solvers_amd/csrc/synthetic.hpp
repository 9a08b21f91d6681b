// synthetic.hpp -- the synthetic system's host side (synthetic.cpp): the
// offsets of every forward block, and a rank's rows of A, P, P_diff generated
// directly in HBM.
#pragma once
#include "dist.hpp"

namespace pls {

// Offsets per forward block (SURVEY.md 8(d) spec; same definition as the CPU
// oracle so both build the identical matrix).
struct SynthHost {
    int dim = 3, N = 1;
    uint64_t seed = 0;
    double delta = 0.05;
    int64_t n[3] = {0, 0, 0}, off[3] = {0, 0, 0}, W[3] = {0, 0, 0};
    int cnt[6] = {0};
    std::vector<int32_t> offs[6];
    void init(const pls_synth_spec &s);
    bool is_bc(int64_t ip) const;
};

// The rows of the slabs D on the device (global columns); P_diff with `three_way`.
struct SynthSystem {
    std::unique_ptr<SynthDev> rows;  // row map (the rhs generator reads it); its offsets live in `offs`
    DBuf<int32_t> offs;
    DevCSR A, P, Pd;
    std::vector<int32_t> bcs;  // BC positions inside the rank's p sub-vector
};
SynthSystem generate_synthetic(const SynthHost &S, const Dist &D, bool three_way, Ctx &c);

}  // namespace pls
