// synthetic.cpp -- the synthetic system's host side (synthetic.hpp).
#include "synthetic.hpp"

#include <algorithm>

namespace pls {

static inline uint64_t mix64h(uint64_t z) {
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static inline uint64_t hash3h(uint64_t s, uint64_t a, uint64_t b) { return mix64h(mix64h(mix64h(s) ^ a) ^ b); }

void SynthHost::init(const pls_synth_spec &s) {
    dim = s.dim;
    N = s.N;
    seed = s.seed;
    delta = s.delta;
    if (N < 1 || (dim != 2 && dim != 3)) throw Error("synthetic spec: dim must be 2 or 3 and N >= 1");
    const int64_t q = 2 * (int64_t)N + 1, v = (int64_t)N + 1;
    if (dim == 3) {
        n[0] = n[1] = 3 * q * q * q;
        n[2] = v * v * v;
        W[0] = W[1] = 6 * q * q;
        W[2] = v * v + v + 1;
        const int c[6] = {85, 85, 8, 85, 8, 15};
        std::copy(c, c + 6, cnt);
    } else {
        n[0] = n[1] = 2 * q * q;
        n[2] = v * v;
        W[0] = W[1] = 4 * q;
        W[2] = v + 1;
        const int c[6] = {23, 23, 5, 23, 5, 7};
        std::copy(c, c + 6, cnt);
    }
    off[0] = 0;
    off[1] = n[0];
    off[2] = n[0] + n[1];
    if (n[0] + n[1] + n[2] >= (int64_t)INT32_MAX) throw Error("synthetic system too large for int32 columns");
    static const int colf[6] = {0, 1, 2, 1, 2, 2};
    for (int b = 0; b < 6; ++b) {
        const bool sym = (b == 0 || b == 1 || b == 3 || b == 5);
        const int want = cnt[b];
        const int half = sym ? want / 2 : want;
        const int64_t Wb = W[colf[b]];
        const uint64_t range = sym ? (uint64_t)Wb : (uint64_t)(2 * Wb + 1);
        if ((uint64_t)half > range) throw Error("synthetic spec: band too narrow for N");
        uint64_t st = hash3h(seed ^ 0x0FF5E7ULL, (uint64_t)b, 0x51ULL);
        std::vector<int32_t> tmp;
        while ((int)tmp.size() < half) {
            st = mix64h(st);
            const int64_t d = sym ? (int64_t)(1 + st % range) : (int64_t)(st % range) - Wb;
            if (std::find(tmp.begin(), tmp.end(), (int32_t)d) == tmp.end()) tmp.push_back((int32_t)d);
        }
        offs[b].clear();
        if (sym) {
            for (int32_t d : tmp) { offs[b].push_back(d); offs[b].push_back(-d); }
            offs[b].push_back(0);
        } else {
            offs[b] = tmp;
        }
        std::sort(offs[b].begin(), offs[b].end());
    }
}

bool SynthHost::is_bc(int64_t ip) const { return (hash3h(seed ^ 0x00BC00ULL, (uint64_t)ip, 7ULL) & 15ULL) == 0ULL; }

SynthSystem generate_synthetic(const SynthHost &S, const Dist &Dd, bool three_way, Ctx &c) {
    SynthSystem out;
    const int64_t n = Dd.nloc;
    const int64_t nglob = S.n[0] + S.n[1] + S.n[2];
    out.offs.alloc(6 * 128);
    auto D = std::make_unique<SynthDev>();
    *D = SynthDev{};
    D->dim = S.dim;
    D->seed = S.seed;
    D->delta = S.delta;
    for (int f = 0; f < 3; ++f) {
        D->n[f] = S.n[f];
        D->off[f] = S.off[f];
        D->rlo[f] = Dd.lo[f];
        D->rlen[f] = Dd.len[f];
        D->rloff[f] = Dd.loff[f];
    }
    D->nrows = n;
    for (int b = 0; b < 6; ++b) {
        D->cnt[b] = S.cnt[b];
        HIPCHK(hipMemcpy(out.offs.p + b * 128, S.offs[b].data(), sizeof(int32_t) * S.cnt[b], hipMemcpyHostToDevice));
        D->offs[b] = out.offs.p + b * 128;
    }
    // pattern (shared by A, P, P_diff)
    DBuf<int64_t> len(n + 1);
    launch_synth_count(*D, len.p, c.st);
    out.A.rp.alloc(n + 1);
    c.ensure_scan(n);
    exclusive_scan_i64(len.p, out.A.rp.p, n, c.scan_tmp.p, c.scan_tmp_bytes, c.st);
    int64_t nnz = 0;
    HIPCHK(hipMemcpyAsync(&nnz, out.A.rp.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, c.st));
    c.sync();
    auto gen = [&](DevCSR &M, int variant) {
        M.nrows = n; M.ncols = nglob; M.nnz = nnz;
        if (!M.rp.p) {
            M.rp.alloc(n + 1);
            HIPCHK(hipMemcpyAsync(M.rp.p, out.A.rp.p, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToDevice, c.st));
        }
        M.ci.alloc(std::max<int64_t>(nnz, 1));
        M.val.alloc(std::max<int64_t>(nnz, 1));
        launch_synth_fill(*D, variant, M.rp.p, M.ci.p, M.val.p, c.st);
        HIPCHK(hipGetLastError());
    };
    gen(out.A, 0);
    gen(out.P, 1);
    if (three_way) gen(out.Pd, 2);
    c.sync();
    for (int64_t i = Dd.lo[2]; i < Dd.lo[2] + Dd.len[2]; ++i)
        if (S.is_bc(i)) out.bcs.push_back((int32_t)(i - Dd.lo[2]));
    out.rows = std::move(D);
    return out;
}

}  // namespace pls
