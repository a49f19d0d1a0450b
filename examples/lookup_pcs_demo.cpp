// lookup_pcs_demo.cpp -- a range check over committed tables, end to end, no Python in the loop: a table t = 0 .. 2^k - 1 and a column f
// of 2^n values from it.  Commit f, t and the multiplicities m with WHIR (provekit::WhirPcs); begin the lookup proof with the three roots
// bound (provekit::Lookup, include/provekit_lookup.hpp); commit the helper columns h_f and h_t; finish with their roots bound; verify the
// proof on the host; then open every commitment at the points of the seven claims -- h_f and h_t at two points in one opening each --
// and see that the evaluations the openings bind are the claims: the condition under which "accepted" holds.  Then the error paths.
//
//   lookup_pcs_demo [n = 12] [k = 8] [seed = 7]
#include <cstdio>
#include <cstdlib>

#include "provekit_lookup.hpp"
#include "provekit_whir.hpp"

using namespace provekit;

static uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

// canonical values -> a device vector of their Montgomery images, by the library's own conversion
static DeviceVec montgomery(const Context& ctx, const std::vector<FieldElement>& canonical) {
    DeviceVec d(ctx, canonical);
    ctx.check(pk_fe_to_mont(ctx.get(), d.data(), d.data(), canonical.size()));
    return d;
}
// a root, a canonical digest, as the field element a transcript absorbs
static FieldElement as_element(const Context& ctx, const std::array<uint8_t, 32>& root) {
    FieldElement c;
    std::memcpy(c.data(), root.data(), 32);
    return montgomery(ctx, {c}).to_host()[0];
}
// the prover's arena -> a vector of the caller's own, for WhirPcs::commit
static DeviceVec copy_of(const Context& ctx, const uint64_t* d_src, size_t n) {
    DeviceVec d(ctx, n);
    ctx.check(pk_memcpy_d2d(ctx.get(), d.data(), d_src, 32 * n));
    return d;
}

struct DeviceIndices {
    const Context& ctx;
    void* p = nullptr;
    DeviceIndices(const Context& c, const std::vector<uint32_t>& v) : ctx(c) {
        c.check(pk_malloc(c.get(), 4 * v.size(), &p));
        c.check(pk_memcpy_h2d(c.get(), p, v.data(), 4 * v.size()));
    }
    ~DeviceIndices() { pk_free(ctx.get(), p); }
    const uint32_t* get() const { return static_cast<const uint32_t*>(p); }
};

int main(int argc, char** argv) {
    const unsigned n = argc > 1 ? std::atoi(argv[1]) : 12, k = argc > 2 ? std::atoi(argv[2]) : 8;
    uint64_t rng = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 7;
    try {
        Context ctx(0);
        const size_t N = (size_t)1 << n, K = (size_t)1 << k;
        std::vector<FieldElement> t(K), f(N);
        std::vector<uint32_t> idx(N);
        for (size_t y = 0; y < K; y++) t[y] = {y, 0, 0, 0};
        for (size_t x = 0; x < N; x++) idx[x] = (uint32_t)(splitmix(rng) % K), f[x] = t[idx[x]];
        const DeviceVec d_f = montgomery(ctx, f), d_t = montgomery(ctx, t);
        DeviceVec d_m(ctx, K);
        const DeviceIndices d_idx(ctx, idx);

        Lookup prover(ctx, n, k, 3, 2);
        prover.multiplicities(d_f, d_t, d_idx.get(), d_m);
        const WhirConfig cfg_n = WhirConfig::for_size(n, 8.0, 1), cfg_k = WhirConfig::for_size(k, 8.0, 1);
        WhirPcs pcs_n(ctx, cfg_n), pcs_k(ctx, cfg_k);
        const PcsCommitment com_f = pcs_n.commit({&d_f}), com_t = pcs_k.commit({&d_t}), com_m = pcs_k.commit({&d_m});
        const std::vector<FieldElement> bind{as_element(ctx, com_f.root()), as_element(ctx, com_t.root()), as_element(ctx, com_m.root())};
        const LookupHelpers helpers = prover.begin(d_t, d_idx.get(), bind);
        const DeviceVec d_hf = copy_of(ctx, helpers.h_f, N), d_ht = copy_of(ctx, helpers.h_t, K);
        const PcsCommitment com_hf = pcs_n.commit({&d_hf}), com_ht = pcs_k.commit({&d_ht});
        const std::vector<FieldElement> bind2{as_element(ctx, com_hf.root()), as_element(ctx, com_ht.root())};
        const LookupProof proof = prover.finish(bind2);

        const LookupVerdict ok = Lookup::verify(prover.statement(), proof.proof, bind, bind2);
        if (!ok) throw Error(-200, "a valid lookup proof was rejected: " + ok.message);
        const LookupClaims& c = ok.claims;
        if (c.r_f != proof.claims.r_f || c.r_t != proof.claims.r_t || c.hf_at_half != proof.claims.hf_at_half || c.alpha != helpers.alpha)
            throw Error(-201, "the verifier derived other claims than the prover returned");

        // accepted PROVIDED the seven claims hold: the commitment scheme proves them
        const FieldElement half = montgomery(ctx, {{0xa1f0fac9f8000001ULL, 0x9419f4243cdcb848ULL, 0xdc2822db40c0ac2eULL, 0x183227397098d014ULL}}).to_host()[0];  // (p + 1) / 2
        const Point half_n(n, half), half_k(k, half);
        size_t opening_bytes = 0;
        auto opened = [&](const WhirPcs& pcs, const WhirConfig& cfg, const PcsCommitment& com, const std::vector<Point>& points, const std::vector<FieldElement>& claimed,
                          const char* what) {
            const PcsOpening opening = pcs.open(com, points);
            const std::array<uint8_t, 32> root = com.root();
            std::vector<FieldElement> bound;
            const PcsVerdict v = WhirPcs::verify(cfg, points, opening.proof, &root, &bound);
            if (!v) throw Error(-202, std::string("a valid opening of ") + what + " was rejected: " + v.message);
            if (bound != claimed) throw Error(-203, std::string("the committed ") + what + " does not take the claimed values");
            opening_bytes += opening.proof.size();
        };
        opened(pcs_n, cfg_n, com_f, {c.r_f}, {c.f_at_rf}, "f");
        opened(pcs_n, cfg_n, com_hf, {c.r_f, half_n}, {c.hf_at_rf, c.hf_at_half}, "h_f");
        opened(pcs_k, cfg_k, com_t, {c.r_t}, {c.t_at_rt}, "t");
        opened(pcs_k, cfg_k, com_m, {c.r_t}, {c.m_at_rt}, "m");
        opened(pcs_k, cfg_k, com_ht, {c.r_t, half_k}, {c.ht_at_rt, c.ht_at_half}, "h_t");
        std::printf("ok n=%u k=%u lookup_bytes=%zu opening_bytes=%zu\n", n, k, proof.proof.size(), opening_bytes);

        // the error paths: a non-member entry, a changed proof byte, another root
        {
            std::vector<FieldElement> bad_f = f;
            const size_t at = N / 3;
            bad_f[at] = {K, 0, 0, 0};  // one past the range
            const DeviceVec d_bad = montgomery(ctx, bad_f);
            uint64_t first_bad = 0;
            try {
                prover.multiplicities(d_bad, d_t, d_idx.get(), d_m, &first_bad);
                throw Error(-204, "a column with a non-member entry was taken");
            } catch (const Error& e) {
                if (e.code != PK_ERR_UNSATISFIED || first_bad != at) throw;
                std::printf("non-member entry: refused at x=%llu (%s)\n", (unsigned long long)first_bad, e.what());
            }
        }
        std::vector<uint8_t> bad = proof.proof;
        bad[32 * 3] ^= 1;  // s, the F side's sum and round 0's h(0) come before it
        const LookupVerdict no = Lookup::verify(prover.statement(), bad, bind, bind2);
        if (no || no.side != PKL_SIDE_F) throw Error(-205, "a changed byte of the f side was not rejected there");
        std::printf("changed proof byte: rejected, side=%d check=%s at offset %llu (%s)\n", no.side, no.check_name(), (unsigned long long)no.offset, no.message.c_str());
        const LookupVerdict other_root = Lookup::verify(prover.statement(), proof.proof, {bind[1], bind[0], bind[2]}, bind2);
        if (other_root) throw Error(-206, "the proof was accepted under other roots");
        std::printf("another root: rejected, side=%d check=%s\n", other_root.side, other_root.check_name());
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
