// fracsum_pcs_demo.cpp -- a range check over committed tables with ONE commitment phase, end to end, no Python in the loop: a table
// t = 0 .. 2^k - 1, a column f of 2^n values from it and the multiplicities m.  Commit f, and t with m in one batch, with WHIR
// (provekit::WhirPcs); prove the lookup with the two roots bound (provekit::GkrLookup, include/provekit_fracsum.hpp): no helper column
// exists, so nothing else is ever committed; verify the proof on the host; then open f at z_F and {t, m} at z_T -- two openings -- and see
// that the evaluations the openings bind are the three claims: the condition under which "accepted" holds.  Then the error paths.
//
//   fracsum_pcs_demo [n = 12] [k = 8] [seed = 7]
#include <cstdio>
#include <cstdlib>

#include "provekit_fracsum.hpp"
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

int main(int argc, char** argv) {
    const unsigned n = argc > 1 ? std::atoi(argv[1]) : 12, k = argc > 2 ? std::atoi(argv[2]) : 8;
    uint64_t rng = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 7;
    try {
        Context ctx(0);
        const size_t N = (size_t)1 << n, K = (size_t)1 << k;
        std::vector<FieldElement> t(K), m(K, FieldElement{0, 0, 0, 0}), f(N);
        for (size_t y = 0; y < K; y++) t[y] = {y, 0, 0, 0};
        for (size_t x = 0; x < N; x++) {
            const size_t y = splitmix(rng) % K;
            f[x] = t[y], m[y][0]++;
        }
        const DeviceVec d_f = montgomery(ctx, f), d_t = montgomery(ctx, t), d_m = montgomery(ctx, m);

        // the one commitment phase: everything the argument will ever need is committed before alpha exists
        const WhirConfig cfg_n = WhirConfig::for_size(n, 8.0, 1), cfg_k = WhirConfig::for_size(k, 8.0, 2);
        WhirPcs pcs_n(ctx, cfg_n), pcs_k(ctx, cfg_k);
        const PcsCommitment com_f = pcs_n.commit({&d_f}), com_tm = pcs_k.commit({&d_t, &d_m});
        const std::vector<FieldElement> bind{as_element(ctx, com_f.root()), as_element(ctx, com_tm.root())};
        GkrLookup prover(ctx, n, k, 2);
        const GkrLookupProof proof = prover.prove(d_f, d_t, d_m, bind);

        const GkrLookupVerdict ok = GkrLookup::verify(prover.statement(), proof.proof, bind);
        if (!ok) throw Error(-200, "a valid lookup proof was rejected: " + ok.message);
        const GkrLookupClaims& c = ok.claims;
        if (c.z_f != proof.claims.z_f || c.z_t != proof.claims.z_t || c.f_value != proof.claims.f_value || c.t_value != proof.claims.t_value ||
            c.m_value != proof.claims.m_value || c.alpha != proof.claims.alpha)
            throw Error(-201, "the verifier derived other claims than the prover returned");

        // accepted PROVIDED the three claims hold: the commitment scheme proves them, with two openings
        size_t opening_bytes = 0;
        auto opened = [&](const WhirPcs& pcs, const WhirConfig& cfg, const PcsCommitment& com, const Point& point, const std::vector<FieldElement>& claimed,
                          const char* what) {
            const PcsOpening opening = pcs.open(com, {point});
            const std::array<uint8_t, 32> root = com.root();
            std::vector<FieldElement> bound;
            const PcsVerdict v = WhirPcs::verify(cfg, {point}, opening.proof, &root, &bound);
            if (!v) throw Error(-202, std::string("a valid opening of ") + what + " was rejected: " + v.message);
            if (bound != claimed) throw Error(-203, std::string("the committed ") + what + " does not take the claimed values");
            opening_bytes += opening.proof.size();
        };
        opened(pcs_n, cfg_n, com_f, c.z_f, {c.f_value}, "f");
        opened(pcs_k, cfg_k, com_tm, c.z_t, {c.t_value, c.m_value}, "t and m");
        std::printf("ok n=%u k=%u lookup_bytes=%zu opening_bytes=%zu commitments=2 phases=1 openings=2\n", n, k, proof.proof.size(), opening_bytes);

        // the error paths: an entry outside the table, another root
        {
            std::vector<FieldElement> bad_f = f;
            bad_f[N / 3] = {K, 0, 0, 0};  // one past the range
            const DeviceVec d_bad = montgomery(ctx, bad_f);
            try {
                prover.prove(d_bad, d_t, d_m, bind);
                throw Error(-204, "a column with an entry outside the table was taken");
            } catch (const Error& e) {
                if (e.code != PK_ERR_UNSATISFIED) throw;
                std::printf("one entry outside the table: refused rc=%d (%s)\n", e.code, e.what());
            }
            if (prover.prove(d_f, d_t, d_m, bind).proof != proof.proof) throw Error(-205, "the prover did not stay usable");
        }
        const GkrLookupVerdict other_root = GkrLookup::verify(prover.statement(), proof.proof, {bind[1], bind[0]});
        if (other_root) throw Error(-206, "the proof was accepted under other roots");
        std::printf("another root: rejected, side=%d layer=%u check=%s\n", other_root.side, other_root.layer, other_root.check_name());
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
