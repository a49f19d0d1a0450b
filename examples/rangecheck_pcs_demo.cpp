// rangecheck_pcs_demo.cpp -- a 32-bit range check over committed columns, end to end, no Python in the loop: a column f of 2^n values
// below 2^32, split on the device into three limbs of 12 bits (the top one of 8) with their multiplicities in 0 .. 2^12 - 1
// (provekit::RangeCheck, include/provekit_rangecheck.hpp).  Commit {f, limb_0, limb_1, limb_2} and m with WHIR (provekit::WhirPcs),
// before any challenge exists; prove the range check with the two roots bound; verify it on the host; open the batch at z_lo and m at
// z_T -- two openings -- and check the three claims on the values the openings bind (RangeCheck::check_claims).  Then the refusals: a
// value of 2^32 in the column, and limbs that recompose but whose top limb is 2^8.
//
//   rangecheck_pcs_demo [n = 10] [seed = 7]
#include <cstdio>
#include <cstdlib>

#include "provekit_rangecheck.hpp"
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
    const unsigned n = argc > 1 ? std::atoi(argv[1]) : 10, bits = 32, k = 12;
    uint64_t rng = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 7;
    try {
        Context ctx(0);
        const size_t N = (size_t)1 << n, K = (size_t)1 << k;
        std::vector<FieldElement> f(N);
        for (size_t x = 0; x < N; x++) f[x] = {splitmix(rng) >> 32, 0, 0, 0};
        f[0] = {0, 0, 0, 0}, f[1] = {0xffffffffull, 0, 0, 0};
        const DeviceVec d_f = montgomery(ctx, f);

        RangeCheck prover(ctx, n, bits, k, 2);
        const unsigned L = prover.limbs();  // 3
        std::vector<DeviceVec> limbs;
        for (unsigned i = 0; i < L; i++) limbs.emplace_back(ctx, N);
        DeviceVec d_m(ctx, K);
        prover.decompose(d_f, {&limbs[0], &limbs[1], &limbs[2]}, d_m);
        const std::vector<const DeviceVec*> limb_cols{&limbs[0], &limbs[1], &limbs[2]};

        // the one commitment phase: the column and its limbs in a batch, m by itself, before the seed exists
        const WhirConfig cfg_n = WhirConfig::for_size(n, 8.0, L + 1), cfg_k = WhirConfig::for_size(k, 8.0, 1);
        WhirPcs pcs_n(ctx, cfg_n), pcs_k(ctx, cfg_k);
        const PcsCommitment com_f = pcs_n.commit({&d_f, &limbs[0], &limbs[1], &limbs[2]}), com_m = pcs_k.commit({&d_m});
        const std::vector<FieldElement> bind{as_element(ctx, com_f.root()), as_element(ctx, com_m.root())};
        const RangeProof proof = prover.prove(limb_cols, d_m, bind);

        const RangeVerdict ok = RangeCheck::verify(prover.statement(), proof.proof, bind);
        if (!ok) throw Error(-200, "a valid range proof was rejected: " + ok.message);
        const RangeClaims& cl = ok.claims;
        if (cl.z_lo != proof.claims.z_lo || cl.z_t != proof.claims.z_t || cl.limbs_value != proof.claims.limbs_value || cl.m_value != proof.claims.m_value)
            throw Error(-201, "the verifier derived other claims than the prover returned");
        std::printf("accepted n=%u bits=%u k=%u limbs=%u proof_bytes=%zu\n", n, bits, k, L, proof.proof.size());

        // accepted PROVIDED the three claims hold: the commitment scheme gives the evaluations, with one opening per commitment
        size_t opening_bytes = 0;
        auto opened = [&](const WhirPcs& pcs, const WhirConfig& cfg, const PcsCommitment& com, const Point& point, const char* what) {
            const PcsOpening opening = pcs.open(com, {point});
            const std::array<uint8_t, 32> root = com.root();
            std::vector<FieldElement> bound;
            const PcsVerdict v = WhirPcs::verify(cfg, {point}, opening.proof, &root, &bound);
            if (!v) throw Error(-202, std::string("a valid opening of ") + what + " was rejected: " + v.message);
            opening_bytes += opening.proof.size();
            return bound;
        };
        const std::vector<FieldElement> cols = opened(pcs_n, cfg_n, com_f, cl.z_lo, "f and its limbs"), m_eval = opened(pcs_k, cfg_k, com_m, cl.z_t, "m");
        const std::vector<FieldElement> limb_evals(cols.begin() + 1, cols.end());
        const int which = RangeCheck::check_claims(prover.statement(), cl, cols[0], limb_evals, m_eval[0]);
        if (which != PKR_CLAIM_NONE) throw Error(-203, "the committed columns do not take the claimed values: claim " + std::to_string(which));
        FieldElement other = cols[0];
        other[0] ^= 1;  // f's evaluation changed: the recomposition fails
        if (RangeCheck::check_claims(prover.statement(), cl, other, limb_evals, m_eval[0]) != PKR_CLAIM_RECOMPOSE) throw Error(-204, "a changed evaluation passed the claims");
        std::printf("claims hold: opening_bytes=%zu commitments=2 phases=1 openings=2\n", opening_bytes);

        // a value of 2^32 in the column: the decomposition refuses it and names the entry
        {
            std::vector<FieldElement> bad = f;
            bad[7] = {1ull << 32, 0, 0, 0};
            const DeviceVec d_bad = montgomery(ctx, bad);
            std::vector<DeviceVec> scratch;
            for (unsigned i = 0; i < L; i++) scratch.emplace_back(ctx, N);
            DeviceVec m_scratch(ctx, K);
            uint64_t first_bad = 0;
            try {
                prover.decompose(d_bad, {&scratch[0], &scratch[1], &scratch[2]}, m_scratch, &first_bad);
                throw Error(-205, "a value of 2^32 was taken");
            } catch (const Error& e) {
                if (e.code != PK_ERR_UNSATISFIED || first_bad != 7) throw;
                std::printf("a value of 2^32: refused rc=%d (%s)\n", e.code, e.what());
            }
        }
        // limbs (lo, mid, 2^8) recompose 2^32 + its low 24 bits, and every limb is below 2^12: the top check refuses them
        {
            std::vector<FieldElement> top = limbs[2].to_host();
            const DeviceVec one = montgomery(ctx, {FieldElement{1ull << 8, 0, 0, 0}});
            top[7] = one.to_host()[0];
            const DeviceVec d_top(ctx, top);
            try {
                prover.prove({&limbs[0], &limbs[1], &d_top}, d_m, bind);
                throw Error(-206, "a top limb of 2^8 was taken");
            } catch (const Error& e) {
                if (e.code != PK_ERR_UNSATISFIED) throw;
                std::printf("a top limb of 2^8: refused rc=%d (%s)\n", e.code, e.what());
            }
            if (prover.prove(limb_cols, d_m, bind).proof != proof.proof) throw Error(-207, "the prover did not stay usable");
        }
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
