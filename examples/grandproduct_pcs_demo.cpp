// grandproduct_pcs_demo.cpp -- a permutation check over committed columns, end to end, no Python in the loop: a column a of 2^n values
// and a column b that holds the same values in another order.  Commit both with WHIR (provekit::WhirPcs); prove that they are equal
// as multisets with the two roots bound (provekit::MultisetEquality, include/provekit_grandproduct.hpp) -- no further commitment;
// verify the proof on the host; then open each commitment at its point and see that the evaluation the opening binds is the claim:
// the condition under which "accepted" holds.  Then the error paths: one entry changed, another root.
//
//   grandproduct_pcs_demo [n = 12] [seed = 7]
#include <cstdio>
#include <cstdlib>

#include "provekit_grandproduct.hpp"
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
    const unsigned n = argc > 1 ? std::atoi(argv[1]) : 12;
    uint64_t rng = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 7;
    try {
        Context ctx(0);
        const size_t N = (size_t)1 << n;
        std::vector<FieldElement> a(N), b;
        for (size_t x = 0; x < N; x++) a[x] = {splitmix(rng), splitmix(rng), splitmix(rng), splitmix(rng) >> 4};  // below 2^252 < p
        b = a;
        for (size_t x = N - 1; x > 0; x--) std::swap(b[x], b[splitmix(rng) % (x + 1)]);
        const DeviceVec d_a = montgomery(ctx, a), d_b = montgomery(ctx, b);

        const WhirConfig cfg = WhirConfig::for_size(n, 8.0, 1);
        WhirPcs pcs(ctx, cfg);
        const PcsCommitment com_a = pcs.commit({&d_a}), com_b = pcs.commit({&d_b});
        const std::vector<FieldElement> bind{as_element(ctx, com_a.root()), as_element(ctx, com_b.root())};
        MultisetEquality prover(ctx, n, 1, 2);
        const MultisetProof proof = prover.prove({&d_a}, {&d_b}, bind);

        const MultisetVerdict ok = MultisetEquality::verify(prover.statement(), proof.proof, bind);
        if (!ok) throw Error(-200, "a valid multiset proof was rejected: " + ok.message);
        const MultisetClaims& c = ok.claims;
        if (c.z_a != proof.claims.z_a || c.z_b != proof.claims.z_b || c.comb_a != proof.claims.comb_a || c.comb_b != proof.claims.comb_b)
            throw Error(-201, "the verifier derived other claims than the prover returned");

        // accepted PROVIDED the two claims hold: the commitment scheme proves them (one column per side: the combination is the column)
        size_t opening_bytes = 0;
        auto opened = [&](const PcsCommitment& com, const Point& point, const FieldElement& claimed, const char* what) {
            const PcsOpening opening = pcs.open(com, {point});
            const std::array<uint8_t, 32> root = com.root();
            std::vector<FieldElement> bound;
            const PcsVerdict v = WhirPcs::verify(cfg, {point}, opening.proof, &root, &bound);
            if (!v) throw Error(-202, std::string("a valid opening of ") + what + " was rejected: " + v.message);
            if (bound != std::vector<FieldElement>{claimed}) throw Error(-203, std::string("the committed ") + what + " does not take the claimed value");
            opening_bytes += opening.proof.size();
        };
        opened(com_a, c.z_a, c.comb_a, "a");
        opened(com_b, c.z_b, c.comb_b, "b");
        std::printf("ok n=%u multiset_bytes=%zu opening_bytes=%zu\n", n, proof.proof.size(), opening_bytes);

        // the error paths: one entry changed, another root
        {
            std::vector<FieldElement> bad_b = b;
            bad_b[N / 3][0] ^= 1;
            const DeviceVec d_bad = montgomery(ctx, bad_b);
            try {
                prover.prove({&d_a}, {&d_bad}, bind);
                throw Error(-204, "two different multisets were taken");
            } catch (const Error& e) {
                if (e.code != PK_ERR_UNSATISFIED) throw;
                std::printf("one entry changed: refused rc=%d (%s)\n", e.code, e.what());
            }
            if (prover.prove({&d_a}, {&d_b}, bind).proof != proof.proof) throw Error(-205, "the prover did not stay usable");
        }
        const MultisetVerdict other_root = MultisetEquality::verify(prover.statement(), proof.proof, {bind[1], bind[0]});
        if (other_root) throw Error(-206, "the proof was accepted under other roots");
        std::printf("another root: rejected, side=%d layer=%u check=%s\n", other_root.side, other_root.layer, other_root.check_name());
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
