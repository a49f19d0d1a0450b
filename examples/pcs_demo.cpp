// pcs_demo.cpp -- WHIR as a polynomial commitment scheme, no Python in the loop: commit to two multilinear polynomials, open them
// at two points, verify on the host, then change one evaluation in the proof and see the rejection (provekit::WhirPcs,
// include/provekit_whir.hpp).
//
//   pcs_demo <n_vars> <seed>
#include <cstdio>
#include <cstdlib>

#include "provekit_whir.hpp"

using namespace provekit;

static uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
static FieldElement random_element(uint64_t& s) { return {splitmix(s), splitmix(s), splitmix(s), splitmix(s) >> 6}; }  // < 2^250 < p

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s n_vars seed\n", argv[0]);
        return 2;
    }
    const unsigned n = std::atoi(argv[1]);
    uint64_t rng = std::strtoull(argv[2], nullptr, 10);
    try {
        Context ctx(0);
        const WhirConfig cfg = WhirConfig::for_size(n, 8.0, 2);
        WhirPcs pcs(ctx, cfg);
        std::vector<FieldElement> f((size_t)1 << n), g((size_t)1 << n);
        for (auto& x : f) x = random_element(rng);
        for (auto& x : g) x = random_element(rng);
        DeviceVec d_f(ctx, f), d_g(ctx, g);
        const PcsCommitment com = pcs.commit({&d_f, &d_g});  // the points are not known yet
        const std::array<uint8_t, 32> root = com.root();

        std::vector<Point> points(2, Point(n));
        for (Point& p : points)
            for (FieldElement& x : p) x = random_element(rng);
        const PcsOpening opening = pcs.open(com, points);

        std::vector<FieldElement> bound;
        const PcsVerdict ok = WhirPcs::verify(cfg, points, opening.proof, &root, &bound);
        if (!ok) throw Error(-200, "a valid opening was rejected: " + ok.message);
        if (bound != opening.evaluations) throw Error(-201, "the verifier read other evaluations than the prover returned");

        // the evaluations sit behind the root, the OOD answers, beta's absence from the bytes, and the points
        const size_t first_eval = 32 + 32 * (size_t)cfg.to_c().commitment_ood_samples * 2 + 32 * (size_t)n * points.size();
        std::vector<uint8_t> bad = opening.proof;
        bad[first_eval] ^= 1;
        const PcsVerdict no = WhirPcs::verify(cfg, points, bad, &root);
        if (no) throw Error(-202, "an opening with a changed evaluation was accepted");
        std::printf("ok n_vars=%u points=%zu proof_bytes=%zu\n", n, points.size(), opening.proof.size());
        std::printf("changed evaluation at byte %zu: rejected, check=%s at offset %llu (%s)\n", first_eval, no.check_name(), (unsigned long long)no.offset,
                    no.message.c_str());
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
