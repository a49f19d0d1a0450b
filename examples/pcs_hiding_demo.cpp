// pcs_hiding_demo.cpp -- a HIDING opening over a WHIR commitment, no Python in the loop: commit to one multilinear polynomial of n
// variables under a mask (the committed batch is [f || mask] and a random g, in n + 1 variables), open it at two points, verify on
// the host, see a second opening of the same commitment refused, and see a tampered proof rejected (provekit::WhirPcs,
// provekit_whir.hpp; provekit_whir_hiding.h states the construction).
//
//   pcs_hiding_demo <n> <seed>
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
        std::fprintf(stderr, "usage: %s n seed\n", argv[0]);
        return 2;
    }
    const unsigned n = std::atoi(argv[1]);
    uint64_t rng = std::strtoull(argv[2], nullptr, 10);
    try {
        Context ctx(0);
        WhirConfig cfg = WhirConfig::for_size(n + 1, 8.0, 2);  // what is committed: n + 1 variables, f^ and g
        // the mask budget: the values of f^ that leave through the first opened codeword (num_queries[0], or final_queries for a config
        // without rounds) must not outnumber the 2^n mask coefficients.  A small demo size gets there with fewer queries than the
        // derived config has -- less soundness, a demo's choice
        const size_t mask = (size_t)1 << n, per_query = (size_t)1 << cfg.folding_factor;
        if (n > 27 || mask < cfg.commitment_ood_samples + per_query) {
            std::fprintf(stderr, "n = %u: the mask budget needs 2^n >= %zu (one query of 2^folding_factor values and the out-of-domain answers)\n", n,
                         cfg.commitment_ood_samples + per_query);
            return 2;
        }
        unsigned& first = cfg.num_queries.empty() ? cfg.final_queries : cfg.num_queries[0];
        if (cfg.commitment_ood_samples + first * per_query > mask) {
            first = (unsigned)((mask - cfg.commitment_ood_samples) / per_query);
            std::printf("n = %u is small: %s lowered to %u to keep the mask budget\n", n, cfg.num_queries.empty() ? "final_queries" : "num_queries[0]", first);
        }
        WhirPcs pcs = WhirPcs::hiding(ctx, cfg);
        std::vector<FieldElement> f(mask);
        for (auto& x : f) x = random_element(rng);
        DeviceVec d_f(ctx, f);
        PcsHidingCommitment com = pcs.commit_hiding({&d_f});  // the key of the mask and g comes from the OS
        const std::array<uint8_t, 32> root = com.root();
        PcsHidingCommitment again = pcs.commit_hiding({&d_f});
        if (again.root() == root) throw Error(-206, "two commitments to one polynomial share a root: the masks were not fresh");

        std::vector<Point> points(2, Point(n));
        for (Point& p : points)
            for (FieldElement& x : p) x = random_element(rng);
        const PcsOpening opening = pcs.open_hiding(com, points);

        std::vector<FieldElement> bound;
        const PcsVerdict ok = WhirPcs::verify_hiding(cfg, points, opening.proof, &root, &bound);
        if (!ok) throw Error(-200, "a valid hiding opening was rejected: " + ok.message);
        if (bound != opening.evaluations) throw Error(-201, "the verifier read other evaluations than the prover returned");

        bool refused = false;
        try {
            pcs.open_hiding(com, points);
        } catch (const Error& e) {
            refused = e.code == PK_ERR_BAD_ARG;
            std::printf("a second opening: refused (%s)\n", e.what());
        }
        if (!refused) throw Error(-202, "a hiding commitment was opened twice");

        std::vector<uint8_t> tampered = opening.proof;
        tampered[tampered.size() / 2] ^= 1;
        const PcsVerdict no = WhirPcs::verify_hiding(cfg, points, tampered, &root);
        if (no) throw Error(-203, "a tampered proof was accepted");
        std::printf("ok n=%u points=%zu proof_bytes=%zu\n", n, points.size(), opening.proof.size());
        std::printf("one bit changed: rejected, check=%s at offset %llu (%s)\n", no.check_name(), (unsigned long long)no.offset, no.message.c_str());
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
