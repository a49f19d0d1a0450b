// pcs_sharded_demo.cpp -- the WHIR commitment library on a device set, no Python in the loop: G ranks (here all on device 0, so the
// library joins them by its in-process transport; distinct devices get RCCL), one host thread per rank, every rank committing to the
// same two polynomials and opening them at the same two points.  Every rank must report the same root and the same proof bytes, and
// the host verifier must accept them (provekit::Context::create_set, provekit::WhirPcs).
//
//   pcs_sharded_demo <n_vars> <ranks> <seed>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "provekit_whir.hpp"

using namespace provekit;

static uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
static FieldElement random_element(uint64_t& s) { return {splitmix(s), splitmix(s), splitmix(s), splitmix(s) >> 6}; }  // < 2^250 < p

struct RankResult {
    std::array<uint8_t, 32> root{};
    PcsOpening opening;
    std::string error;
};

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s n_vars ranks seed\n", argv[0]);
        return 2;
    }
    const unsigned n = std::atoi(argv[1]);
    const int G = std::atoi(argv[2]);
    uint64_t rng = std::strtoull(argv[3], nullptr, 10);
    try {
        const WhirConfig cfg = WhirConfig::for_size(n, 8.0, 2);
        std::vector<FieldElement> f((size_t)1 << n), g((size_t)1 << n);
        for (auto& x : f) x = random_element(rng);
        for (auto& x : g) x = random_element(rng);
        std::vector<Point> points(2, Point(n));
        for (Point& p : points)
            for (FieldElement& x : p) x = random_element(rng);

        const std::vector<std::unique_ptr<Context>> ranks = Context::create_set(std::vector<int>((size_t)G, 0));
        std::vector<RankResult> got((size_t)G);
        std::vector<std::thread> threads;
        for (int r = 0; r < G; r++)
            threads.emplace_back([&, r] {  // the same calls with the same inputs in the same order on every rank
                try {
                    const Context& ctx = *ranks[(size_t)r];
                    WhirPcs pcs(ctx, cfg);
                    DeviceVec d_f(ctx, f), d_g(ctx, g);
                    const PcsCommitment com = pcs.commit({&d_f, &d_g});
                    got[(size_t)r].root = com.root();
                    got[(size_t)r].opening = pcs.open(com, points);
                } catch (const Error& e) {
                    got[(size_t)r].error = e.what();
                }
            });
        for (std::thread& t : threads) t.join();
        for (int r = 0; r < G; r++) {
            const RankResult& x = got[(size_t)r];
            if (!x.error.empty()) throw Error(-200, "rank " + std::to_string(r) + ": " + x.error);
            if (x.root != got[0].root) throw Error(-201, "rank " + std::to_string(r) + " committed to another root than rank 0");
            if (x.opening.proof != got[0].opening.proof || x.opening.evaluations != got[0].opening.evaluations)
                throw Error(-202, "rank " + std::to_string(r) + " wrote another proof than rank 0");
        }
        std::vector<FieldElement> bound;
        const PcsVerdict ok = WhirPcs::verify(cfg, points, got[0].opening.proof, &got[0].root, &bound);
        if (!ok) throw Error(-203, "the set's opening was rejected: " + ok.message);
        if (bound != got[0].opening.evaluations) throw Error(-204, "the verifier read other evaluations than the ranks returned");
        std::printf("ok n_vars=%u ranks=%d points=%zu proof_bytes=%zu: one root, one proof, accepted\n", n, G, points.size(), got[0].opening.proof.size());
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
