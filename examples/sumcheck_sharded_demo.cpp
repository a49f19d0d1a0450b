// sumcheck_sharded_demo.cpp -- a relation over committed tables on a device set, no Python in the loop: G ranks (here all on device 0,
// so the library joins them by its in-process transport; distinct devices get RCCL), one host thread per rank.  Every rank commits to
// a, b and c = a * b with the set's sharded WHIR scheme (provekit::WhirPcs), proves sum_x eq(tau, x) (a b - c)(x) = 0 with the root
// bound, sharded over the ranks (provekit::ShardedProductSumcheck, include/provekit_sumcheck_sharded.hpp), and opens the commitment at
// the sumcheck's point, sharded again.  Every rank must report the same root, the same sumcheck proof and the same opening; one host
// verification of each follows, and the opening's evaluations must be the sumcheck's final values.
//
//   sumcheck_sharded_demo <n_vars> <ranks> <seed>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "provekit_sumcheck_sharded.hpp"
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
    std::vector<FieldElement> bind;
    SumcheckProof sumcheck;
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
        const size_t N = (size_t)1 << n;
        std::vector<FieldElement> a(N), b(N), tau(n);
        for (auto& x : a) x = random_element(rng);
        for (auto& x : b) x = random_element(rng);
        for (auto& x : tau) x = random_element(rng);
        const WhirConfig cfg = WhirConfig::for_size(n, 8.0, 3);
        const FieldElement zero{0, 0, 0, 0};

        const std::vector<std::unique_ptr<Context>> ranks = Context::create_set(std::vector<int>((size_t)G, 0));
        // 1 and -1 as field elements (Montgomery), from the library's own conversion
        FieldElement one, minus_one;
        {
            const Context& ctx = *ranks[0];
            DeviceVec d_small(ctx, std::vector<FieldElement>{{1, 0, 0, 0}, zero});
            ctx.check(pk_fe_to_mont(ctx.get(), d_small.data(), d_small.data(), 1));
            ctx.check(pk_fe_sub(ctx.get(), d_small.data() + 4, d_small.data(), d_small.data() + 4, 1));
            const std::vector<FieldElement> units = d_small.to_host();
            one = units[0], minus_one = units[1];
        }
        SumcheckStatement st(n, 3, true, 1);
        st.add_term(one, {0, 1}).add_term(minus_one, {2});
        const struct pkss_plan plan = sharded_sumcheck_plan(st, (unsigned)G);

        std::vector<RankResult> got((size_t)G);
        std::vector<std::thread> threads;
        for (int r = 0; r < G; r++)
            threads.emplace_back([&, r] {  // the same calls with the same inputs in the same order on every rank
                RankResult& mine = got[(size_t)r];
                try {
                    const Context& ctx = *ranks[(size_t)r];
                    DeviceVec d_a(ctx, a), d_b(ctx, b), d_c(ctx, N);
                    ctx.check(pk_fe_mul(ctx.get(), d_a.data(), d_b.data(), d_c.data(), N));
                    WhirPcs pcs(ctx, cfg);
                    const PcsCommitment com = pcs.commit({&d_a, &d_b, &d_c});
                    mine.root = com.root();
                    // the root, a canonical digest, as the field element the sumcheck's transcript absorbs first
                    FieldElement root_canonical;
                    std::memcpy(root_canonical.data(), mine.root.data(), 32);
                    DeviceVec d_root(ctx, std::vector<FieldElement>{root_canonical});
                    ctx.check(pk_fe_to_mont(ctx.get(), d_root.data(), d_root.data(), 1));
                    mine.bind = d_root.to_host();
                    ShardedProductSumcheck prover(ctx, st);
                    mine.sumcheck = prover.prove({&d_a, &d_b, &d_c}, tau, mine.bind);
                    mine.opening = pcs.open(com, {mine.sumcheck.point});
                } catch (const Error& e) {
                    mine.error = e.what();
                }
            });
        for (std::thread& t : threads) t.join();
        for (int r = 0; r < G; r++) {
            const RankResult& x = got[(size_t)r];
            if (!x.error.empty()) throw Error(-200, "rank " + std::to_string(r) + ": " + x.error);
            if (x.root != got[0].root) throw Error(-201, "rank " + std::to_string(r) + " committed to another root than rank 0");
            if (x.sumcheck.proof != got[0].sumcheck.proof || x.sumcheck.point != got[0].sumcheck.point || x.sumcheck.finals != got[0].sumcheck.finals)
                throw Error(-202, "rank " + std::to_string(r) + " wrote another sumcheck proof than rank 0");
            if (x.opening.proof != got[0].opening.proof || x.opening.evaluations != got[0].opening.evaluations)
                throw Error(-203, "rank " + std::to_string(r) + " wrote another opening than rank 0");
        }
        const RankResult& x = got[0];
        const SumcheckVerdict ok = ProductSumcheck::verify(st, x.sumcheck.proof, tau, x.bind, &zero);
        if (!ok) throw Error(-204, "the set's sumcheck was rejected: " + ok.message);
        if (ok.point != x.sumcheck.point || ok.finals != x.sumcheck.finals) throw Error(-205, "the verifier read another point or other final values than the ranks returned");
        const std::vector<Point> points{ok.point};
        std::vector<FieldElement> bound;
        const PcsVerdict pcs_ok = WhirPcs::verify(cfg, points, x.opening.proof, &x.root, &bound);
        if (!pcs_ok) throw Error(-206, "the set's opening was rejected: " + pcs_ok.message);
        if (bound != ok.finals) throw Error(-207, "the committed tables do not take the sumcheck's final values at its point");
        std::printf("ok n_vars=%u ranks=%d sharded_rounds=%u arena_bytes=%zu sumcheck_bytes=%zu opening_bytes=%zu: one root, one sumcheck, one opening, accepted\n", n, G,
                    plan.S, plan.arena_bytes, x.sumcheck.proof.size(), x.opening.proof.size());
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
