// pcs_sparse_demo.cpp -- a linear statement with SPARSE weights over a WHIR commitment, no Python in the loop: commit to two
// multilinear polynomials, open them at one point and at three weights given as index/value lists -- a single position, a strided
// selector and the zero weight --, verify on the host, where every deferred value is judged from the entries (no dense table, no
// conditional verdict), then change one entry on the verifier's side and see the rejection (provekit::WhirPcs, provekit_whir.hpp).
//
//   pcs_sparse_demo <n_vars> <seed>
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
        const size_t N = (size_t)1 << n;
        std::vector<FieldElement> f(N), g(N);
        for (auto* v : {&f, &g})
            for (auto& x : *v) x = random_element(rng);
        DeviceVec d_f(ctx, f), d_g(ctx, g);
        const PcsCommitment com = pcs.commit({&d_f, &d_g});
        const std::array<uint8_t, 32> root = com.root();

        PcsSparseWeights weights;
        weights.add({(uint32_t)(N / 3)}, {random_element(rng)});  // one position of the table
        std::vector<uint32_t> every16;
        std::vector<FieldElement> ones;
        for (uint32_t x = 5; x < N; x += 16) {  // a selector: the same value at every 16th position
            every16.push_back(x);
            ones.push_back(ones.empty() ? random_element(rng) : ones[0]);
        }
        weights.add(every16, ones);
        weights.add({}, {});  // the zero weight: its sums are zero
        const std::vector<Point> points(1, [&] {
            Point p(n);
            for (FieldElement& x : p) x = random_element(rng);
            return p;
        }());
        const std::vector<FieldElement> tags = {random_element(rng), random_element(rng), random_element(rng)};
        const PcsLinearOpening opening = pcs.open_sparse(ctx, com, points, weights, tags);
        for (unsigned b = 0; b < 2; b++)
            if (opening.sums[b * 3 + 2] != FieldElement{0, 0, 0, 0}) throw Error(-205, "the zero weight has a non-zero sum");

        const PcsLinearVerdict ok = WhirPcs::verify_sparse(cfg, points, tags, weights, opening.proof, &root);
        if (!ok) throw Error(-200, "a valid opening was rejected: " + ok.verdict.message);
        if (ok.unchecked != 0 || ok.sums != opening.sums || ok.evaluations != opening.evaluations)
            throw Error(-201, "the verifier read another statement than the prover returned");

        PcsSparseWeights other = weights;  // the selector moved by one position: a well-formed list of another weight
        other.index[1 + every16.size() / 2] += 1;
        const PcsLinearVerdict no = WhirPcs::verify_sparse(cfg, points, tags, other, opening.proof, &root);
        if (no) throw Error(-204, "an opening was accepted for a weight it was not made for");
        std::printf("ok n_vars=%u points=%zu weights=%u entries=%zu proof_bytes=%zu\n", n, points.size(), weights.count(), weights.index.size(),
                    opening.proof.size());
        std::printf("one index changed on the verifier's side: rejected, check=%s at offset %llu (%s)\n", no.verdict.check_name(),
                    (unsigned long long)no.verdict.offset, no.verdict.message.c_str());
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
