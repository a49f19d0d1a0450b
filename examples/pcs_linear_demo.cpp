// pcs_linear_demo.cpp -- a LINEAR statement over a WHIR commitment, no Python in the loop: commit to two multilinear polynomials,
// open them at one point and at two dense weight tables (<w_i, poly_b> = s_{b,i}), verify on the host once with the tables given
// and once without -- closing the condition "deferred[i] is the extension of w_i at the folding point" with pkw_evaluate -- then
// change one sum in the proof and see the rejection (provekit::WhirPcs, include/provekit_whir.hpp).
//
//   pcs_linear_demo <n_vars> <seed>
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
        std::vector<FieldElement> f(N), g(N), w0(N), w1(N);
        for (auto* v : {&f, &g, &w0, &w1})
            for (auto& x : *v) x = random_element(rng);
        DeviceVec d_f(ctx, f), d_g(ctx, g), d_w0(ctx, w0), d_w1(ctx, w1);
        const PcsCommitment com = pcs.commit({&d_f, &d_g});
        const std::array<uint8_t, 32> root = com.root();

        const std::vector<Point> points(1, [&] {
            Point p(n);
            for (FieldElement& x : p) x = random_element(rng);
            return p;
        }());
        // the tags bind the weights under Fiat-Shamir: here two labels the two sides agreed on beforehand
        const std::vector<FieldElement> tags = {random_element(rng), random_element(rng)};
        const PcsLinearOpening opening = pcs.open_linear(com, points, {&d_w0, &d_w1}, tags);

        const PcsLinearVerdict full = WhirPcs::verify_linear(cfg, points, tags, {&w0, &w1}, opening.proof, &root);
        if (!full) throw Error(-200, "a valid opening was rejected: " + full.verdict.message);
        if (full.unchecked != 0 || full.sums != opening.sums || full.evaluations != opening.evaluations)
            throw Error(-201, "the verifier read another statement than the prover returned");

        // without the tables the verdict is conditional; a dense table's side of the condition is one pkw_evaluate
        const PcsLinearVerdict cond = WhirPcs::verify_linear(cfg, points, tags, {}, opening.proof, &root);
        if (!cond || cond.unchecked != 2) throw Error(-202, "the conditional verdict is not what it should be");
        std::vector<uint64_t> fold;
        for (const FieldElement& x : cond.fold_point) fold.insert(fold.end(), x.begin(), x.end());
        const DeviceVec* tables[2] = {&d_w0, &d_w1};
        for (int i = 0; i < 2; i++) {
            const uint64_t* d = tables[i]->data();
            FieldElement at;
            ctx.check(pkw_evaluate(ctx.get(), &d, 1, n, fold.data(), 1, at.data()));
            if (at != cond.deferred[i]) throw Error(-203, "a deferred value is not the weight's extension at the folding point");
        }

        // the sums sit behind the root, the OOD answers, the point, the tags and the evaluations
        const size_t first_sum = 32 + 32 * (size_t)cfg.to_c().commitment_ood_samples * 2 + 32 * (size_t)n + 32 * 2 + 32 * 2;
        std::vector<uint8_t> bad = opening.proof;
        bad[first_sum] ^= 1;
        const PcsLinearVerdict no = WhirPcs::verify_linear(cfg, points, tags, {&w0, &w1}, bad, &root);
        if (no) throw Error(-204, "an opening with a changed sum was accepted");
        std::printf("ok n_vars=%u points=%zu weights=%zu proof_bytes=%zu\n", n, points.size(), tags.size(), opening.proof.size());
        std::printf("tables withheld: accepted with unchecked=%u, condition closed with pkw_evaluate at the folding point\n", cond.unchecked);
        std::printf("changed sum at byte %zu: rejected, check=%s at offset %llu (%s)\n", first_sum, no.verdict.check_name(),
                    (unsigned long long)no.verdict.offset, no.verdict.message.c_str());
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
