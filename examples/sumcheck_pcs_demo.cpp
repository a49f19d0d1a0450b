// sumcheck_pcs_demo.cpp -- a relation over committed tables, end to end, no Python in the loop: commit to a, b and c = a * b with WHIR
// (provekit::WhirPcs), prove sum_x eq(tau, x) (a b - c)(x) = 0 with the commitment's root bound into the transcript
// (provekit::ProductSumcheck, include/provekit_sumcheck.hpp), open the commitment at the sumcheck's point, verify both on the host and
// see that the opening's evaluations are the sumcheck's final values -- the condition under which "accepted" holds.  Then the error paths.
//
//   sumcheck_pcs_demo <n_vars> <seed>
#include <cstdio>
#include <cstdlib>

#include "provekit_sumcheck.hpp"
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
        const size_t N = (size_t)1 << n;
        std::vector<FieldElement> a(N), b(N);
        for (auto& x : a) x = random_element(rng);
        for (auto& x : b) x = random_element(rng);
        DeviceVec d_a(ctx, a), d_b(ctx, b), d_c(ctx, N);
        ctx.check(pk_fe_mul(ctx.get(), d_a.data(), d_b.data(), d_c.data(), N));

        // 1, -1 and 0 as field elements (Montgomery), from the library's own conversion
        const FieldElement zero{0, 0, 0, 0};
        DeviceVec d_small(ctx, std::vector<FieldElement>{{1, 0, 0, 0}, zero});
        ctx.check(pk_fe_to_mont(ctx.get(), d_small.data(), d_small.data(), 1));
        ctx.check(pk_fe_sub(ctx.get(), d_small.data() + 4, d_small.data(), d_small.data() + 4, 1));
        const std::vector<FieldElement> units = d_small.to_host();
        const FieldElement one = units[0], minus_one = units[1];

        const WhirConfig cfg = WhirConfig::for_size(n, 8.0, 3);
        WhirPcs pcs(ctx, cfg);
        const PcsCommitment com = pcs.commit({&d_a, &d_b, &d_c});
        const std::array<uint8_t, 32> root = com.root();
        // the root, a canonical digest, as the field element the sumcheck's transcript absorbs first
        FieldElement root_canonical;
        std::memcpy(root_canonical.data(), root.data(), 32);
        DeviceVec d_root(ctx, std::vector<FieldElement>{root_canonical});
        ctx.check(pk_fe_to_mont(ctx.get(), d_root.data(), d_root.data(), 1));
        const std::vector<FieldElement> bind = d_root.to_host();

        SumcheckStatement st(n, 3, true, 1);
        st.add_term(one, {0, 1}).add_term(minus_one, {2});
        std::vector<FieldElement> tau(n);
        for (auto& x : tau) x = random_element(rng);
        ProductSumcheck prover(ctx, st);
        const SumcheckProof proof = prover.prove({&d_a, &d_b, &d_c}, tau, bind);

        const SumcheckVerdict ok = ProductSumcheck::verify(st, proof.proof, tau, bind, &zero);
        if (!ok) throw Error(-200, "a valid sumcheck was rejected: " + ok.message);
        if (ok.point != proof.point || ok.finals != proof.finals) throw Error(-201, "the verifier read another point or other final values than the prover returned");

        // accepted PROVIDED a, b, c take the final values at the point: the commitment scheme proves that
        const std::vector<Point> points{ok.point};
        const PcsOpening opening = pcs.open(com, points);
        std::vector<FieldElement> bound;
        const PcsVerdict pcs_ok = WhirPcs::verify(cfg, points, opening.proof, &root, &bound);
        if (!pcs_ok) throw Error(-202, "a valid opening was rejected: " + pcs_ok.message);
        if (bound != ok.finals) throw Error(-203, "the committed tables do not take the sumcheck's final values at its point");
        std::printf("ok n_vars=%u sumcheck_bytes=%zu opening_bytes=%zu\n", n, proof.proof.size(), opening.proof.size());

        // the error paths: a changed round value, another root, a sum that is not zero, a statement that is none
        std::vector<uint8_t> bad = proof.proof;
        bad[32 * 4] ^= 1;  // h_1(0): s and round 0's three values come before it
        const SumcheckVerdict no = ProductSumcheck::verify(st, bad, tau, bind, &zero);
        if (no || no.check != PKS_CHECK_ROUND) throw Error(-204, "a changed round value was not rejected at its round");
        std::printf("changed round value: rejected, check=%s at offset %llu (%s)\n", no.check_name(), (unsigned long long)no.offset, no.message.c_str());
        const SumcheckVerdict other_root = ProductSumcheck::verify(st, proof.proof, tau, {one}, &zero);
        if (other_root) throw Error(-205, "the proof was accepted under another root");
        std::printf("another root: rejected, check=%s\n", other_root.check_name());
        const SumcheckVerdict other_sum = ProductSumcheck::verify(st, proof.proof, tau, bind, &one);
        if (other_sum || other_sum.check != PKS_CHECK_SUM) throw Error(-206, "the proof was accepted for another sum");
        std::printf("another sum: rejected, check=%s\n", other_sum.check_name());
        try {
            SumcheckStatement none(n, 3, true, 1);
            none.add_term(one, {0, 3});
            none.proof_bytes();
            throw Error(-207, "a statement that names a table >= m was taken");
        } catch (const Error& e) {
            if (e.code != PK_ERR_BAD_ARG) throw;
            std::printf("a term over table 3 of 3: refused (%s)\n", e.what());
        }
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
