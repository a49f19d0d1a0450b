// gate_pcs_demo.cpp -- a vanilla Plonk gate over committed columns, end to end, no Python in the loop: commit to the selectors qL, qR,
// qM, qO and to qC, a, b, c as two WHIR batches of four (provekit::WhirPcs), prove
//     sum_x eq(tau, x) (qL a + qR b + qM a b + qO c + qC)(x) = 0
// with both roots bound into the transcript (provekit::WideSumcheck, include/provekit_sumcheck_wide.hpp: 8 tables and 5 terms, more
// than provekit::ProductSumcheck states), open all eight columns at the sumcheck's point, verify both on the host and see that the
// openings' evaluations are the sumcheck's final values -- the condition under which "accepted" holds.  Then the error paths.
//
//   gate_pcs_demo <n_vars> <seed>
#include <cstdio>
#include <cstdlib>

#include "provekit_sumcheck_wide.hpp"
#include "provekit_whir.hpp"

using namespace provekit;

static uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
static FieldElement random_element(uint64_t& s) { return {splitmix(s), splitmix(s), splitmix(s), splitmix(s) >> 6}; }  // < 2^250 < p

// a commitment's root, a canonical digest, as the field element the sumcheck's transcript absorbs
static FieldElement root_element(const Context& ctx, const std::array<uint8_t, 32>& root) {
    FieldElement canonical;
    std::memcpy(canonical.data(), root.data(), 32);
    DeviceVec d(ctx, std::vector<FieldElement>{canonical});
    ctx.check(pk_fe_to_mont(ctx.get(), d.data(), d.data(), 1));
    return d.to_host()[0];
}

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
        auto random_column = [&] {
            std::vector<FieldElement> v(N);
            for (auto& x : v) x = random_element(rng);
            return DeviceVec(ctx, v);
        };
        // seven free columns; qC closes the gate in every row: qC = -(qL a + qR b + qM a b + qO c)
        DeviceVec qL = random_column(), qR = random_column(), qM = random_column(), qO = random_column(), a = random_column(), b = random_column(), c = random_column();
        DeviceVec qC(ctx, N), t(ctx, N);
        pk_ctx* h = ctx.get();
        ctx.check(pk_fe_mul(h, qL.data(), a.data(), qC.data(), N));
        ctx.check(pk_fe_mul(h, qR.data(), b.data(), t.data(), N));
        ctx.check(pk_fe_add(h, qC.data(), t.data(), qC.data(), N));
        ctx.check(pk_fe_mul(h, qM.data(), a.data(), t.data(), N));
        ctx.check(pk_fe_mul(h, t.data(), b.data(), t.data(), N));
        ctx.check(pk_fe_add(h, qC.data(), t.data(), qC.data(), N));
        ctx.check(pk_fe_mul(h, qO.data(), c.data(), t.data(), N));
        ctx.check(pk_fe_add(h, qC.data(), t.data(), qC.data(), N));
        ctx.check(pk_fe_sub(h, t.data(), t.data(), t.data(), N));  // 0
        ctx.check(pk_fe_sub(h, t.data(), qC.data(), qC.data(), N));

        // 1 and 0 as field elements (Montgomery), from the library's own conversion
        const FieldElement zero{0, 0, 0, 0};
        DeviceVec d_one(ctx, std::vector<FieldElement>{{1, 0, 0, 0}});
        ctx.check(pk_fe_to_mont(h, d_one.data(), d_one.data(), 1));
        const FieldElement one = d_one.to_host()[0];

        const WhirConfig cfg = WhirConfig::for_size(n, 8.0, 4);
        WhirPcs pcs(ctx, cfg);
        const PcsCommitment selectors = pcs.commit({&qL, &qR, &qM, &qO});
        const PcsCommitment wires = pcs.commit({&qC, &a, &b, &c});
        const std::array<uint8_t, 32> root_s = selectors.root(), root_w = wires.root();
        const std::vector<FieldElement> bind{root_element(ctx, root_s), root_element(ctx, root_w)};

        // tables 0 .. 7: qL qR qM qO qC a b c
        WideSumcheckStatement st(n, 8, true, 2);
        st.add_term(one, {0, 5}).add_term(one, {1, 6}).add_term(one, {2, 5, 6}).add_term(one, {3, 7}).add_term(one, {4});
        std::vector<FieldElement> tau(n);
        for (auto& x : tau) x = random_element(rng);
        WideSumcheck prover(ctx, st);
        const SumcheckProof proof = prover.prove({&qL, &qR, &qM, &qO, &qC, &a, &b, &c}, tau, bind);

        const SumcheckVerdict ok = WideSumcheck::verify(st, proof.proof, tau, bind, &zero);
        if (!ok) throw Error(-200, "a valid gate sumcheck was rejected: " + ok.message);
        if (ok.point != proof.point || ok.finals != proof.finals) throw Error(-201, "the verifier read another point or other final values than the prover returned");

        // accepted PROVIDED the eight columns take the final values at the point: the two openings prove that
        const std::vector<Point> points{ok.point};
        const PcsOpening open_s = pcs.open(selectors, points), open_w = pcs.open(wires, points);
        std::vector<FieldElement> bound_s, bound_w;
        const PcsVerdict ok_s = WhirPcs::verify(cfg, points, open_s.proof, &root_s, &bound_s);
        const PcsVerdict ok_w = WhirPcs::verify(cfg, points, open_w.proof, &root_w, &bound_w);
        if (!ok_s || !ok_w) throw Error(-202, "a valid opening was rejected: " + (ok_s ? ok_w.message : ok_s.message));
        bound_s.insert(bound_s.end(), bound_w.begin(), bound_w.end());
        if (bound_s != ok.finals) throw Error(-203, "the committed columns do not take the sumcheck's final values at its point");
        std::printf("ok n_vars=%u sumcheck_bytes=%zu opening_bytes=%zu+%zu arena_bytes=%zu\n", n, proof.proof.size(), open_s.proof.size(), open_w.proof.size(),
                    st.arena_bytes());

        // the error paths: a changed round value, another root, a gate that does not hold, a statement that is none
        std::vector<uint8_t> bad = proof.proof;
        bad[32 * 5] ^= 1;  // h_1(0): s and round 0's four values come before it
        const SumcheckVerdict no = WideSumcheck::verify(st, bad, tau, bind, &zero);
        if (no || no.check != PKS_CHECK_ROUND) throw Error(-204, "a changed round value was not rejected at its round");
        std::printf("changed round value: rejected, check=%s at offset %llu (%s)\n", no.check_name(), (unsigned long long)no.offset, no.message.c_str());
        const SumcheckVerdict other_root = WideSumcheck::verify(st, proof.proof, tau, {bind[1], bind[0]}, &zero);
        if (other_root) throw Error(-205, "the proof was accepted under other roots");
        std::printf("the roots exchanged: rejected, check=%s\n", other_root.check_name());
        const SumcheckProof false_gate = prover.prove({&qL, &qR, &qM, &qO, &a, &a, &b, &c}, tau, bind);  // qC replaced: the gate does not hold
        const SumcheckVerdict not_zero = WideSumcheck::verify(st, false_gate.proof, tau, bind, &zero);
        if (not_zero || not_zero.check != PKS_CHECK_SUM) throw Error(-206, "a gate that does not hold was accepted with sum 0");
        std::printf("a gate that does not hold: rejected, check=%s\n", not_zero.check_name());
        try {
            WideSumcheckStatement none(n, 8, true, 2);
            none.add_term(one, {5, 0});
            none.proof_bytes();
            throw Error(-207, "a term whose list is not non-decreasing was taken");
        } catch (const Error& e) {
            if (e.code != PK_ERR_BAD_ARG) throw;
            std::printf("the term {5, 0}: refused (%s)\n", e.what());
        }
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
