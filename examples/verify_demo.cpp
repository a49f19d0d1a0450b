// verify_demo.cpp -- prove, verify, flip a byte, see the rejection: provekit::Verifier (include/provekit_verify.hpp) next to the
// prover types of provekit_hip.hpp, no Python in the loop.
//
//   verify_demo <m> <m_0> <num_constraints> <num_inputs> <seed>
//
// The instance is prove_demo's: row i says (sum a z)(sum b z) = z[1 + num_inputs + i].  Four proofs are verified by the host core
// and, in one call, by the device path; then one byte of a proof is flipped and both paths must name the same failed check.
#include <cstdio>
#include <cstdlib>

#include "provekit_verify.hpp"

using namespace provekit;

static uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s m m_0 num_constraints num_inputs seed\n", argv[0]);
        return 2;
    }
    const unsigned m = std::atoi(argv[1]), m_0 = std::atoi(argv[2]);
    const size_t nc = std::strtoull(argv[3], nullptr, 10), n_in = std::strtoull(argv[4], nullptr, 10);
    uint64_t rng = std::strtoull(argv[5], nullptr, 10);
    const size_t nw = 1 + n_in + nc;
    try {
        Context ctx(0);
        const uint64_t small[8] = {1, 2, 3, 5, 7, 11, 13, 17};
        std::vector<FieldElement> canon(8, FieldElement{0, 0, 0, 0});
        for (int i = 0; i < 8; i++) canon[i][0] = small[i];
        DeviceVec d_canon(ctx, canon), d_int(ctx, 8);
        ctx.check(pk_fe_to_mont(ctx.get(), d_canon.data(), d_int.data(), 8));
        const std::vector<FieldElement> interner = d_int.to_host();
        SparseMatrix A, B, Cm;
        for (SparseMatrix* M : {&A, &B}) {
            M->num_rows = nc;
            M->num_cols = nw;
            for (size_t i = 0; i < nc; i++) {
                M->new_row_indices.push_back((uint32_t)M->col_indices.size());
                const uint32_t c0 = (uint32_t)(splitmix(rng) % (1 + n_in - 2));
                for (uint32_t k = 0; k < 3; k++) {
                    M->col_indices.push_back(c0 + k);
                    M->values.push_back((uint32_t)(splitmix(rng) % 8));
                }
            }
        }
        Cm.num_rows = nc;
        Cm.num_cols = nw;
        for (size_t i = 0; i < nc; i++) {
            Cm.new_row_indices.push_back((uint32_t)i);
            Cm.col_indices.push_back((uint32_t)(1 + n_in + i));
            Cm.values.push_back(0);
        }
        R1CS r1cs(ctx, A, B, Cm, interner);
        std::vector<FieldElement> z(nw, FieldElement{0, 0, 0, 0});
        z[0] = interner[0];
        for (size_t i = 1; i <= n_in; i++) z[i] = {splitmix(rng), splitmix(rng), splitmix(rng), splitmix(rng) >> 6};
        DeviceVec d_z(ctx, z), d_az(ctx, nc), d_bz(ctx, nc);
        ctx.check(pk_r1cs_matvec(ctx.get(), r1cs.get(), 0, 0, d_z.data(), d_az.data()));
        ctx.check(pk_r1cs_matvec(ctx.get(), r1cs.get(), 1, 0, d_z.data(), d_bz.data()));
        ctx.check(pk_fe_mul(ctx.get(), d_az.data(), d_bz.data(), d_z.data() + 4 * (1 + n_in), nc));
        r1cs.test_witness_satisfaction(d_z);

        WhirR1CSScheme scheme(ctx, r1cs, m, m_0, WhirConfig::for_size(m, 8.0), WhirConfig::for_hiding_spartan(m_0, 8.0));
        std::vector<WhirR1CSProof> proofs;
        for (int i = 0; i < 4; i++) proofs.push_back(scheme.prove(d_z));  // production randomness: four different transcripts

        Verifier verifier(scheme);
        verifier.set_r1cs(A, B, Cm, interner);
        verifier.attach(ctx);
        std::vector<const std::vector<uint8_t>*> batch;
        for (const auto& p : proofs) batch.push_back(&p.transcript);
        const std::vector<Verdict> many = verifier.verify_many(batch);
        for (size_t i = 0; i < proofs.size(); i++) {
            const Verdict host = verifier.verify(proofs[i].transcript);
            if (!host || !many[i]) throw Error(-200, "a valid proof was rejected: " + (host ? many[i].message : host.message));
        }
        std::vector<uint8_t> bad = proofs[0].transcript;
        bad[bad.size() / 2] ^= 1;
        const Verdict host = verifier.verify(bad);
        batch[0] = &bad;
        const std::vector<Verdict> again = verifier.verify_many(batch);
        if (host || again[0]) throw Error(-201, "a proof with a flipped byte was accepted");
        if (host.check != again[0].check || host.offset != again[0].offset) throw Error(-202, "host core and device path disagree on the failed check");
        for (size_t i = 1; i < again.size(); i++)
            if (!again[i]) throw Error(-203, "a tampered batch mate disturbed a valid proof");
        std::printf("ok verified=%zu proof_bytes=%zu\n", proofs.size(), proofs[0].transcript.size());
        std::printf("flipped byte %zu: rejected, check=%s at offset %llu (%s)\n", bad.size() / 2, host.check_name(), (unsigned long long)host.offset,
                    host.message.c_str());
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
