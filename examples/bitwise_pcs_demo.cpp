// bitwise_pcs_demo.cpp -- a 32-bit XOR over committed columns, end to end, no Python in the loop: columns a and b of 2^n values below
// 2^32, c = a XOR b formed on the device and all three split into four digits of 8 bits with the multiplicities of their rows in the XOR
// table of 2^16 rows (provekit::Bitwise, include/provekit_bitwise.hpp).  Commit {a, b, c}, the three digit batches and m with WHIR
// (provekit::WhirPcs), before any challenge exists; prove the operation with the five roots bound; verify it on the host; open the four
// batches at z_lo and m at z_T and check the five claims on the values the openings bind (Bitwise::check_claims).  Then the refusals: an
// operand of 2^32, a given c that is off in one bit, and digit columns with one row that is not a row of the XOR table.
//
//   bitwise_pcs_demo [n = 10] [seed = 7]
#include <cstdio>
#include <cstdlib>

#include "provekit_bitwise.hpp"
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
    const unsigned n = argc > 1 ? std::atoi(argv[1]) : 10, d = 8, L = 4;
    uint64_t rng = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 7;
    try {
        Context ctx(0);
        const size_t N = (size_t)1 << n, K = (size_t)1 << (2 * d);
        std::vector<FieldElement> a(N), b(N);
        for (size_t x = 0; x < N; x++) a[x] = {splitmix(rng) >> 32, 0, 0, 0}, b[x] = {splitmix(rng) >> 32, 0, 0, 0};
        a[0] = {0, 0, 0, 0}, b[0] = {0xffffffffull, 0, 0, 0}, a[1] = b[1] = {0xffffffffull, 0, 0, 0};
        const DeviceVec d_a = montgomery(ctx, a), d_b = montgomery(ctx, b);

        Bitwise prover(ctx, n, PKB_XOR, d, L, 5);
        DeviceVec d_c(ctx, N), d_m(ctx, K);
        std::vector<DeviceVec> digits;
        for (unsigned i = 0; i < 3 * L; i++) digits.emplace_back(ctx, N);
        std::vector<DeviceVec*> digits_out;
        std::vector<const DeviceVec*> digit_cols;
        for (DeviceVec& v : digits) digits_out.push_back(&v), digit_cols.push_back(&v);
        prover.decompose(d_a, d_b, d_c, false, digits_out, d_m);

        // the one commitment phase: {a, b, c}, the digits of each column as a batch, m by itself, before the seed exists
        const WhirConfig cfg_abc = WhirConfig::for_size(n, 8.0, 3), cfg_dig = WhirConfig::for_size(n, 8.0, L), cfg_m = WhirConfig::for_size(2 * d, 8.0, 1);
        WhirPcs pcs_abc(ctx, cfg_abc), pcs_dig(ctx, cfg_dig), pcs_m(ctx, cfg_m);
        const PcsCommitment com_abc = pcs_abc.commit({&d_a, &d_b, &d_c});
        std::vector<PcsCommitment> com_dig;
        for (unsigned j = 0; j < 3; j++) com_dig.push_back(pcs_dig.commit({&digits[j * L], &digits[j * L + 1], &digits[j * L + 2], &digits[j * L + 3]}));
        const PcsCommitment com_m = pcs_m.commit({&d_m});
        std::vector<FieldElement> bind{as_element(ctx, com_abc.root())};
        for (const PcsCommitment& com : com_dig) bind.push_back(as_element(ctx, com.root()));
        bind.push_back(as_element(ctx, com_m.root()));
        const BitwiseProof proof = prover.prove(digit_cols, d_m, bind);

        const BitwiseVerdict ok = Bitwise::verify(prover.statement(), proof.proof, bind);
        if (!ok) throw Error(-200, "a valid bitwise proof was rejected: " + ok.message);
        const BitwiseClaims& cl = ok.claims;
        if (cl.z_lo != proof.claims.z_lo || cl.z_t != proof.claims.z_t || cl.digits_value != proof.claims.digits_value || cl.m_value != proof.claims.m_value)
            throw Error(-201, "the verifier derived other claims than the prover returned");
        std::printf("accepted n=%u op=xor d=%u L=%u proof_bytes=%zu\n", n, d, L, proof.proof.size());

        // accepted PROVIDED the five claims hold: the commitment scheme gives the evaluations, with one opening per commitment
        size_t opening_bytes = 0;
        auto opened = [&](const WhirPcs& pcs, const WhirConfig& cfg, const PcsCommitment& com, const Point& point, const char* what) {
            const PcsOpening opening = pcs.open(com, {point});
            const std::array<uint8_t, 32> root = com.root();
            std::vector<FieldElement> bound;
            const PcsVerdict v = WhirPcs::verify(cfg, {point}, opening.proof, &root, &bound);
            if (!v) throw Error(-202, std::string("a valid opening of ") + what + " was rejected: " + v.message);
            opening_bytes += opening.proof.size();
            return bound;
        };
        const std::vector<FieldElement> abc = opened(pcs_abc, cfg_abc, com_abc, cl.z_lo, "a, b and c");
        std::vector<FieldElement> digit_evals;
        for (unsigned j = 0; j < 3; j++) {
            const std::vector<FieldElement> part = opened(pcs_dig, cfg_dig, com_dig[j], cl.z_lo, "a digit batch");
            digit_evals.insert(digit_evals.end(), part.begin(), part.end());
        }
        const std::vector<FieldElement> m_eval = opened(pcs_m, cfg_m, com_m, cl.z_t, "m");
        const int which = Bitwise::check_claims(prover.statement(), cl, abc, digit_evals, m_eval[0]);
        if (which != PKB_CLAIM_NONE) throw Error(-203, "the committed columns do not take the claimed values: claim " + std::to_string(which));
        std::vector<FieldElement> other = abc;
        other[2][0] ^= 1;  // c's evaluation changed: its recomposition fails
        if (Bitwise::check_claims(prover.statement(), cl, other, digit_evals, m_eval[0]) != PKB_CLAIM_RECOMPOSE_C) throw Error(-204, "a changed evaluation passed the claims");
        std::printf("claims hold: opening_bytes=%zu commitments=5 phases=1 openings=5\n", opening_bytes);

        std::vector<DeviceVec> scratch;
        for (unsigned i = 0; i < 3 * L; i++) scratch.emplace_back(ctx, N);
        std::vector<DeviceVec*> scratch_out;
        for (DeviceVec& v : scratch) scratch_out.push_back(&v);
        DeviceVec m_scratch(ctx, K), c_scratch(ctx, N);
        // an operand of 2^32: the decomposition refuses it and names the entry and the operand
        {
            std::vector<FieldElement> bad = b;
            bad[7] = {1ull << 32, 0, 0, 0};
            const DeviceVec d_bad = montgomery(ctx, bad);
            uint64_t first_bad = 0;
            try {
                prover.decompose(d_a, d_bad, c_scratch, false, scratch_out, m_scratch, &first_bad);
                throw Error(-205, "an operand of 2^32 was taken");
            } catch (const Error& e) {
                if (e.code != PK_ERR_UNSATISFIED || first_bad != 7) throw;
                std::printf("an operand of 2^32: refused rc=%d (%s)\n", e.code, e.what());
            }
        }
        // a given c that is off in one bit at entry 9
        {
            std::vector<FieldElement> c_host(N);
            for (size_t x = 0; x < N; x++) c_host[x] = {a[x][0] ^ b[x][0], 0, 0, 0};
            c_host[9][0] ^= 1ull << 17;
            DeviceVec d_wrong = montgomery(ctx, c_host);
            uint64_t first_bad = 0;
            try {
                prover.decompose(d_a, d_b, d_wrong, true, scratch_out, m_scratch, &first_bad);
                throw Error(-206, "a wrong c was taken");
            } catch (const Error& e) {
                if (e.code != PK_ERR_UNSATISFIED || first_bad != 9) throw;
                std::printf("a given c off in one bit: refused rc=%d (%s)\n", e.code, e.what());
            }
        }
        // digit 2 of c changed at entry 5: the row (a_2, b_2, c_2) is not a row of the XOR table
        {
            std::vector<FieldElement> col = digits[2 * L + 2].to_host();
            const uint64_t c2 = ((a[5][0] ^ b[5][0]) >> (2 * d)) & 0xff;
            col[5] = montgomery(ctx, {FieldElement{c2 ^ 1, 0, 0, 0}}).to_host()[0];
            const DeviceVec d_col(ctx, col);
            std::vector<const DeviceVec*> changed = digit_cols;
            changed[2 * L + 2] = &d_col;
            try {
                prover.prove(changed, d_m, bind);
                throw Error(-207, "a digit row outside the table was taken");
            } catch (const Error& e) {
                if (e.code != PK_ERR_UNSATISFIED) throw;
                std::printf("a row outside the table: refused rc=%d (%s)\n", e.code, e.what());
            }
            if (prover.prove(digit_cols, d_m, bind).proof != proof.proof) throw Error(-208, "the prover did not stay usable");
        }
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
