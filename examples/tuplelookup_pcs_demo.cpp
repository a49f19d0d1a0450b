// tuplelookup_pcs_demo.cpp -- a binop table over committed columns, end to end, no Python in the loop: the XOR table of 4-bit operands,
// 2^8 rows (a, b, a XOR b), and two groups of 2^n rows (a, b, a XOR b) that must all be rows of it.  Commit each group's three columns
// and {t0, t1, t2, m} with WHIR (provekit::WhirPcs), all before alpha and beta exist; count the multiplicities on the device; prove the
// lookup of both groups in ONE proof with the three roots bound (provekit::TupleLookup, include/provekit_tuplelookup.hpp); verify it on
// the host; open each group at z_lo and the table's columns at z_T -- three openings -- and check the three claims on the values the
// openings bind (TupleLookup::check_claims).  Then a row outside the table: refused, and why.
//
//   tuplelookup_pcs_demo [n = 10] [seed = 7]
#include <cstdio>
#include <cstdlib>

#include "provekit_tuplelookup.hpp"
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
    const unsigned n = argc > 1 ? std::atoi(argv[1]) : 10, k = 8, w = 3, c = 2;
    uint64_t rng = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 7;
    try {
        Context ctx(0);
        const size_t N = (size_t)1 << n, K = (size_t)1 << k;
        // row y = 16 a + b of the table is (a, b, a XOR b)
        std::vector<std::vector<FieldElement>> t(w, std::vector<FieldElement>(K));
        for (uint64_t y = 0; y < K; y++) t[0][y] = {y >> 4, 0, 0, 0}, t[1][y] = {y & 15, 0, 0, 0}, t[2][y] = {(y >> 4) ^ (y & 15), 0, 0, 0};
        std::vector<std::vector<std::vector<FieldElement>>> f(c, std::vector<std::vector<FieldElement>>(w, std::vector<FieldElement>(N)));
        std::vector<std::vector<uint32_t>> idx(c, std::vector<uint32_t>(N));
        for (unsigned g = 0; g < c; g++)
            for (size_t x = 0; x < N; x++) {
                const uint32_t y = idx[g][x] = (uint32_t)(splitmix(rng) % K);
                for (unsigned j = 0; j < w; j++) f[g][j][x] = t[j][y];
            }
        std::vector<DeviceVec> d_t, d_f, d_idx;
        for (unsigned j = 0; j < w; j++) d_t.push_back(montgomery(ctx, t[j]));
        for (unsigned g = 0; g < c; g++) {
            for (unsigned j = 0; j < w; j++) d_f.push_back(montgomery(ctx, f[g][j]));
            d_idx.push_back(TupleLookup::indices(ctx, idx[g]));
        }
        const TupleLookup::Columns table{&d_t[0], &d_t[1], &d_t[2]};
        const std::vector<TupleLookup::Columns> groups{{&d_f[0], &d_f[1], &d_f[2]}, {&d_f[3], &d_f[4], &d_f[5]}};

        TupleLookup prover(ctx, n, k, w, c, c + 1);
        DeviceVec d_m(ctx, K);
        prover.multiplicities(groups, table, {&d_idx[0], &d_idx[1]}, d_m);

        // the one commitment phase: each group's columns in a batch, the table's columns and m in another, before alpha and beta exist
        const WhirConfig cfg_n = WhirConfig::for_size(n, 8.0, w), cfg_k = WhirConfig::for_size(k, 8.0, w + 1);
        WhirPcs pcs_n(ctx, cfg_n), pcs_k(ctx, cfg_k);
        const PcsCommitment com_0 = pcs_n.commit(groups[0]), com_1 = pcs_n.commit(groups[1]), com_t = pcs_k.commit({&d_t[0], &d_t[1], &d_t[2], &d_m});
        const std::vector<FieldElement> bind{as_element(ctx, com_0.root()), as_element(ctx, com_1.root()), as_element(ctx, com_t.root())};
        const TupleLookupProof proof = prover.prove(groups, table, d_m, bind);

        const TupleLookupVerdict ok = TupleLookup::verify(prover.statement(), proof.proof, bind);
        if (!ok) throw Error(-200, "a valid tuple lookup proof was rejected: " + ok.message);
        const TupleLookupClaims& cl = ok.claims;
        if (cl.z_lo != proof.claims.z_lo || cl.z_t != proof.claims.z_t || cl.f_value != proof.claims.f_value || cl.t_value != proof.claims.t_value ||
            cl.m_value != proof.claims.m_value || cl.alpha != proof.claims.alpha || cl.beta != proof.claims.beta)
            throw Error(-201, "the verifier derived other claims than the prover returned");

        // accepted PROVIDED the three claims hold: the commitment scheme gives the evaluations, with one opening per commitment
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
        std::vector<FieldElement> f_evals = opened(pcs_n, cfg_n, com_0, cl.z_lo, "group 0");
        const std::vector<FieldElement> second = opened(pcs_n, cfg_n, com_1, cl.z_lo, "group 1"), tm = opened(pcs_k, cfg_k, com_t, cl.z_t, "t and m");
        f_evals.insert(f_evals.end(), second.begin(), second.end());
        const std::vector<FieldElement> t_evals(tm.begin(), tm.begin() + w);
        const int which = TupleLookup::check_claims(prover.statement(), cl, f_evals, t_evals, tm[w]);
        if (which != PKT_CLAIM_NONE) throw Error(-203, "the committed columns do not take the claimed values: claim " + std::to_string(which));
        std::vector<FieldElement> other = f_evals;
        other[4][0] ^= 1;  // one evaluation changed: the first claim fails
        if (TupleLookup::check_claims(prover.statement(), cl, other, t_evals, tm[w]) != PKT_CLAIM_F) throw Error(-204, "a changed evaluation passed the claims");
        std::printf("ok n=%u k=%u w=%u c=%u proof_bytes=%zu opening_bytes=%zu commitments=3 phases=1 openings=3 claims=hold\n", n, k, w, c, proof.proof.size(),
                    opening_bytes);

        // a row outside the table: 5 XOR 3 is not 7
        {
            std::vector<FieldElement> bad = f[1][2];
            const size_t x = N / 3;
            f[1][0][x] = {5, 0, 0, 0}, f[1][1][x] = {3, 0, 0, 0}, bad[x] = {7, 0, 0, 0};
            const DeviceVec d_a = montgomery(ctx, f[1][0]), d_b = montgomery(ctx, f[1][1]), d_bad = montgomery(ctx, bad);
            try {
                prover.prove({groups[0], {&d_a, &d_b, &d_bad}}, table, d_m, bind);
                throw Error(-205, "a row outside the table was taken");
            } catch (const Error& e) {
                if (e.code != PK_ERR_UNSATISFIED) throw;
                std::printf("one row outside the table: refused rc=%d (%s)\n", e.code, e.what());
            }
            if (prover.prove(groups, table, d_m, bind).proof != proof.proof) throw Error(-206, "the prover did not stay usable");
        }
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
