// memcheck_pcs_demo.cpp -- a RAM over committed columns, end to end, no Python in the loop: 2^n loads and stores on a memory of 2^k
// cells.  Build the trace on the device (provekit::MemCheck::trace, include/provekit_memcheck.hpp); commit the operation columns
// {a, wv, rv, rt} as one batch, the memory columns {init, fin, ft} as another and {m, s} as a third with WHIR (provekit::WhirPcs), all
// before gamma and beta exist; prove the memory check with the three roots bound; verify it on the host; open the operation columns at
// z_ops AND z_f in one opening, the memory columns at y and m at z_T, and check the four claims on the values the openings bind
// (MemCheck::check_claims).  The load constraint the library leaves to the caller -- a load writes back what it read,
// sum_x eq(tau, x) (1 - s)(wv - rv) = 0 with s = 1 on stores -- is one product sumcheck of four terms over three tables
// (provekit::ProductSumcheck).  Then the three refusals: one rv changed, one m changed, a read from the future.
//
//   memcheck_pcs_demo [n = 10] [k = 6] [seed = 7]
#include <cstdio>
#include <cstdlib>

#include "provekit_memcheck.hpp"
#include "provekit_sumcheck.hpp"
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
    const unsigned n = argc > 1 ? std::atoi(argv[1]) : 10, k = argc > 2 ? std::atoi(argv[2]) : 6;
    uint64_t rng = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 7;
    try {
        Context ctx(0);
        const size_t N = (size_t)1 << n, K = (size_t)1 << k;
        // the program: operation i is a store of a fresh value (s = 1) or a load (s = 0).  A load leaves in the cell what it found there, so
        // its wv is known only once the memory has been replayed: the host does that for the loads' wv alone, the device builds the rest
        std::vector<uint32_t> addr(N);
        std::vector<FieldElement> wv(N), s(N), init(K), cell(K);
        for (size_t j = 0; j < K; j++) cell[j] = init[j] = {splitmix(rng) >> 1, 0, 0, 0};
        for (size_t i = 0; i < N; i++) {
            addr[i] = (uint32_t)(splitmix(rng) % K);
            const bool store = splitmix(rng) & 1;
            s[i] = {store ? 1u : 0u, 0, 0, 0};
            if (store) cell[addr[i]] = {splitmix(rng) >> 1, 0, 0, 0};
            wv[i] = cell[addr[i]];
        }
        const DeviceVec d_addr = MemCheck::addresses(ctx, addr), d_wv = montgomery(ctx, wv), d_init = montgomery(ctx, init), d_s = montgomery(ctx, s);
        DeviceVec d_a(ctx, N), d_rv(ctx, N), d_rt(ctx, N), d_m(ctx, N), d_fin(ctx, K), d_ft(ctx, K);

        MemCheck prover(ctx, n, k, 3);
        prover.trace(d_addr, d_wv, d_init, d_a, d_rv, d_rt, d_fin, d_ft, d_m);
        const MemCheckColumns cols{&d_a, &d_wv, &d_rv, &d_rt, &d_init, &d_fin, &d_ft, &d_m};

        // the one commitment phase, before gamma and beta exist
        const WhirConfig cfg_ops = WhirConfig::for_size(n, 8.0, 4), cfg_mem = WhirConfig::for_size(k, 8.0, 3), cfg_ms = WhirConfig::for_size(n, 8.0, 2);
        WhirPcs pcs_ops(ctx, cfg_ops), pcs_mem(ctx, cfg_mem), pcs_ms(ctx, cfg_ms);
        const PcsCommitment com_ops = pcs_ops.commit({&d_a, &d_wv, &d_rv, &d_rt}), com_mem = pcs_mem.commit({&d_init, &d_fin, &d_ft}), com_ms = pcs_ms.commit({&d_m, &d_s});
        const std::vector<FieldElement> bind{as_element(ctx, com_ops.root()), as_element(ctx, com_mem.root()), as_element(ctx, com_ms.root())};
        const MemCheckProof proof = prover.prove(cols, bind);

        const MemCheckVerdict ok = MemCheck::verify(prover.statement(), proof.proof, bind);
        if (!ok) throw Error(-200, "a valid memory-checking proof was rejected: " + ok.message);
        const MemCheckClaims& cl = ok.claims;
        if (cl.z_ops != proof.claims.z_ops || cl.z_mem != proof.claims.z_mem || cl.z_f != proof.claims.z_f || cl.z_t != proof.claims.z_t ||
            cl.ops_value != proof.claims.ops_value || cl.mem_value != proof.claims.mem_value || cl.rt_value != proof.claims.rt_value || cl.m_value != proof.claims.m_value)
            throw Error(-201, "the verifier derived other claims than the prover returned");

        // accepted PROVIDED the four claims hold: the commitment scheme gives the nine evaluations, with one opening per commitment
        size_t opening_bytes = 0;
        auto opened = [&](const WhirPcs& pcs, const WhirConfig& cfg, const PcsCommitment& com, const std::vector<Point>& points, const char* what) {
            const PcsOpening opening = pcs.open(com, points);
            const std::array<uint8_t, 32> root = com.root();
            std::vector<FieldElement> bound;  // [polynomial][point]
            const PcsVerdict v = WhirPcs::verify(cfg, points, opening.proof, &root, &bound);
            if (!v) throw Error(-202, std::string("a valid opening of ") + what + " was rejected: " + v.message);
            opening_bytes += opening.proof.size();
            return bound;
        };
        const std::vector<FieldElement> at_ops = opened(pcs_ops, cfg_ops, com_ops, {cl.z_ops, cl.z_f}, "the operation columns"),
                                        mem_evals = opened(pcs_mem, cfg_mem, com_mem, {cl.z_mem}, "the memory columns"),
                                        at_t = opened(pcs_ms, cfg_ms, com_ms, {cl.z_t}, "m");
        const std::vector<FieldElement> ops_evals{at_ops[0], at_ops[2], at_ops[4], at_ops[6]};  // a, wv, rv, rt at z_ops; at_ops[7] = rt(z_f)
        const int which = MemCheck::check_claims(prover.statement(), cl, ops_evals, mem_evals, at_ops[7], at_t[0]);
        if (which != PKM_CLAIM_NONE) throw Error(-203, "the committed columns do not take the claimed values: claim " + std::to_string(which));
        std::vector<FieldElement> other = ops_evals;
        other[2][0] ^= 1;  // one evaluation changed: the first claim fails
        if (MemCheck::check_claims(prover.statement(), cl, other, mem_evals, at_ops[7], at_t[0]) != PKM_CLAIM_OPS) throw Error(-204, "a changed evaluation passed the claims");

        // the load constraint: eq(tau, x) (wv - rv - s wv + s rv) sums to 0 over the tables {s, wv, rv}
        const FieldElement one = montgomery(ctx, {{1, 0, 0, 0}}).to_host()[0],
                           minus_one = montgomery(ctx, {{0x43e1f593f0000000ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL}}).to_host()[0];
        SumcheckStatement load(n, 3, true);
        load.add_term(one, {1}).add_term(minus_one, {2}).add_term(minus_one, {0, 1}).add_term(one, {0, 2});
        std::vector<FieldElement> tau(n);  // in a circuit: squeezed after the commitments.  Here: any point
        for (FieldElement& t : tau) t = {splitmix(rng), splitmix(rng), splitmix(rng), splitmix(rng) >> 4};
        ProductSumcheck row(ctx, load);
        const SumcheckProof load_proof = row.prove({&d_s, &d_wv, &d_rv}, tau);
        const FieldElement zero{0, 0, 0, 0};
        const SumcheckVerdict load_ok = ProductSumcheck::verify(load, load_proof.proof, tau, {}, &zero);
        if (!load_ok) throw Error(-205, "the load constraint's sumcheck was rejected: " + load_ok.message);
        std::printf("ok n=%u k=%u proof_bytes=%zu opening_bytes=%zu commitments=3 phases=1 openings=3 claims=hold load_constraint=proved load_proof_bytes=%zu\n", n, k,
                    proof.proof.size(), opening_bytes, load_proof.proof.size());

        // the three refusals; after each the same prover proves the good trace again
        auto refused = [&](const MemCheckColumns& bad, const char* what, MemCheck& with, const MemCheckColumns& good, const std::vector<FieldElement>& roots,
                           const std::vector<uint8_t>& want) {
            try {
                with.prove(bad, roots);
                throw Error(-206, std::string(what) + ": an inconsistent trace was taken");
            } catch (const Error& e) {
                if (e.code != PK_ERR_UNSATISFIED) throw;
                std::printf("%s: refused rc=%d (%s)\n", what, e.code, e.what());
            }
            if (with.prove(good, roots).proof != want) throw Error(-207, "the prover did not stay usable");
        };
        {
            std::vector<FieldElement> rv = d_rv.to_host(), m = d_m.to_host();
            rv[N / 3][0] ^= 1, m[0][0] ^= 1;
            const DeviceVec d_bad_rv(ctx, rv), d_bad_m(ctx, m);
            MemCheckColumns bad = cols;
            bad.rv = &d_bad_rv;
            refused(bad, "one rv changed", prover, cols, bind, proof.proof);
            bad = cols, bad.m = &d_bad_m;
            refused(bad, "one m changed", prover, cols, bind, proof.proof);
        }
        {
            // provekit_memcheck.h's trace: one cell of init 0 in use; operation 0 claims (rv, rt) = (7, 2) and writes 7, operation 1 claims
            // (0, 0) and writes 7; fin = 7, ft = 1.  The two multisets are equal; only the time check refuses it
            auto column = [&](std::initializer_list<uint64_t> values) {
                std::vector<FieldElement> v;
                for (uint64_t x : values) v.push_back({x, 0, 0, 0});
                return montgomery(ctx, v);
            };
            const DeviceVec a = column({0, 0}), w = column({7, 7}), rv = column({7, 0}), rt = column({2, 0}), in = column({0, 5}), fin = column({7, 5}), ft = column({1, 0}),
                            m = column({1, 1}), rv_real = column({0, 7}), rt_real = column({0, 1}), ft_real = column({2, 0}), m_real = column({2, 0});
            MemCheck tiny(ctx, 1, 1);
            const MemCheckColumns real{&a, &w, &rv_real, &rt_real, &in, &fin, &ft_real, &m_real};
            const std::vector<uint8_t> want = tiny.prove(real).proof;
            refused({&a, &w, &rv, &rt, &in, &fin, &ft, &m}, "a read from the future", tiny, real, {}, want);
        }
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
