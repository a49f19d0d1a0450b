// pcs.hpp -- what the sources of libprovekit_whir.so share: which configs the library takes, the IO pattern of an opening proof, and
// the statement value every layer passes.  Host only.  The entry points are declared by the public headers alone, included here.
// The wire rules (sponge, hint framing, STIR indexes, PoW bytes) are protocol.hpp's; the verifier side of the transcript and the WHIR
// walk are verify/core.hpp's.
#pragma once
#include <string>

#include "../../../include/provekit_whir.h"
#include "../../../include/provekit_whir_hiding.h"
#include "../../../include/provekit_whir_sparse.h"
#include "../verify/core.hpp"
#include "evaluate.hpp"

namespace pkw {

using pk::fe;

extern thread_local std::string g_error;  // pkw_create_error
inline int refuse(const std::string& why) {
    g_error = why;
    return PK_ERR_BAD_ARG;
}

// a config both sides take: the prover's bounds (what pk_whir_r1cs_io_pattern refuses, the product library's own rule) and the
// verifier core's
inline bool config_ok(const pk_whir_config* c, std::string& why) {
    if (!c) {
        why = "null config";
        return false;
    }
#ifndef PKW_HOST_ONLY  // the sanitizer build of the verifier (asan_main.cpp) links no product library: the core's rule alone
    size_t n = 0;
    if (pk_whir_r1cs_io_pattern(1, c, c, nullptr, 0, &n) != PK_OK) {
        why = "pk_whir_r1cs_io_pattern refuses this config";
        return false;
    }
#endif
    return pkv::config_ok(*c, why);
}

// "<domain>" then commit_statement, the statement, add_whir_proof -- the operations and labels of whir_config.hip's restatement of
// whir's pattern, zero-count operations omitted where whir guards them.  l = 0: the evaluation statement of pkw_open; l >= 1: the
// linear statement of pkw_open_linear (its own domain label, the tags after the points, the sums after the evaluations).  hiding: the
// evaluation statement of pkw_open_hiding over the extended config -- the same operations under a label of their own
inline std::string io_pattern(const pk_whir_config& c, unsigned q, unsigned l = 0, bool hiding = false) {
    std::string d = hiding ? "provekit-hip/whir-pcs-hiding/v1" : l ? "provekit-hip/whir-pcs-linear/v1" : "provekit-hip/whir-pcs/v1";
    auto op = [&](char kind, size_t count, const char* label) {
        d.push_back('\0');
        d.push_back(kind);
        if (kind == 'A' || kind == 'S') d += std::to_string(count);
        d += label;
    };
    auto A = [&](size_t n, const char* l) { if (n) op('A', n, l); };
    auto S = [&](size_t n, const char* l) { if (n) op('S', n, l); };
    auto pow = [&](double bits) {
        if (bits > 0.0) {
            S(pk::units_for_bytes(pk::POW_CHALLENGE_BYTES), "pow_queries");
            A(pk::POW_NONCE_BYTES, "pow-nonce");
        }
    };
    auto sumcheck = [&](unsigned rounds) {
        for (unsigned i = 0; i < rounds; i++) {
            A(3, "sumcheck_poly");
            S(1, "folding_randomness");
        }
    };
    auto openings = [&](size_t domain, unsigned queries, const char* label) {
        S(pk::units_for_bytes((size_t)queries * pk::stir_query_bytes(domain, c.folding_factor)), label);
        op('H', 0, "stir_answers");
        op('H', 0, "merkle_proof");
    };
    // commit_statement
    A(1, "merkle_digest");
    S(c.commitment_ood_samples, "ood_query");
    A((size_t)c.commitment_ood_samples * c.batch_size, "ood_ans");
    if (c.batch_size > 1) S(1, "batching_randomness");
    // the statement: where, and what the polynomials are claimed to be there
    A((size_t)q * c.n_vars, "points");
    A(l, "tags");
    A((size_t)q * c.batch_size, "evaluations");
    A((size_t)l * c.batch_size, "sums");
    // add_whir_proof
    const unsigned k = c.folding_factor;
    S(1, "initial_combination_randomness");
    sumcheck(k);
    size_t domain = (size_t)1 << (c.n_vars + c.starting_log_inv_rate);
    for (unsigned r = 0; r < c.n_rounds; r++) {
        A(1, "merkle_digest");
        S(c.ood_samples[r], "ood_query");
        A(c.ood_samples[r], "ood_ans");
        pow(c.pow_bits[r]);
        openings(domain, c.num_queries[r], "stir_queries");
        S(1, "combination_randomness");
        sumcheck(k);
        domain >>= 1;
    }
    const unsigned final_vars = c.n_vars - k * (c.n_rounds + 1);
    A((size_t)1 << final_vars, "final_coeffs");
    pow(c.final_pow_bits);
    openings(domain, c.final_queries, "final_queries");
    sumcheck(final_vars);
    pow(c.final_folding_pow_bits);
    op('H', 0, "deferred_weight_evaluations");
    return d;
}

// the device memory one opening needs, in field elements.  Every buffer is rounded up to 8 elements.  The sizes of a commit's buffers
// are `sizes(batch, n_vars, log_inv_rate, &leaves, &nodes, &scratch)`: pk_commit_sizes' rule outside a device set (leaves = rows * width,
// nodes = 2 rows, scratch = 2 rows * width) for plan(), which is host only and has no context -- pkw_scheme_arena_bytes -- and
// pk_commit_sizes itself under the context's set for the arena a scheme allocates (pcs.cpp)
struct Plan {
    size_t total = 0, scratch = 0;
};
inline size_t round8(size_t fes) { return (fes + 7) & ~(size_t)7; }
template <class Sizes>
inline int plan_with(const pk_whir_config& c, Sizes sizes, Plan& p) {
    p = Plan{};
    const unsigned n = c.n_vars, k = c.folding_factor;
    const size_t N = (size_t)1 << n;
    size_t leaves = 0, nodes = 0, scratch = 0;
    if (int rc = sizes(c.batch_size, n, c.starting_log_inv_rate, &leaves, &nodes, &scratch)) return rc;
    p.scratch = scratch;  // pkw_commit's
    // ... and a linear opening's deferred evaluations borrow it for the partials of EVAL_MAX_BATCH tables: more than the commit's
    // where batch * 2^(n + rate) < 16
    p.scratch = std::max(p.scratch, eval_partial_fes(EVAL_MAX_BATCH, n));
    p.total+= 3 * round8(N) + 2 * round8(N / 2 ? N / 2 : 1);              // combined coefficients, p and w with their halves
    unsigned nv = n, rate = c.starting_log_inv_rate;
    for (unsigned r = 0; r <= c.n_rounds; r++) {  // the folded polynomials, the last one being the final coefficients
        nv -= k;
        p.total += round8((size_t)1 << nv);
        if (r == c.n_rounds) break;
        rate += k - 1;
        if (int rc = sizes(1, nv, rate, &leaves, &nodes, &scratch)) return rc;
        p.total += round8(leaves) + round8(nodes);
        p.scratch = std::max(p.scratch, scratch);
    }
    p.total += round8(p.scratch);
    // pkw_open's evaluations: the points, the kernel's partial sums, the results
    p.total += round8((size_t)PKW_MAX_POINTS * n) + round8(eval_partial_fes(c.batch_size, n)) + round8((size_t)PKW_MAX_POINTS * c.batch_size);
    return PK_OK;
}
inline Plan plan(const pk_whir_config& c) {
    Plan p;
    plan_with(c, [&](unsigned batch, unsigned nv, unsigned rate, size_t* leaves, size_t* nodes, size_t* scratch) {
        const size_t rows = (size_t)1 << (nv + rate - c.folding_factor), width = (size_t)batch << c.folding_factor;
        *leaves = rows * width, *nodes = 2 * rows, *scratch = 2 * rows * width;
        return (int)PK_OK;
    }, p);
    return p;
}

// ONE statement about the committed polynomials, as every layer between the C entry points and the transcript passes it: q points,
// then l weights bound by the caller's tags (l = 0: the evaluation statement of pkw_open / pkw_verify).  The weights are dense tables
// or index/value lists, never both -- device memory for an opening, host memory for a verification, where dense may also be null or
// hold null entries: tables the verifier was not given
struct SparseWeights;  // sparse.hpp
struct Statement {
    const uint64_t* points = nullptr;  // q * n_vars elements
    unsigned q = 0;
    const uint64_t* tags = nullptr;  // l elements
    unsigned l = 0;
    const uint64_t* const* dense = nullptr;
    const SparseWeights* sparse = nullptr;
    bool hiding = false;  // the statement of a hiding opening (points (0, z_i), l = 0): the pattern carries the hiding label
};
// what a verification hands back next to its verdict; every pointer may be null
struct VerifyOutputs {
    uint64_t *evals = nullptr, *sums = nullptr, *fold_point = nullptr, *deferred = nullptr;
    unsigned* unchecked = nullptr;
};

// The two rules a config must keep for a hiding commitment (provekit_whir_hiding.h): the batch is the caller's 1..3 polynomials and
// g, and the values of each masked polynomial that leave through the committed codeword's openings and the out-of-domain answers
// do not outnumber its 2^(n_vars - 1) mask coefficients
inline bool hiding_config_ok(const pk_whir_config& c, std::string& why) {
    if (c.batch_size < 2 || c.batch_size > 4) {
        why = "a hiding commitment holds 1..3 polynomials and g: batch_size must be 2..4";
        return false;
    }
    if (c.n_vars < 2) {
        why = "a hiding commitment holds polynomials of n_vars - 1 >= 1 variables: n_vars must be at least 2";
        return false;
    }
    const uint64_t mask = (uint64_t)1 << (c.n_vars - 1);
    const uint64_t leave = c.commitment_ood_samples + ((uint64_t)(c.n_rounds ? c.num_queries[0] : c.final_queries) << c.folding_factor);
    if (leave > mask) {
        why = "mask budget: " + std::to_string(leave) + " values of each masked polynomial leave through the proof (commitment_ood_samples + " +
              (c.n_rounds ? "num_queries[0]" : "final_queries") + " * 2^folding_factor), more than its " + std::to_string(mask) + " mask coefficients";
        return false;
    }
    return true;
}

// the counts of a linear statement, refused with a reason
inline bool linear_counts_ok(unsigned q, unsigned l, std::string& why) {
    if (q > PKW_MAX_POINTS) {
        why = "the number of points must be 0..64";
        return false;
    }
    if (l < 1 || l > PKW_MAX_WEIGHTS) {
        why = "the number of weights must be 1..16";
        return false;
    }
    return true;
}

}  // namespace pkw
