// whir_config.hip -- the scheme's shape, host only: which WHIR configs the prover runs and WhirConfig::new, the size of a scheme's
// arena, and the spongefish IO patterns (the list of operations a proof performs, which is also its domain separator).  Nothing here
// touches a device: every entry point works without a GPU.  Also here, for want of a better home: copy_out, the one way a string goes
// into a caller's (buf, cap, *len), which the entry points below and pk_scheme_domain_separator (prover.hip) share.
#include <cmath>

#include "internal.hpp"
#include "protocol.hpp"

namespace pk {

// the WHIR configs this prover runs: nullptr if `c` is one, else why not.  pk_scheme_create refuses the rest, and so does every
// host-only entry point that takes a config.
const char* whir_config_error(const pk_whir_config* c) {
    if (!c) return "null pointer";
    if (c->folding_factor < 1 || c->folding_factor > 8) return "folding factor out of range (1 .. 8)";
    if (c->n_rounds > PK_MAX_WHIR_ROUNDS) return "too many WHIR rounds";
    if (c->n_vars < c->folding_factor * (c->n_rounds + 1)) return "WHIR rounds exceed the number of variables";
    if (c->commitment_ood_samples > 4) return "too many OOD samples";
    if (c->batch_size < 1 || c->batch_size > 4) return "batch size out of range";
    // the evaluation domain must exist in BN254-Fr (two-adicity 28) and the codeword must fit pk_rs_encode's bound
    if (c->starting_log_inv_rate < 1 || c->starting_log_inv_rate > 28 || c->n_vars > 28 - c->starting_log_inv_rate)
        return "n_vars + starting_log_inv_rate exceeds 28";
    if (c->n_vars + c->starting_log_inv_rate - c->folding_factor > 27) return "codeword has more than 2^27 rows";
    for (unsigned r = 0; r < c->n_rounds; r++)
        if (c->ood_samples[r] > 4) return "too many OOD samples";
    return nullptr;
}

// the blinding polynomial's variables less one: 2^nb = next_power_of_two(4 m_0)
unsigned blinding_log_len(unsigned m_0) {
    unsigned nb = 0;
    while (((size_t)1 << nb) < 4 * (size_t)m_0) nb++;
    return nb;
}

// arena = the sum of pk_prove's allocations (nothing is freed inside a proof).  With N = 2^m, R = 2^starting_log_inv_rate,
// F = 2^folding_factor: f, g in both forms 4N; initial codeword batch*R*N and its tree 2R/F N; working polynomial and the
// sumcheck ping-pong 4N; round codewords (domain halves each round) < R N, their trees < 2R/F N, folded polynomials
// < 2/F N; deferred eq table N; a, b, c, eq and the second eq table 5*2^m_0; external rows 3*num_witnesses.  The small
// blinding scheme (2^(nb+1) <= 2^9 elements) and alignment are covered by the constant.
size_t scheme_arena_bytes(unsigned m, unsigned m_0, size_t num_witnesses, const pk_whir_config& w) {
    const double N = (double)((size_t)1 << m), R = (double)((size_t)1 << w.starting_log_inv_rate), F = (double)((size_t)1 << w.folding_factor);
    const double units = 4.0 + w.batch_size * R + 2.0 * R / F + 4.0 + R + 2.0 * R / F + 2.0 / F + 1.0;
    const double fes = units * N + 5.0 * (double)((size_t)1 << m_0) + 3.0 * (double)num_witnesses;
    return (size_t)(1.05 * 32.0 * fes) + ((size_t)64 << 20);
}

// create_witness_io_pattern (provekit/prover/src/noir_proof_scheme.rs:94-109) with witness_io_pattern.rs:18-41: the spongefish
// op list "<domain>\0A2shape[\0A<n>pub_inputs][\0S<n>wb:challenges]"
std::string witness_io_pattern(size_t n_public, size_t n_challenges) {
    std::string d = "\xF0\x9F\x93\x9C";  // "📜"
    d.push_back('\0');
    d += "A2shape";
    if (n_public) {
        d.push_back('\0');
        d += "A" + std::to_string(n_public) + "pub_inputs";
    }
    if (n_challenges) {
        d.push_back('\0');
        d += "S" + std::to_string(n_challenges) + "wb:challenges";
    }
    return d;
}

// WhirR1CSScheme::create_io_pattern (provekit/common/src/whir_r1cs.rs:28-39) restated:
//   IOPattern::new("🌪️").commit_statement(w).add_rand(m_0).commit_statement(b).add_zk_sumcheck_polynomials(m_0)
//            .add_whir_proof(b).hint("claimed_evaluations").add_whir_proof(w)
// provekit's own labels (utils/sumcheck.rs:119-142) are in the tree.  commit_statement / add_whir_proof live in whir @3e7f8c2
// (absent): their OPERATIONS are pinned by the in-tree Go verifier's read order (mtUtilities.go:51-76, whir.go:51-220) and the
// labels "stir_answers", "merkle_proof", "deferred_weight_evaluations", "pow-nonce" by its pattern walker (common.go:41-100);
// the remaining labels are whir's / spongefish-pow's as published (merkle_digest, ood_query, ood_ans, sumcheck_poly,
// folding_randomness, combination_randomness, pow_queries, stir_queries, final_coeffs, final_queries) -- UNPINNED here, which is
// why a caller that holds the reference's bytes overrides this string (pk_scheme_set_io_pattern).  Zero-count operations are
// omitted exactly where whir guards them (no OOD samples, no grinding).
std::string whir_r1cs_io_pattern(unsigned m_0, const pk_whir_config& w, const pk_whir_config& h) {
    std::string d = "\xF0\x9F\x8C\xAA\xEF\xB8\x8F";  // "🌪️"
    auto op = [&](char kind, size_t count, const char* label) {
        d.push_back('\0');
        d.push_back(kind);
        if (kind == 'A' || kind == 'S') d += std::to_string(count);
        d += label;
    };
    auto A = [&](size_t n, const char* l) { if (n) op('A', n, l); };
    auto S = [&](size_t n, const char* l) { if (n) op('S', n, l); };
    auto challenge_bytes = [&](size_t n, const char* l) { S(units_for_bytes(n), l); };
    auto pow = [&](double bits) {  // spongefish-pow challenge_pow: the challenge bytes, then the nonce's
        if (bits > 0.0) {
            challenge_bytes(POW_CHALLENGE_BYTES, "pow_queries");
            A(POW_NONCE_BYTES, "pow-nonce");
        }
    };
    auto add_ood = [&](size_t samples, size_t batch) {
        S(samples, "ood_query");
        A(samples * batch, "ood_ans");
    };
    auto add_sumcheck = [&](unsigned rounds) {
        for (unsigned i = 0; i < rounds; i++) {
            A(3, "sumcheck_poly");
            S(1, "folding_randomness");
        }
    };
    auto commit_statement = [&](const pk_whir_config& c) {
        A(1, "merkle_digest");
        add_ood(c.commitment_ood_samples, c.batch_size);
        if (c.batch_size > 1) S(1, "batching_randomness");  // drawn right after the commitment (mtUtilities.go:71-75)
    };
    auto add_whir_proof = [&](const pk_whir_config& c) {
        const unsigned k = c.folding_factor;
        S(1, "initial_combination_randomness");
        add_sumcheck(k);
        size_t domain = (size_t)1 << (c.n_vars + c.starting_log_inv_rate);
        for (unsigned r = 0; r < c.n_rounds; r++) {
            A(1, "merkle_digest");
            add_ood(c.ood_samples[r], 1);
            pow(c.pow_bits[r]);
            challenge_bytes((size_t)c.num_queries[r] * stir_query_bytes(domain, k), "stir_queries");
            op('H', 0, "stir_answers");
            op('H', 0, "merkle_proof");
            S(1, "combination_randomness");
            add_sumcheck(k);
            domain >>= 1;
        }
        const unsigned final_vars = c.n_vars - k * (c.n_rounds + 1);
        A((size_t)1 << final_vars, "final_coeffs");
        pow(c.final_pow_bits);
        challenge_bytes((size_t)c.final_queries * stir_query_bytes(domain, k), "final_queries");
        op('H', 0, "stir_answers");
        op('H', 0, "merkle_proof");
        add_sumcheck(final_vars);
        pow(c.final_folding_pow_bits);  // once, after the last round (whir.go:196-201)
        op('H', 0, "deferred_weight_evaluations");
    };
    commit_statement(w);
    S(m_0, "rand");
    commit_statement(h);
    A(1, "Sum of G over boolean hypercube");
    S(1, "Rho");
    for (unsigned i = 0; i < m_0; i++) {
        A(4, "Sumcheck Polynomials");
        S(1, "Sumcheck Random");
    }
    A(2, "Polynomial sums");
    add_whir_proof(h);
    op('H', 0, "claimed_evaluations");
    add_whir_proof(w);
    return d;
}

// do the caller's IO-pattern bytes declare the operations pk_prove performs for (m_0, w, h)?  "" = yes, else the first difference
std::string io_pattern_mismatch(const std::string& theirs, unsigned m_0, const pk_whir_config& w, const pk_whir_config& h) {
    std::vector<IoOp> a, b;
    std::string err;
    if (!io_pattern_parse(theirs, a, err)) return err;
    if (!io_pattern_parse(whir_r1cs_io_pattern(m_0, w, h), b, err)) return "internal: " + err;
    auto name = [](const IoOp& o) { return std::string(1, o.kind) + (o.kind == 'A' || o.kind == 'S' ? std::to_string(o.count) : std::string()); };
    for (size_t i = 0; i < a.size() && i < b.size(); i++)
        if (a[i].kind != b[i].kind || a[i].count != b[i].count)
            return "IO pattern operation #" + std::to_string(i + 1) + " (after merging) is " + name(a[i]) + " but this scheme's prover performs " + name(b[i]);
    if (a.size() != b.size())
        return "IO pattern declares " + std::to_string(a.size()) + " operations (after merging), this scheme's prover performs " + std::to_string(b.size());
    return "";
}

// a string into the caller's (buf, cap): *len is always its size, the bytes are copied only where they fit (buf = null: size query)
void copy_out(const std::string& s, void* buf, size_t cap, size_t* len) {
    *len = s.size();
    if (buf && cap >= s.size()) memcpy(buf, s.data(), s.size());
}

}  // namespace pk

using namespace pk;

extern "C" {

int pk_scheme_arena_bytes(unsigned m, unsigned m_0, size_t num_witnesses, const pk_whir_config* whir_witness, size_t* bytes) {
    if (!bytes || m > 28 || m_0 > m || whir_config_error(whir_witness)) return PK_ERR_BAD_ARG;
    *bytes = scheme_arena_bytes(m, m_0, num_witnesses, *whir_witness);
    return PK_OK;
}

// WhirConfig::new for provekit's parameters (provekit/r1cs-compiler/src/whir_r1cs.rs:38-53); see include/provekit_hip.h
int pk_whir_config_derive(unsigned n_vars, unsigned batch_size, unsigned folding_factor, unsigned starting_log_inv_rate,
                          unsigned security_level, int pow_bits, pk_whir_config* out) {
    // n_vars < folding_factor: whir would run no folding round at all; this prover always folds folding_factor variables before
    // the first re-commit (pk_scheme_create requires n_vars >= folding_factor * (n_rounds + 1)), so the smallest scheme is
    // n_vars = folding_factor -- m_0 >= 2 for the blinding scheme at fold 4 (include/provekit_hip.h)
    if (!out || folding_factor < 1 || folding_factor > 8 || n_vars < folding_factor || starting_log_inv_rate < 1 || batch_size < 1) return PK_ERR_BAD_ARG;
    const unsigned k = folding_factor;
    const double field_bits = 254.0, sec = (double)security_level;
    // default_max_pow(num_variables, log_inv_rate) = num_variables + log_inv_rate - 3 (whir::parameters)
    const double pow_param = pow_bits >= 0 ? (double)pow_bits : (double)(n_vars + starting_log_inv_rate) - 3.0;
    const double protocol_sec = sec > pow_param ? sec - pow_param : 0.0;
    // ConjectureList: log_eta = -(log_inv_rate + 1); list_size_bits = (nv + log_inv_rate) - log_eta
    auto list_size_bits = [](unsigned nv, unsigned rate) { return (double)(nv + rate) + (double)(rate + 1); };
    auto ood_for = [&](unsigned nv, unsigned rate) -> unsigned {
        for (unsigned s = 1; s < 64; s++) {
            double err = 2.0 * list_size_bits(nv, rate) + (double)nv * s;
            if ((double)s * field_bits + 1.0 - err >= sec) return s;
        }
        return 64;
    };
    auto queries_for = [&](unsigned rate) { return (unsigned)ceil(protocol_sec / (double)rate); };
    pk_whir_config c;
    memset(&c, 0, sizeof c);
    c.n_vars = n_vars;
    c.batch_size = batch_size;
    c.folding_factor = k;
    c.starting_log_inv_rate = starting_log_inv_rate;
    const unsigned final_vars = n_vars % k;
    c.n_rounds = (n_vars - final_vars) / k - 1;
    if (c.n_rounds > PK_MAX_WHIR_ROUNDS) return PK_ERR_BAD_ARG;
    c.commitment_ood_samples = ood_for(n_vars, starting_log_inv_rate);
    unsigned nv = n_vars - k, rate = starting_log_inv_rate;
    for (unsigned r = 0; r < c.n_rounds; r++) {
        const unsigned next_rate = rate + (k - 1);
        c.num_queries[r] = queries_for(rate);  // queries against the OLD rate, the rest against the new one
        c.ood_samples[r] = ood_for(nv, next_rate);
        const double query_error = (double)c.num_queries[r] * rate;
        const double combination_error = field_bits - (log2((double)(c.ood_samples[r] + c.num_queries[r])) + list_size_bits(nv, next_rate) + 1.0);
        const double e = query_error < combination_error ? query_error : combination_error;
        c.pow_bits[r] = sec > e ? sec - e : 0.0;
        nv -= k;
        rate = next_rate;
    }
    c.final_queries = queries_for(rate);
    const double fq = (double)c.final_queries * rate;
    c.final_pow_bits = sec > fq ? sec - fq : 0.0;
    c.final_folding_pow_bits = sec > field_bits - 1.0 ? sec - (field_bits - 1.0) : 0.0;
    *out = c;
    return PK_OK;
}

int pk_whir_r1cs_io_pattern(unsigned m_0, const pk_whir_config* whir_witness, const pk_whir_config* whir_for_hiding_spartan, uint8_t* buf,
                            size_t cap, size_t* len) {
    if (!len || m_0 < 1 || m_0 > 27 || whir_config_error(whir_witness) || whir_config_error(whir_for_hiding_spartan)) return PK_ERR_BAD_ARG;
    copy_out(whir_r1cs_io_pattern(m_0, *whir_witness, *whir_for_hiding_spartan), buf, cap, len);
    return PK_OK;
}

int pk_io_pattern_check(const uint8_t* pattern, size_t n, unsigned m_0, const pk_whir_config* whir_witness,
                        const pk_whir_config* whir_for_hiding_spartan, char* why, size_t why_cap) {
    if (why && why_cap) why[0] = 0;
    if (!pattern || m_0 < 1 || m_0 > 27 || whir_config_error(whir_witness) || whir_config_error(whir_for_hiding_spartan)) return PK_ERR_BAD_ARG;
    const std::string bad = io_pattern_mismatch(std::string((const char*)pattern, n), m_0, *whir_witness, *whir_for_hiding_spartan);
    if (bad.empty()) return PK_OK;
    if (why && why_cap) snprintf(why, why_cap, "%s", bad.c_str());
    return PK_ERR_IO_PATTERN;
}

}  // extern "C"
