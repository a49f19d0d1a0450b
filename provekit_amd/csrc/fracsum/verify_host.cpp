// verify_host.cpp -- the host half of libprovekit_fracsum.so's C ABI: the statements' rules, the two outer IO patterns and the two
// verifiers.  No device code and no HIP call; of other libraries it calls pks_verify and pks_check_name (provekit_sumcheck.h).
// This file and its headers are also what the sanitizer build (make asan, fracsum/asan_main.cpp) compiles, next to the sumcheck
// library's host verifier.
#include <vector>

#include "layout.hpp"

namespace pkf {
thread_local std::string g_error;
}

namespace {

using pk::fe;

using pk::verdict;

struct Sum {
    fe P, Q, value_p, value_q;
    fe point[PKF_MAX_VARS];
};

// What the verifier adds to the chain's rule (pkf::Chain, statement.hpp): the fraction (P, Q) of the top values with its three checks,
// and over unit leaves the check that the last layer's u is the table the statement says.
struct Verifying : pkf::Chain {
    const fe* wanted;  // (num, den) or NULL
    fe P, Q;
    Verifying(const pkf_statement& st, const fe* expected_or_null) : Chain(st), wanted(expected_or_null) {}
    bool check_top(const fe* top, pkv_result* result) {
        pkf::fraction_of(top, P, Q);
        if (pk::is_zero(Q)) return verdict(result, PKF_CHECK_DENOMINATOR, pkf::TOP_BYTES, "Q = 0: a denominator is zero"), false;
        if (s.unit && s.n == 1 && !(pk::fe_eq(top[0], pk::fe_one()) && pk::fe_eq(top[1], pk::fe_one())))
            return verdict(result, PKF_CHECK_UNIT, pkf::TOP_BYTES, "a top numerator of a unit statement is not 1"), false;
        if (wanted && !pkf::same_fraction(P, Q, wanted[0], wanted[1]))
            return verdict(result, PKF_CHECK_FRACTION, pkf::TOP_BYTES, "the fraction of the top values is not the expected one"), false;
        return true;
    }
    bool check_finals(unsigned d, const fe* finals, const fe* ch, pkv_result* result) const {
        if (!pkf::unit_layer(s, d) || pkf::unit_final_ok(finals, ch[0])) return true;
        return verdict(result, PKF_CHECK_UNIT, layer_at(d) + layer_bytes(d), "layer " + std::to_string(d) + ": the final value of u is not 1 + lambda qR"), false;
    }
};

// One fractional-sum proof of exactly pkf::proof_bytes(s) bytes against a parsed pattern: gkr/chain.hpp's walk.  expected: (num, den)
// or NULL.  PK_OK: the verdict is in *result, its offset in bytes of this proof, `layer` what it is about; accepted: `out` is written.
int verify_sum(const pkf_statement& s, const pkv::Statement& st, const uint64_t* bind, const fe* expected, const uint8_t* proof, Sum& out, unsigned& layer,
               pkv_result* result) {
    Verifying rule(s, expected);
    if (int rc = pk::gkr::verify_chain(rule, st, bind, proof, out.point, layer, result, pkf::g_error)) return rc;
    if (!result->accepted) return PK_OK;
    out.P = rule.P, out.Q = rule.Q, out.value_p = rule.claim.has_p ? rule.claim.cp : pk::fe_one(), out.value_q = rule.claim.cq;
    return PK_OK;
}

}  // namespace

extern "C" {

int pkf_abi_version(void) { return 1; }

const char* pkf_check_name(int check) {
    return check == PKF_CHECK_FRACTION ? "FRACTION" : check == PKF_CHECK_DENOMINATOR ? "DENOMINATOR" : check == PKF_CHECK_UNIT ? "UNIT" : pks_check_name(check);
}

const char* pkf_create_error(void) { return pkf::g_error.c_str(); }

int pkf_io_pattern(const pkf_statement* stmt, uint8_t* buf, size_t cap, size_t* len) { return pk::pattern_out<pkf::Lib>(stmt, buf, cap, len); }
int pkf_proof_bytes(const pkf_statement* stmt, size_t* len) { return pk::size_out<pkf::Lib>(stmt, len, [](auto& s) { return pkf::proof_bytes(s); }); }
int pkf_lookup_io_pattern(const pkf_lookup_statement* stmt, uint8_t* buf, size_t cap, size_t* len) { return pk::pattern_out<pkf::Lib>(stmt, buf, cap, len); }
int pkf_lookup_proof_bytes(const pkf_lookup_statement* stmt, size_t* len) { return pk::size_out<pkf::Lib>(stmt, len, [](auto& s) { return pkf::proof_bytes(s); }); }

unsigned pkf_tail_max_n(void) { return pkf::TAIL_MAX_N; }

int pkf_verify(const pkf_statement* stmt, const uint8_t* io_pattern_or_null, size_t io_pattern_len, const uint64_t* bind, const uint64_t* expected_fraction_or_null,
               const uint8_t* proof, size_t len, uint64_t* fraction_out, uint64_t* point_out, uint64_t* value_p_out, uint64_t* value_q_out, unsigned* layer_out,
               pkv_result* result) {
    std::string why;
    if (!result || (!proof && len)) return pkf::refuse("null pointer");
    if (!pkf::statement_ok(stmt, why)) return pkf::refuse(why);
    const pkf_statement& s = *stmt;
    if (s.n_bind && !bind) return pkf::refuse("the statement binds elements: pass them");
    if (!pkf::elements_below_p(bind, s.n_bind, "bind", why)) return pkf::refuse(why);
    if (expected_fraction_or_null && !pkf::elements_below_p(expected_fraction_or_null, 2, "expected_fraction", why)) return pkf::refuse(why);
    try {
        pkv::Statement st;
        if (int rc = pk::parse_pattern(st, io_pattern_or_null, io_pattern_len, pkf::io_pattern(s), pkf::g_error)) return rc;
        if (layer_out) *layer_out = 0;
        // framing first: every part has a fixed length, so a proof of another length is judged before any part is read
        const size_t total = pkf::proof_bytes(s);
        if (len < total) return verdict(result, PKV_CHECK_TRANSCRIPT_SHORT, len, "the proof is shorter than its parts"), PK_OK;
        if (len > total) return verdict(result, PKV_CHECK_TRAILING_BYTES, total, "bytes left after the proof"), PK_OK;
        fe expected[2];
        if (expected_fraction_or_null) expected[0] = pk::h_load(expected_fraction_or_null), expected[1] = pk::h_load(expected_fraction_or_null + 4);
        Sum out;
        unsigned layer = 0;
        if (int rc = verify_sum(s, st, bind, expected_fraction_or_null ? expected : nullptr, proof, out, layer, result)) return rc;
        if (layer_out) *layer_out = layer;
        if (!result->accepted) return PK_OK;
        if (fraction_out) pkf::put_fe(fraction_out, out.P), pkf::put_fe(fraction_out + 4, out.Q);
        if (value_p_out && !s.unit) pkf::put_fe(value_p_out, out.value_p);
        if (value_q_out) pkf::put_fe(value_q_out, out.value_q);
        if (point_out) memcpy(point_out, out.point, 32 * (size_t)s.n);
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

int pkf_lookup_verify(const pkf_lookup_statement* stmt, const uint8_t* io_pattern_or_null, size_t io_pattern_len, const uint64_t* bind, const uint8_t* proof,
                      size_t len, pkf_lookup_claims* claims_out, int* side_out, unsigned* layer_out, pkv_result* result) {
    std::string why;
    if (!result || (!proof && len)) return pkf::refuse("null pointer");
    if (!pkf::statement_ok(stmt, why)) return pkf::refuse(why);
    const pkf_lookup_statement& s = *stmt;
    if (s.n_bind && !bind) return pkf::refuse("the statement binds elements: pass them");
    if (!pkf::elements_below_p(bind, s.n_bind, "bind", why)) return pkf::refuse(why);
    try {
        pkv::Statement st;
        if (int rc = pk::parse_pattern(st, io_pattern_or_null, io_pattern_len, pkf::io_pattern(s), pkf::g_error)) return rc;
        const pkf_statement side[2] = {pkf::side_f(s), pkf::side_t(s)};
        const pk::TwoSides sides(pkf::proof_bytes(side[0]), pkf::proof_bytes(side[1]), side_out, layer_out, result);
        if (!sides.framed(len)) return PK_OK;
        fe alpha, seeds[2];
        if (!pk::squeeze_outer(st, bind, s.n_bind, {{1, &alpha}, {2, seeds}}, result)) return PK_OK;
        Sum out[2];
        if (int rc = sides.each([&](int which, unsigned& layer) {
                pkv::Statement inner;
                if (int r = pk::parse_pattern(inner, nullptr, 0, pkf::io_pattern(side[which]), pkf::g_error)) return r;
                return verify_sum(side[which], inner, (const uint64_t*)seeds[which].v, nullptr, proof + sides.at[which], out[which], layer, result);
            }))
            return rc;
        if (!result->accepted) return PK_OK;
        if (!pkf::same_fraction(out[0].P, out[0].Q, out[1].P, out[1].Q))
            return verdict(result, PKF_CHECK_FRACTION, sides.at[1] + pkf::TOP_BYTES, "the two sides' fractions differ"), PK_OK;
        sides.accept();
        if (claims_out) {
            memset(claims_out, 0, sizeof *claims_out);
            pkf::put_fe(claims_out->alpha, alpha);
            memcpy(claims_out->z_f, out[0].point, 32 * (size_t)s.n);
            memcpy(claims_out->z_t, out[1].point, 32 * (size_t)s.k);
            pkf::put_fe(claims_out->f_value, pk::h_sub(alpha, out[0].value_q));
            pkf::put_fe(claims_out->t_value, pk::h_sub(alpha, out[1].value_q));
            pkf::put_fe(claims_out->m_value, out[1].value_p);
        }
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

}  // extern "C"
