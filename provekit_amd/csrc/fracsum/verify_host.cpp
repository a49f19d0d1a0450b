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

void verdict(pkv_result* r, int check, uint64_t offset, const std::string& msg) {
    pkv::Verdict v;
    v.failed = check != PKV_CHECK_NONE, v.check = check, v.offset = offset, v.message = msg;
    pkv::to_result(v, r);
}

using pk::put_canonical;

struct Sum {
    fe P, Q, value_p, value_q;
    fe point[PKF_MAX_VARS];
};

// One fractional-sum proof of exactly pkf::proof_bytes(s) bytes against a parsed pattern.  expected: (num, den) or NULL.  PK_OK: the
// verdict is in *result, its offset in bytes of this proof, `layer` what it is about; accepted: `out` is written.
int verify_sum(const pkf_statement& s, const pkv::Statement& st, const uint64_t* bind, const fe* expected, const uint8_t* proof, Sum& out, unsigned& layer,
               pkv_result* result) {
    const unsigned n = s.n;
    layer = 0;
    // the outer transcript reads one string: bind | top | the finals of every layer, which sit at the end of that layer's proof
    std::vector<uint8_t> bytes;
    bytes.reserve(32 * ((size_t)s.n_bind + 4 * n));
    put_canonical(bytes, bind, s.n_bind);
    const size_t prefix = bytes.size();
    bytes.insert(bytes.end(), proof, proof + pkf::TOP_BYTES);
    for (unsigned d = 1; d < n; d++) {
        const size_t end = pkf::layer_at(s, d + 1);
        bytes.insert(bytes.end(), proof + end - 32 * (size_t)pkf::layer_tables(s, d), proof + end);
    }

    pkv::Verdict v;
    pkv::Arthur A(st, bytes.data(), bytes.size(), v);
    // an outer failure: inside top its own place, later the end of the layer whose finals were being absorbed
    auto outer_failed = [&](size_t proof_at) {
        if (!v.failed) A.fail(PKV_CHECK_TRANSCRIPT_SHORT, "the walk stopped without a verdict");
        v.offset = v.offset > prefix && v.offset <= prefix + pkf::TOP_BYTES ? v.offset - prefix : proof_at;
        pkv::to_result(v, result);
        layer = 0;
        return PK_OK;
    };
    fe scratch[PKF_MAX_BIND], top[4], rho, lambda, seed, finals[4];
    if ((s.n_bind && !A.next_scalars(s.n_bind, scratch)) || !A.next_scalars(4, top)) return outer_failed(0);
    fe P, Q;
    pkf::fraction_of(top, P, Q);
    if (pk::fe_eq(Q, pk::fe_zero())) return verdict(result, PKF_CHECK_DENOMINATOR, pkf::TOP_BYTES, "Q = 0: a denominator is zero"), PK_OK;
    if (s.unit && n == 1 && !(pk::fe_eq(top[0], pk::fe_one()) && pk::fe_eq(top[1], pk::fe_one())))
        return verdict(result, PKF_CHECK_UNIT, pkf::TOP_BYTES, "a top numerator of a unit statement is not 1"), PK_OK;
    if (expected && !pkf::same_fraction(P, Q, expected[0], expected[1]))
        return verdict(result, PKF_CHECK_FRACTION, pkf::TOP_BYTES, "the fraction of the top values is not the expected one"), PK_OK;
    if (!A.challenge_scalars(1, &rho)) return outer_failed(pkf::TOP_BYTES);
    fe z[PKF_MAX_VARS], r[PKF_MAX_VARS];
    pkf::Claims claim;
    claim.from_top(top, rho);
    claim.has_p = !(s.unit && n == 1);
    z[0] = rho;
    for (unsigned d = 1; d < n; d++) {
        const size_t at = pkf::layer_at(s, d), end = at + pkf::layer_bytes(s, d);
        if (!A.challenge_scalars(1, &lambda) || !A.challenge_scalars(1, &seed)) return outer_failed(at);
        const pks_statement ps = pkf::layer_statement(s, d);
        const fe sum = claim.expected(lambda);
        const int rc = pks_verify(&ps, nullptr, 0, (const uint64_t*)z, (const uint64_t*)seed.v, (const uint64_t*)sum.v, proof + at, pkf::layer_bytes(s, d),
                                  (uint64_t*)r, (uint64_t*)finals, result);
        if (rc) return pkf::g_error = pks_create_error(), rc;
        result->offset += at;
        layer = d;
        if (!result->accepted) return PK_OK;
        const bool unit_leaves = pkf::unit_layer(s, d);
        if (unit_leaves && !pkf::unit_final_ok(finals, lambda))
            return verdict(result, PKF_CHECK_UNIT, end, "layer " + std::to_string(d) + ": the final value of u is not 1 + lambda qR"), PK_OK;
        layer = 0;
        fe again[4];  // the same bytes pks_verify took: canonical
        if (!A.next_scalars(ps.m, again) || !A.challenge_scalars(1, &rho)) return outer_failed(end);
        claim.step(unit_leaves, finals, lambda, rho);
        for (unsigned i = 0; i < d; i++) z[i + 1] = r[i];
        z[0] = rho;
    }
    if (!A.done()) {
        A.fail(PKV_CHECK_IO_PATTERN, "declared operations left after the outer transcript");
        return outer_failed(pkf::layer_at(s, n));
    }
    verdict(result, PKV_CHECK_NONE, pkf::layer_at(s, n), "");
    out.P = P, out.Q = Q, out.value_p = claim.has_p ? claim.cp : pk::fe_one(), out.value_q = claim.cq;
    for (unsigned i = 0; i < n; i++) out.point[i] = z[i];
    return PK_OK;
}

template <class S>
int pattern_out(const S* stmt, uint8_t* buf, size_t cap, size_t* len) {
    std::string why;
    if (!len) return pkf::refuse("null pointer");
    if (!pkf::statement_ok(stmt, why)) return pkf::refuse(why);
    try {
        return pk::pattern_out(pkf::io_pattern(*stmt), buf, cap, len);
    } catch (...) {
        return PK_ERR_OOM;
    }
}
template <class S>
int bytes_out(const S* stmt, size_t* len) {
    std::string why;
    if (!len) return pkf::refuse("null pointer");
    if (!pkf::statement_ok(stmt, why)) return pkf::refuse(why);
    *len = pkf::proof_bytes(*stmt);
    return PK_OK;
}

}  // namespace

extern "C" {

int pkf_abi_version(void) { return 1; }

const char* pkf_check_name(int check) {
    return check == PKF_CHECK_FRACTION ? "FRACTION" : check == PKF_CHECK_DENOMINATOR ? "DENOMINATOR" : check == PKF_CHECK_UNIT ? "UNIT" : pks_check_name(check);
}

const char* pkf_create_error(void) { return pkf::g_error.c_str(); }

int pkf_io_pattern(const pkf_statement* stmt, uint8_t* buf, size_t cap, size_t* len) { return pattern_out(stmt, buf, cap, len); }
int pkf_proof_bytes(const pkf_statement* stmt, size_t* len) { return bytes_out(stmt, len); }
int pkf_lookup_io_pattern(const pkf_lookup_statement* stmt, uint8_t* buf, size_t cap, size_t* len) { return pattern_out(stmt, buf, cap, len); }
int pkf_lookup_proof_bytes(const pkf_lookup_statement* stmt, size_t* len) { return bytes_out(stmt, len); }

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
        if (layer_out) *layer_out = 0;
        if (side_out) *side_out = PKF_SIDE_F;
        const pkf_statement sides[2] = {pkf::side_f(s), pkf::side_t(s)};
        const size_t at[2] = {0, pkf::proof_bytes(sides[0])}, total = pkf::proof_bytes(s);
        if (len < total) return verdict(result, PKV_CHECK_TRANSCRIPT_SHORT, len, "the proof is shorter than its two parts"), PK_OK;
        if (len > total) return verdict(result, PKV_CHECK_TRAILING_BYTES, total, "bytes left after the proof"), PK_OK;

        // the outer transcript absorbs nothing of the proof
        std::vector<uint8_t> bytes;
        put_canonical(bytes, bind, s.n_bind);
        pkv::Verdict v;
        pkv::Arthur A(st, bytes.data(), bytes.size(), v);
        fe scratch[PKF_MAX_BIND], alpha, seeds[2];
        const bool walked = (!s.n_bind || A.next_scalars(s.n_bind, scratch)) && A.challenge_scalars(1, &alpha) && A.challenge_scalars(2, seeds) &&
                            (A.done() || A.fail(PKV_CHECK_IO_PATTERN, "declared operations left after the outer transcript"));
        if (!walked) {
            v.offset = 0;
            pkv::to_result(v, result);
            return PK_OK;
        }
        Sum out[2];
        for (int which = PKF_SIDE_F; which <= PKF_SIDE_T; which++) {
            pkv::Statement inner;
            if (int rc = pk::parse_pattern(inner, nullptr, 0, pkf::io_pattern(sides[which]), pkf::g_error)) return rc;
            unsigned layer = 0;
            if (int rc = verify_sum(sides[which], inner, (const uint64_t*)seeds[which].v, nullptr, proof + at[which], out[which], layer, result)) return rc;
            result->offset += at[which];
            if (side_out) *side_out = which;
            if (layer_out) *layer_out = layer;
            if (!result->accepted) return PK_OK;
        }
        if (!pkf::same_fraction(out[0].P, out[0].Q, out[1].P, out[1].Q))
            return verdict(result, PKF_CHECK_FRACTION, at[1] + pkf::TOP_BYTES, "the two sides' fractions differ"), PK_OK;
        verdict(result, PKV_CHECK_NONE, total, "");
        if (side_out) *side_out = PKF_SIDE_F;  // accepted: no part to point at
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
