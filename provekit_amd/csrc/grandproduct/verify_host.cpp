// verify_host.cpp -- the host half of libprovekit_grandproduct.so's C ABI: the statements' rules, the two outer IO patterns and the
// two verifiers.  No device code and no HIP call; of other libraries it calls pks_verify and pks_check_name (provekit_sumcheck.h).
// This file and its headers are also what the sanitizer build (make asan, grandproduct/asan_main.cpp) compiles, next to the sumcheck
// library's host verifier.
#include <vector>

#include "layout.hpp"

namespace pkg {
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

struct Product {
    fe product, value;
    fe point[PKG_MAX_VARS];
};

// One grand-product proof of exactly pkg::proof_bytes(s) bytes against a parsed pattern.  PK_OK: the verdict is in *result, its
// offset in bytes of this proof, `layer` what it is about; accepted: `out` is written.
int verify_product(const pkg_statement& s, const pkv::Statement& st, const uint64_t* bind, const fe* expected, const uint8_t* proof, Product& out,
                   unsigned& layer, pkv_result* result) {
    const unsigned n = s.n;
    layer = 0;
    // the outer transcript reads one string: bind | top | the two finals of every layer, which sit at the end of that layer's proof
    std::vector<uint8_t> bytes;
    bytes.reserve(32 * ((size_t)s.n_bind + 2 * n));
    put_canonical(bytes, bind, s.n_bind);
    const size_t prefix = bytes.size();
    bytes.insert(bytes.end(), proof, proof + 64);
    for (unsigned d = 1; d < n; d++) bytes.insert(bytes.end(), proof + pkg::layer_at(d + 1) - 64, proof + pkg::layer_at(d + 1));

    pkv::Verdict v;
    pkv::Arthur A(st, bytes.data(), bytes.size(), v);
    // an outer failure: inside top its own place, later the end of the layer whose finals were being absorbed
    auto outer_failed = [&](size_t proof_at) {
        if (!v.failed) A.fail(PKV_CHECK_TRANSCRIPT_SHORT, "the walk stopped without a verdict");
        v.offset = v.offset > prefix && v.offset <= prefix + 64 ? v.offset - prefix : proof_at;
        pkv::to_result(v, result);
        layer = 0;
        return PK_OK;
    };
    fe scratch[PKG_MAX_BIND], top[2], rho, seed, lr[2];
    if ((s.n_bind && !A.next_scalars(s.n_bind, scratch)) || !A.next_scalars(2, top)) return outer_failed(0);
    const fe product = pk::h_mul(top[0], top[1]);
    if (expected && !pk::fe_eq(product, *expected)) return verdict(result, PKG_CHECK_PRODUCT, 64, "the product of the top values is not the expected one"), PK_OK;
    if (!A.challenge_scalars(1, &rho)) return outer_failed(64);
    fe z[PKG_MAX_VARS], r[PKG_MAX_VARS];
    fe claim = pkg::next_claim(top[0], top[1], rho);
    z[0] = rho;
    for (unsigned d = 1; d < n; d++) {
        const size_t at = pkg::layer_at(d);
        if (!A.challenge_scalars(1, &seed)) return outer_failed(at);
        const pks_statement ps = pkg::layer_statement(d);
        const int rc = pks_verify(&ps, nullptr, 0, (const uint64_t*)z, (const uint64_t*)seed.v, (const uint64_t*)claim.v, proof + at, pkg::layer_bytes(d),
                                  (uint64_t*)r, (uint64_t*)lr, result);
        if (rc) return pkg::g_error = pks_create_error(), rc;
        result->offset += at;
        layer = d;
        if (!result->accepted) return PK_OK;
        layer = 0;
        fe again[2];  // the same bytes pks_verify took: canonical
        if (!A.next_scalars(2, again) || !A.challenge_scalars(1, &rho)) return outer_failed(at + pkg::layer_bytes(d));
        claim = pkg::next_claim(lr[0], lr[1], rho);
        for (unsigned i = 0; i < d; i++) z[i + 1] = r[i];
        z[0] = rho;
    }
    if (!A.done()) {
        A.fail(PKV_CHECK_IO_PATTERN, "declared operations left after the outer transcript");
        return outer_failed(pkg::layer_at(n));
    }
    verdict(result, PKV_CHECK_NONE, pkg::layer_at(n), "");
    out.product = product, out.value = claim;
    for (unsigned i = 0; i < n; i++) out.point[i] = z[i];
    return PK_OK;
}

template <class S>
int pattern_out(const S* stmt, uint8_t* buf, size_t cap, size_t* len) {
    std::string why;
    if (!len) return pkg::refuse("null pointer");
    if (!pkg::statement_ok(stmt, why)) return pkg::refuse(why);
    try {
        return pk::pattern_out(pkg::io_pattern(*stmt), buf, cap, len);
    } catch (...) {
        return PK_ERR_OOM;
    }
}
template <class S>
int bytes_out(const S* stmt, size_t* len) {
    std::string why;
    if (!len) return pkg::refuse("null pointer");
    if (!pkg::statement_ok(stmt, why)) return pkg::refuse(why);
    *len = pkg::proof_bytes(*stmt);
    return PK_OK;
}

}  // namespace

extern "C" {

int pkg_abi_version(void) { return 1; }

const char* pkg_check_name(int check) { return check == PKG_CHECK_PRODUCT ? "PRODUCT" : pks_check_name(check); }

const char* pkg_create_error(void) { return pkg::g_error.c_str(); }

int pkg_io_pattern(const pkg_statement* stmt, uint8_t* buf, size_t cap, size_t* len) { return pattern_out(stmt, buf, cap, len); }
int pkg_proof_bytes(const pkg_statement* stmt, size_t* len) { return bytes_out(stmt, len); }
int pkg_multiset_io_pattern(const pkg_multiset_statement* stmt, uint8_t* buf, size_t cap, size_t* len) { return pattern_out(stmt, buf, cap, len); }
int pkg_multiset_proof_bytes(const pkg_multiset_statement* stmt, size_t* len) { return bytes_out(stmt, len); }

unsigned pkg_tail_max_n(void) { return pkg::TAIL_MAX_N; }

int pkg_verify(const pkg_statement* stmt, const uint8_t* io_pattern_or_null, size_t io_pattern_len, const uint64_t* bind, const uint64_t* expected_product_or_null,
               const uint8_t* proof, size_t len, uint64_t* product_out, uint64_t* point_out, uint64_t* value_out, unsigned* layer_out, pkv_result* result) {
    std::string why;
    if (!result || (!proof && len)) return pkg::refuse("null pointer");
    if (!pkg::statement_ok(stmt, why)) return pkg::refuse(why);
    const pkg_statement& s = *stmt;
    if (s.n_bind && !bind) return pkg::refuse("the statement binds elements: pass them");
    if (!pkg::elements_below_p(bind, s.n_bind, "bind", why)) return pkg::refuse(why);
    if (expected_product_or_null && !pkg::elements_below_p(expected_product_or_null, 1, "expected_product", why)) return pkg::refuse(why);
    try {
        pkv::Statement st;
        if (int rc = pk::parse_pattern(st, io_pattern_or_null, io_pattern_len, pkg::io_pattern(s), pkg::g_error)) return rc;
        if (layer_out) *layer_out = 0;
        // framing first: every part has a fixed length, so a proof of another length is judged before any part is read
        const size_t total = pkg::proof_bytes(s);
        if (len < total) return verdict(result, PKV_CHECK_TRANSCRIPT_SHORT, len, "the proof is shorter than its parts"), PK_OK;
        if (len > total) return verdict(result, PKV_CHECK_TRAILING_BYTES, total, "bytes left after the proof"), PK_OK;
        fe expected;
        if (expected_product_or_null) expected = pk::h_load(expected_product_or_null);
        Product out;
        unsigned layer = 0;
        if (int rc = verify_product(s, st, bind, expected_product_or_null ? &expected : nullptr, proof, out, layer, result)) return rc;
        if (layer_out) *layer_out = layer;
        if (!result->accepted) return PK_OK;
        if (product_out) pkg::put_fe(product_out, out.product);
        if (value_out) pkg::put_fe(value_out, out.value);
        if (point_out) memcpy(point_out, out.point, 32 * (size_t)s.n);
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

int pkg_multiset_verify(const pkg_multiset_statement* stmt, const uint8_t* io_pattern_or_null, size_t io_pattern_len, const uint64_t* bind, const uint8_t* proof,
                        size_t len, pkg_multiset_claims* claims_out, int* side_out, unsigned* layer_out, pkv_result* result) {
    std::string why;
    if (!result || (!proof && len)) return pkg::refuse("null pointer");
    if (!pkg::statement_ok(stmt, why)) return pkg::refuse(why);
    const pkg_multiset_statement& s = *stmt;
    if (s.n_bind && !bind) return pkg::refuse("the statement binds elements: pass them");
    if (!pkg::elements_below_p(bind, s.n_bind, "bind", why)) return pkg::refuse(why);
    try {
        pkv::Statement st;
        if (int rc = pk::parse_pattern(st, io_pattern_or_null, io_pattern_len, pkg::io_pattern(s), pkg::g_error)) return rc;
        if (layer_out) *layer_out = 0;
        if (side_out) *side_out = PKG_SIDE_A;
        const pkg_statement side = pkg::side_statement(s);
        const size_t half = pkg::proof_bytes(side), total = 2 * half;
        if (len < total) return verdict(result, PKV_CHECK_TRANSCRIPT_SHORT, len, "the proof is shorter than its two parts"), PK_OK;
        if (len > total) return verdict(result, PKV_CHECK_TRAILING_BYTES, total, "bytes left after the proof"), PK_OK;

        // the outer transcript absorbs nothing of the proof
        std::vector<uint8_t> bytes;
        put_canonical(bytes, bind, s.n_bind);
        pkv::Verdict v;
        pkv::Arthur A(st, bytes.data(), bytes.size(), v);
        fe scratch[PKG_MAX_BIND], gamma, beta = pk::fe_one(), seeds[2];
        const bool walked = (!s.n_bind || A.next_scalars(s.n_bind, scratch)) && A.challenge_scalars(1, &gamma) && (s.w == 1 || A.challenge_scalars(1, &beta)) &&
                            A.challenge_scalars(2, seeds) && (A.done() || A.fail(PKV_CHECK_IO_PATTERN, "declared operations left after the outer transcript"));
        if (!walked) {
            v.offset = 0;
            pkv::to_result(v, result);
            return PK_OK;
        }
        pkv::Statement inner;
        if (int rc = pk::parse_pattern(inner, nullptr, 0, pkg::io_pattern(side), pkg::g_error)) return rc;
        Product out[2];
        for (int which = PKG_SIDE_A; which <= PKG_SIDE_B; which++) {
            unsigned layer = 0;
            if (int rc = verify_product(side, inner, (const uint64_t*)seeds[which].v, nullptr, proof + which * half, out[which], layer, result)) return rc;
            result->offset += which * half;
            if (side_out) *side_out = which;
            if (layer_out) *layer_out = layer;
            if (!result->accepted) return PK_OK;
        }
        if (!pk::fe_eq(out[0].product, out[1].product)) return verdict(result, PKG_CHECK_PRODUCT, half + 64, "the two sides' products differ"), PK_OK;
        if (side_out) *side_out = PKG_SIDE_A;  // accepted: no part to point at
        if (claims_out) {
            memset(claims_out, 0, sizeof *claims_out);
            pkg::put_fe(claims_out->gamma, gamma);
            pkg::put_fe(claims_out->beta, beta);
            memcpy(claims_out->z_a, out[0].point, 32 * (size_t)s.n);
            memcpy(claims_out->z_b, out[1].point, 32 * (size_t)s.n);
            pkg::put_fe(claims_out->comb_a, pk::h_sub(gamma, out[0].value));
            pkg::put_fe(claims_out->comb_b, pk::h_sub(gamma, out[1].value));
        }
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

}  // extern "C"
