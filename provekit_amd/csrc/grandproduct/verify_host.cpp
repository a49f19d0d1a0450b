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

using pk::verdict;

struct Product {
    fe product, value;
    fe point[PKG_MAX_VARS];
};

// What the verifier adds to the chain's rule (pkg::Chain, statement.hpp): the product of the top values, which must be the expected
// one where one is given.  A layer's finals have no check beyond its sumcheck's own.
struct Verifying : pkg::Chain {
    const fe* wanted;  // or NULL
    fe product;
    Verifying(const pkg_statement& st, const fe* expected_or_null) : Chain(st), wanted(expected_or_null) {}
    bool check_top(const fe* top, pkv_result* result) {
        product = pk::h_mul(top[0], top[1]);
        if (wanted && !pk::fe_eq(product, *wanted)) return verdict(result, PKG_CHECK_PRODUCT, 64, "the product of the top values is not the expected one"), false;
        return true;
    }
    bool check_finals(unsigned, const fe*, const fe*, pkv_result*) const { return true; }
};

// One grand-product proof of exactly pkg::proof_bytes(s) bytes against a parsed pattern: gkr/chain.hpp's walk.  PK_OK: the verdict is
// in *result, its offset in bytes of this proof, `layer` what it is about; accepted: `out` is written.
int verify_product(const pkg_statement& s, const pkv::Statement& st, const uint64_t* bind, const fe* expected, const uint8_t* proof, Product& out,
                   unsigned& layer, pkv_result* result) {
    Verifying rule(s, expected);
    if (int rc = pk::gkr::verify_chain(rule, st, bind, proof, out.point, layer, result, pkg::g_error)) return rc;
    if (result->accepted) out.product = rule.product, out.value = rule.claim;
    return PK_OK;
}

}  // namespace

extern "C" {

int pkg_abi_version(void) { return 1; }

const char* pkg_check_name(int check) { return check == PKG_CHECK_PRODUCT ? "PRODUCT" : pks_check_name(check); }

const char* pkg_create_error(void) { return pkg::g_error.c_str(); }

int pkg_io_pattern(const pkg_statement* stmt, uint8_t* buf, size_t cap, size_t* len) { return pk::pattern_out<pkg::Lib>(stmt, buf, cap, len); }
int pkg_proof_bytes(const pkg_statement* stmt, size_t* len) { return pk::size_out<pkg::Lib>(stmt, len, [](auto& s) { return pkg::proof_bytes(s); }); }
int pkg_multiset_io_pattern(const pkg_multiset_statement* stmt, uint8_t* buf, size_t cap, size_t* len) { return pk::pattern_out<pkg::Lib>(stmt, buf, cap, len); }
int pkg_multiset_proof_bytes(const pkg_multiset_statement* stmt, size_t* len) { return pk::size_out<pkg::Lib>(stmt, len, [](auto& s) { return pkg::proof_bytes(s); }); }

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
        const pkg_statement side = pkg::side_statement(s);
        const size_t half = pkg::proof_bytes(side);
        const pk::TwoSides sides(half, half, side_out, layer_out, result);
        if (!sides.framed(len)) return PK_OK;
        fe gamma, beta = pk::fe_one(), seeds[2];
        if (!pk::squeeze_outer(st, bind, s.n_bind, {{1, &gamma}, {s.w > 1, &beta}, {2, seeds}}, result)) return PK_OK;
        pkv::Statement inner;
        if (int rc = pk::parse_pattern(inner, nullptr, 0, pkg::io_pattern(side), pkg::g_error)) return rc;
        Product out[2];
        if (int rc = sides.each([&](int which, unsigned& layer) {
                return verify_product(side, inner, (const uint64_t*)seeds[which].v, nullptr, proof + sides.at[which], out[which], layer, result);
            }))
            return rc;
        if (!result->accepted) return PK_OK;
        if (!pk::fe_eq(out[0].product, out[1].product)) return verdict(result, PKG_CHECK_PRODUCT, half + 64, "the two sides' products differ"), PK_OK;
        sides.accept();
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
