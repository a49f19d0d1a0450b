// verify_host.cpp -- the host half of libprovekit_sumcheck.so's C ABI: the statement's rule, the IO pattern and the verifier, for
// pks_* and for the wide statements' pksw_* (one walk, verify_walk, over either statement).  No device code, no HIP call and no call of
// the product library: this file and its headers are also what the sanitizer build (make asan, asan_main.cpp) compiles.
#include "layout.hpp"

namespace pks {
thread_local std::string g_error;
thread_local std::string g_wide_error;
}

namespace {

const char* const kOwnCheckNames[PKS_CHECK_COUNT - PKV_CHECK_COUNT] = {"ROUND", "FINAL", "SUM"};
// the verifier core's names, restated: this library does not link libprovekit_verify.so
const char* const kCoreCheckNames[PKV_CHECK_COUNT] = {
    "NONE",          "TRANSCRIPT_SHORT", "NON_CANONICAL", "IO_PATTERN", "HINT_FORMAT", "OPENING_COUNT",   "MERKLE",         "ZK_SUMCHECK", "WHIR_SUMCHECK",
    "POW",           "STIR_INDICES",     "FINAL_POLY",    "WHIR_FINAL", "BLINDING_WEIGHT", "TRAILING_BYTES", "SPARTAN", "WITNESS_FIT", "MATRIX_EVAL"};

using pk::fe;

// the statement's public part as the transcript sees it: bind, tau, the coefficients, canonical.  false: an element is not below p
template <class S>
bool public_prefix(const S& st, const uint64_t* tau, const uint64_t* bind, std::vector<uint8_t>& out, std::string& why) {
    auto put = [&](const uint64_t* v, size_t n, const char* what) { return pk::elements_below_p(v, n, what, why) && (pk::put_canonical(out, v, n), true); };
    return put(bind, st.n_bind, "bind") && put(tau, st.has_tau ? st.n : 0, "tau") && put(&st.coeffs[0][0], st.T, "coefficient");
}

// pks_verify and pksw_verify after the statement's own check: the walk is written once, over either statement (statement.hpp and
// wide_statement.hpp give degree, io_pattern, public_elems and terms_at for both).  A refusal's reason goes to `slot`
template <class S>
int verify_walk(const S& s, std::string& slot, const uint8_t* io_pattern_or_null, size_t io_pattern_len, const uint64_t* tau_or_null, const uint64_t* bind,
                const uint64_t* expected_sum_or_null, const uint8_t* proof, size_t len, uint64_t* point_out, uint64_t* finals_out, pkv_result* result) {
    std::string why;
    if (s.has_tau && !tau_or_null) return pk::refuse(slot, "the statement has a tau: pass it");
    if (!s.has_tau && tau_or_null) return pk::refuse(slot, "the statement has no tau: pass NULL");
    if (s.n_bind && !bind) return pk::refuse(slot, "the statement binds elements: pass them");
    try {
        pkv::Statement st;
        if (int rc = pk::parse_pattern(st, io_pattern_or_null, io_pattern_len, pks::io_pattern(s), slot)) return rc;
        // both sides absorb the public part first: it goes in front of the proof, and the transcript reads one string
        std::vector<uint8_t> bytes;
        bytes.reserve(32 * pks::public_elems(s) + len);
        if (!public_prefix(s, tau_or_null, bind, bytes, why)) return pk::refuse(slot, why);
        const size_t prefix = bytes.size();
        bytes.insert(bytes.end(), proof, proof + len);

        pkv::Verdict v;
        pkv::Arthur A(st, bytes.data(), bytes.size(), v);
        const unsigned D = pks::degree(s);
        std::vector<fe> pub(pks::public_elems(s)), point(s.n), finals(s.m);
        const fe* tau = pub.data() + s.n_bind;
        auto walk = [&]() -> bool {
            if (!A.next_scalars(pub.size(), pub.data())) return false;
            fe claim;
            if (!A.next_scalars(1, &claim)) return false;
            if (expected_sum_or_null && !pk::fe_eq(claim, pk::h_load(expected_sum_or_null)))
                return A.fail(PKS_CHECK_SUM, "the proof's sum is not the expected one");
            fe e = pk::fe_one();
            for (unsigned i = 0; i < s.n; i++) {
                fe h[pks::MAX_ROUND_VALUES];
                if (!A.next_scalars(D + 1, h)) return false;
                fe lhs;
                if (s.has_tau)  // e_i ((1 - tau_i) h(0) + tau_i h(1))
                    lhs = pk::h_mul(e, pk::h_add(h[0], pk::h_mul(tau[i], pk::h_sub(h[1], h[0]))));
                else
                    lhs = pk::h_add(h[0], h[1]);
                if (!pk::fe_eq(lhs, claim)) return A.fail(PKS_CHECK_ROUND, "round " + std::to_string(i) + ": the values do not add up to the claim");
                if (!A.challenge_scalars(1, &point[i])) return false;
                claim = pks::round_poly_at(h, D, point[i]);
                if (s.has_tau) {
                    e = pk::h_mul(e, pks::eq1(tau[i], point[i]));
                    claim = pk::h_mul(e, claim);
                }
            }
            if (!A.next_scalars(s.m, finals.data())) return false;
            fe g = pks::terms_at(s, finals.data());
            if (s.has_tau) g = pk::h_mul(e, g);
            if (!pk::fe_eq(g, claim)) return A.fail(PKS_CHECK_FINAL, "the terms of the final values are not the last claim");
            if (!A.done()) return A.fail(PKV_CHECK_TRAILING_BYTES, "bytes or declared operations left after the proof");
            return true;
        };
        const bool ok = walk();
        if (!ok && !v.failed) A.fail(PKV_CHECK_TRANSCRIPT_SHORT, "the walk stopped without a verdict");
        if (!v.failed) v.offset = A.pos();
        v.offset = v.offset > prefix ? v.offset - prefix : 0;  // in bytes of the proof
        pkv::to_result(v, result);
        if (ok) {
            if (point_out) memcpy(point_out, point.data(), 32 * (size_t)s.n);
            if (finals_out) memcpy(finals_out, finals.data(), 32 * (size_t)s.m);
        }
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

}  // namespace

extern "C" {

int pks_abi_version(void) { return 1; }

const char* pks_check_name(int check) {
    if (check >= 0 && check < PKV_CHECK_COUNT) return kCoreCheckNames[check];
    return check >= PKV_CHECK_COUNT && check < PKS_CHECK_COUNT ? kOwnCheckNames[check - PKV_CHECK_COUNT] : "UNKNOWN";
}

const char* pks_create_error(void) { return pks::g_error.c_str(); }

int pks_io_pattern(const pks_statement* stmt, uint8_t* buf, size_t cap, size_t* len) {
    std::string why;
    if (!len) return pks::refuse("null pointer");
    if (!pks::statement_ok(stmt, why)) return pks::refuse(why);
    try {
        return pk::pattern_out(pks::io_pattern(*stmt), buf, cap, len);
    } catch (...) {
        return PK_ERR_OOM;
    }
}

int pks_proof_bytes(const pks_statement* stmt, size_t* len) {
    std::string why;
    if (!len) return pks::refuse("null pointer");
    if (!pks::statement_ok(stmt, why)) return pks::refuse(why);
    *len = 32 * pks::proof_elems(*stmt);
    return PK_OK;
}

int pks_verify(const pks_statement* stmt, const uint8_t* io_pattern_or_null, size_t io_pattern_len, const uint64_t* tau_or_null, const uint64_t* bind,
               const uint64_t* expected_sum_or_null, const uint8_t* proof, size_t len, uint64_t* point_out, uint64_t* finals_out, pkv_result* result) {
    std::string why;
    if (!result || (!proof && len)) return pks::refuse("null pointer");
    if (!pks::statement_ok(stmt, why)) return pks::refuse(why);
    return verify_walk(*stmt, pks::g_error, io_pattern_or_null, io_pattern_len, tau_or_null, bind, expected_sum_or_null, proof, len, point_out, finals_out, result);
}

// ---- the wide statements (include/provekit_sumcheck_wide.h) ----------------------------------------------------------------------

int pksw_abi_version(void) { return 1; }

const char* pksw_create_error(void) { return pks::g_wide_error.c_str(); }

int pksw_io_pattern(const pksw_statement* stmt, uint8_t* buf, size_t cap, size_t* len) {
    std::string why;
    if (!len) return pks::refuse_wide("null pointer");
    if (!pks::statement_ok(stmt, why)) return pks::refuse_wide(why);
    try {
        return pk::pattern_out(pks::io_pattern(*stmt), buf, cap, len);
    } catch (...) {
        return PK_ERR_OOM;
    }
}

int pksw_proof_bytes(const pksw_statement* stmt, size_t* len) {
    std::string why;
    if (!len) return pks::refuse_wide("null pointer");
    if (!pks::statement_ok(stmt, why)) return pks::refuse_wide(why);
    *len = 32 * pks::proof_elems(*stmt);
    return PK_OK;
}

int pksw_arena_bytes(const pksw_statement* stmt, size_t* len) {
    std::string why;
    if (!len) return pks::refuse_wide("null pointer");
    if (!pks::statement_ok(stmt, why)) return pks::refuse_wide(why);
    *len = 32 * pkss::layout(stmt->n, stmt->m, 0, pks::WIDE_SCRATCH_FES).total;
    return PK_OK;
}

int pksw_verify(const pksw_statement* stmt, const uint8_t* io_pattern_or_null, size_t io_pattern_len, const uint64_t* tau_or_null, const uint64_t* bind,
                const uint64_t* expected_sum_or_null, const uint8_t* proof, size_t len, uint64_t* point_out, uint64_t* finals_out, pkv_result* result) {
    std::string why;
    if (!result || (!proof && len)) return pks::refuse_wide("null pointer");
    if (!pks::statement_ok(stmt, why)) return pks::refuse_wide(why);
    return verify_walk(*stmt, pks::g_wide_error, io_pattern_or_null, io_pattern_len, tau_or_null, bind, expected_sum_or_null, proof, len, point_out, finals_out, result);
}

}  // extern "C"
