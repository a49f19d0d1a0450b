// verify_host.cpp -- the host half of libprovekit_lookup.so's C ABI: the statement's rule, the outer IO pattern and the verifier.  No
// device code and no HIP call; of other libraries it calls pks_proof_bytes and pks_verify (provekit_sumcheck.h).  This file and its
// headers are also what the sanitizer build (make asan, lookup/asan_main.cpp) compiles, next to the sumcheck library's host verifier.
#include <vector>

#include "layout.hpp"

namespace pkl {
thread_local std::string g_error;
}

namespace {

using pk::fe;

void verdict(pkv_result* r, int* side_out, int side, int check, uint64_t offset, const std::string& msg) {
    pkv::Verdict v;
    v.failed = check != PKV_CHECK_NONE, v.check = check, v.offset = offset, v.message = msg;
    pkv::to_result(v, r);
    if (side_out) *side_out = side;
}

}  // namespace

extern "C" {

int pkl_abi_version(void) { return 1; }

const char* pkl_create_error(void) { return pkl::g_error.c_str(); }

int pkl_io_pattern(const pkl_statement* stmt, uint8_t* buf, size_t cap, size_t* len) {
    std::string why;
    if (!len) return pkl::refuse("null pointer");
    if (!pkl::statement_ok(stmt, why)) return pkl::refuse(why);
    try {
        return pk::pattern_out(pkl::io_pattern(*stmt), buf, cap, len);
    } catch (...) {
        return PK_ERR_OOM;
    }
}

int pkl_proof_bytes(const pkl_statement* stmt, size_t* len) {
    std::string why;
    if (!len) return pkl::refuse("null pointer");
    if (!pkl::statement_ok(stmt, why)) return pkl::refuse(why);
    pkl::Framing fr;
    if (int rc = pkl::framing(*stmt, fr)) return pkl::g_error = pks_create_error(), rc;
    *len = fr.total;
    return PK_OK;
}

unsigned pkl_count_lds_max_k(void) { return pkl::COUNT_LDS_MAX_K; }
unsigned pkl_gather_lds_max_k(void) { return pkl::GATHER_LDS_MAX_K; }

int pkl_verify(const pkl_statement* stmt, const uint8_t* io_pattern_or_null, size_t io_pattern_len, const uint64_t* bind, const uint64_t* bind2,
               const uint8_t* proof, size_t len, pkl_claims* claims_out, int* side_out, pkv_result* result) {
    std::string why;
    if (!result || (!proof && len)) return pkl::refuse("null pointer");
    if (!pkl::statement_ok(stmt, why)) return pkl::refuse(why);
    const pkl_statement& s = *stmt;
    if (s.n_bind && !bind) return pkl::refuse("the statement binds elements: pass them");
    if (s.n_bind2 && !bind2) return pkl::refuse("the statement binds elements after the helper tables: pass them");
    if (!pk::elements_below_p(bind, s.n_bind, "bind", why) || !pk::elements_below_p(bind2, s.n_bind2, "bind2", why)) return pkl::refuse(why);
    try {
        pkv::Statement st;
        if (int rc = pk::parse_pattern(st, io_pattern_or_null, io_pattern_len, pkl::io_pattern(s), pkl::g_error)) return rc;
        pkl::Framing fr;
        if (int rc = pkl::framing(s, fr)) return pkl::g_error = pks_create_error(), rc;
        // framing first: the three parts have fixed lengths, so a proof of another length is judged before any part is read
        if (len < fr.total) return verdict(result, side_out, PKL_SIDE_OUTER, PKV_CHECK_TRANSCRIPT_SHORT, len, "the proof is shorter than its three parts"), PK_OK;
        if (len > fr.total) return verdict(result, side_out, PKL_SIDE_OUTER, PKV_CHECK_TRAILING_BYTES, fr.total, "bytes left after the proof"), PK_OK;

        // the outer transcript reads one string: bind | bind2 | s
        std::vector<uint8_t> bytes;
        pk::put_canonical(bytes, bind, s.n_bind);
        pk::put_canonical(bytes, bind2, s.n_bind2);
        const size_t prefix = bytes.size();
        bytes.insert(bytes.end(), proof, proof + 32);

        pkv::Verdict v;
        pkv::Arthur A(st, bytes.data(), bytes.size(), v);
        std::vector<fe> scratch(PKL_MAX_BIND), tau_f(s.n), tau_t(s.k);
        fe alpha, sum, seed;
        auto walk = [&]() -> bool {
            if (s.n_bind && !A.next_scalars(s.n_bind, scratch.data())) return false;
            if (!A.challenge_scalars(1, &alpha)) return false;
            if (s.n_bind2 && !A.next_scalars(s.n_bind2, scratch.data())) return false;
            if (!A.next_scalars(1, &sum)) return false;
            if (!A.challenge_scalars(s.n, tau_f.data()) || !A.challenge_scalars(s.k, tau_t.data()) || !A.challenge_scalars(1, &seed)) return false;
            if (!A.done()) return A.fail(PKV_CHECK_IO_PATTERN, "declared operations left after the outer transcript");
            return true;
        };
        if (!walk()) {
            if (!v.failed) A.fail(PKV_CHECK_TRANSCRIPT_SHORT, "the walk stopped without a verdict");
            v.offset = v.offset > prefix ? v.offset - prefix : 0;
            pkv::to_result(v, result);
            if (side_out) *side_out = PKL_SIDE_OUTER;
            return PK_OK;
        }

        fe r_f[PKL_MAX_VARS], r_t[PKL_MAX_VARS], finals_f[2], finals_t[3];
        for (int side = PKL_SIDE_F; side <= PKL_SIDE_T; side++) {
            const pks_statement ps = pkl::side_statement(s, side);
            const fe expected = pkl::side_expected_sum(side);
            const bool is_f = side == PKL_SIDE_F;
            const size_t at = is_f ? fr.f_at : fr.t_at;
            const int rc = pks_verify(&ps, nullptr, 0, (const uint64_t*)(is_f ? tau_f.data() : tau_t.data()), (const uint64_t*)seed.v, (const uint64_t*)expected.v,
                                      proof + at, is_f ? fr.f_len : fr.t_len, (uint64_t*)(is_f ? r_f : r_t), (uint64_t*)(is_f ? finals_f : finals_t), result);
            if (rc) return pkl::g_error = pks_create_error(), rc;
            result->offset += at;
            if (side_out) *side_out = side;
            if (!result->accepted) return PK_OK;
        }
        if (side_out) *side_out = PKL_SIDE_OUTER;  // accepted: no part to point at
        if (claims_out) pkl::derive_claims(s, alpha, sum, r_f, r_t, finals_f, finals_t, claims_out);
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

}  // extern "C"
