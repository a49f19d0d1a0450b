// verify_host.cpp -- the host half of libprovekit_memcheck.so's C ABI: the statement's rules, the outer IO pattern, the verifier with
// its four checks and the claims' four combinations.  No device code and no HIP call; of other libraries it calls pkf_verify,
// pkf_lookup_verify, the two lengths, pkf_check_name and pkf_create_error (provekit_fracsum.h).  This file and its headers are also what
// the sanitizer build (make asan, memcheck/asan_main.cpp) compiles, next to the fractional-sum and sumcheck libraries' host verifiers.
#include <vector>

#include "statement.hpp"

namespace pkm {
thread_local std::string g_error;
}

namespace {

using pk::fe;

using pk::verdict;

// the three parts' lengths; a pkf refusal of a statement this library made is passed on with its reason
int side_bytes(const pkm_statement& s, size_t out[3]) {
    for (int side = PKM_SIDE_OPS; side <= PKM_SIDE_MEM; side++) {
        const pkf_statement sum = pkm::side_sum(s, side);
        if (int rc = pkf_proof_bytes(&sum, &out[side])) return pkm::g_error = pkf_create_error(), rc;
    }
    const pkf_lookup_statement time = pkm::side_time(s);
    if (int rc = pkf_lookup_proof_bytes(&time, &out[PKM_SIDE_TIME])) return pkm::g_error = pkf_create_error(), rc;
    return PK_OK;
}

}  // namespace

extern "C" {

int pkm_abi_version(void) { return 1; }

const char* pkm_check_name(int check) {
    return check == PKM_CHECK_SIGN ? "SIGN" : check == PKM_CHECK_BALANCE ? "BALANCE" : check == PKM_CHECK_TIME_TABLE ? "TIME_TABLE" : pkf_check_name(check);
}

const char* pkm_create_error(void) { return pkm::g_error.c_str(); }

int pkm_io_pattern(const pkm_statement* stmt, uint8_t* buf, size_t cap, size_t* len) { return pk::pattern_out<pkm::Lib>(stmt, buf, cap, len); }

int pkm_proof_bytes(const pkm_statement* stmt, size_t* len) {
    std::string why;
    if (!len) return pkm::refuse("null pointer");
    if (!pkm::statement_ok(stmt, why)) return pkm::refuse(why);
    size_t part[3];
    if (int rc = side_bytes(*stmt, part)) return rc;
    *len = part[0] + part[1] + part[2];
    return PK_OK;
}

int pkm_verify(const pkm_statement* stmt, const uint8_t* io_pattern_or_null, size_t io_pattern_len, const uint64_t* bind, const uint8_t* proof, size_t len,
               pkm_claims* claims_out, int* side_out, unsigned* layer_out, pkv_result* result) {
    std::string why;
    if (!result || (!proof && len)) return pkm::refuse("null pointer");
    if (!pkm::statement_ok(stmt, why)) return pkm::refuse(why);
    const pkm_statement& s = *stmt;
    if (s.n_bind && !bind) return pkm::refuse("the statement binds elements: pass them");
    if (!pkm::elements_below_p(bind, s.n_bind, "bind", why)) return pkm::refuse(why);
    try {
        pkv::Statement st;
        if (int rc = pk::parse_pattern(st, io_pattern_or_null, io_pattern_len, pkm::io_pattern(s), pkm::g_error)) return rc;
        size_t part[3];
        if (int rc = side_bytes(s, part)) return rc;
        const size_t at[3] = {0, part[0], part[0] + part[1]}, total = at[2] + part[2];
        // where a verdict points: the side and the layer it is about
        auto about = [&](int side, unsigned layer) {
            if (side_out) *side_out = side;
            if (layer_out) *layer_out = layer;
        };
        about(PKM_SIDE_OPS, 0);
        // framing first: all three parts have a fixed length, so a proof of another length is judged before any part is read
        if (len < total) return verdict(result, PKV_CHECK_TRANSCRIPT_SHORT, len, "the proof is shorter than its three parts"), PK_OK;
        if (len > total) return verdict(result, PKV_CHECK_TRAILING_BYTES, total, "bytes left after the proof"), PK_OK;
        pkm::Challenges ch;
        if (!pk::squeeze_outer(st, bind, s.n_bind, {{1, &ch.gamma}, {1, &ch.beta}, {3, ch.seeds}}, result)) return PK_OK;
        fe frac[2][2], z[2][PKF_MAX_VARS], cq[2], cp[2];
        for (int side = PKM_SIDE_OPS; side <= PKM_SIDE_MEM; side++) {
            const pkf_statement sum = pkm::side_sum(s, side);
            unsigned layer = 0;
            if (int rc = pkf_verify(&sum, nullptr, 0, (const uint64_t*)ch.seeds[side].v, nullptr, proof + at[side], part[side], (uint64_t*)frac[side], (uint64_t*)z[side],
                                    (uint64_t*)cp[side].v, (uint64_t*)cq[side].v, &layer, result))
                return pkm::g_error = pkf_create_error(), rc;
            result->offset += at[side];
            about(side, layer);
            if (!result->accepted) return PK_OK;
            about(side, 0);
            if (!pk::fe_eq(cp[side], pkm::sign_at(z[side][0])))
                return verdict(result, PKM_CHECK_SIGN, at[side] + part[side], "the numerator claim is not the sign table's value 1 - 2 z_0 at the side's point"), PK_OK;
        }
        if (!pkm::balanced(frac[0][0], frac[0][1], frac[1][0], frac[1][1]))
            return verdict(result, PKM_CHECK_BALANCE, at[PKM_SIDE_MEM] + 128, "the two sides' fractions do not cancel: the multisets differ"), PK_OK;
        const pkf_lookup_statement time = pkm::side_time(s);
        pkf_lookup_claims seen;
        unsigned layer = 0;
        if (int rc = pkf_lookup_verify(&time, nullptr, 0, (const uint64_t*)ch.seeds[PKM_SIDE_TIME].v, proof + at[PKM_SIDE_TIME], part[PKM_SIDE_TIME], &seen, nullptr, &layer,
                                       result))
            return pkm::g_error = pkf_create_error(), rc;
        result->offset += at[PKM_SIDE_TIME];
        about(PKM_SIDE_TIME, layer);
        if (!result->accepted) return PK_OK;
        about(PKM_SIDE_TIME, 0);
        fe z_t[PKM_MAX_VARS];
        for (unsigned i = 0; i < s.n; i++) z_t[i] = pk::h_load(seen.z_t[i]);
        if (!pk::fe_eq(pk::h_load(seen.t_value), pkm::index_at(z_t, s.n)))
            return verdict(result, PKM_CHECK_TIME_TABLE, total, "the time side's table claim is not I(z_T): its table is not 0 .. 2^n - 1"), PK_OK;
        verdict(result, PKV_CHECK_NONE, total, "");
        about(PKM_SIDE_OPS, 0);
        if (claims_out) pkm::fill_claims(s, ch, z[0], cq[0], z[1], cq[1], seen, claims_out);
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

int pkm_check_claims(const pkm_statement* stmt, const pkm_claims* claims, const uint64_t* ops_evals, const uint64_t* mem_evals, const uint64_t* rt_eval,
                     const uint64_t* m_eval, int* which_out) {
    std::string why;
    if (!claims || !ops_evals || !mem_evals || !rt_eval || !m_eval || !which_out) return pkm::refuse("null pointer");
    if (!pkm::statement_ok(stmt, why)) return pkm::refuse(why);
    if (!pkm::elements_below_p(ops_evals, 4, "ops_evals", why) || !pkm::elements_below_p(mem_evals, 3, "mem_evals", why) ||
        !pkm::elements_below_p(rt_eval, 1, "rt_eval", why) || !pkm::elements_below_p(m_eval, 1, "m_eval", why) ||
        !pkm::elements_below_p(&claims->gamma[0], sizeof *claims / 32, "claims", why))
        return pkm::refuse(why);
    fe sum_ops = pk::fe_zero(), sum_mem = pk::fe_zero();
    for (unsigned j = 0; j < 4; j++) sum_ops = pk::h_add(sum_ops, pk::h_mul(pk::h_load(claims->ops_coeff[j]), pk::h_load(ops_evals + 4 * j)));
    for (unsigned j = 0; j < 3; j++) sum_mem = pk::h_add(sum_mem, pk::h_mul(pk::h_load(claims->mem_coeff[j]), pk::h_load(mem_evals + 4 * j)));
    *which_out = !pk::fe_eq(sum_ops, pk::h_load(claims->ops_value))                 ? PKM_CLAIM_OPS
                 : !pk::fe_eq(sum_mem, pk::h_load(claims->mem_value))               ? PKM_CLAIM_MEM
                 : !pk::fe_eq(pk::h_load(rt_eval), pk::h_load(claims->rt_value))    ? PKM_CLAIM_RT
                 : !pk::fe_eq(pk::h_load(m_eval), pk::h_load(claims->m_value))      ? PKM_CLAIM_M
                                                                                    : PKM_CLAIM_NONE;
    return PK_OK;
}

}  // extern "C"
