// verify_host.cpp -- the host half of libprovekit_bitwise.so's C ABI: the statement's rules and the plan, the outer IO pattern, the
// verifier with its table check and the five claims.  No device code and no HIP call; of other libraries it calls pkt_verify,
// pkt_proof_bytes, pkt_create_error and pkf_check_name.  This file and its headers are also what the sanitizer build (make asan,
// bitwise/asan_main.cpp) compiles, next to the three host verifiers below it.
#include <vector>

#include "layout.hpp"

namespace pkb {
thread_local std::string g_error;
}

namespace {

using pk::fe;
using pk::verdict;

}  // namespace

extern "C" {

int pkb_abi_version(void) { return 1; }

const char* pkb_check_name(int check) { return check == PKB_CHECK_TABLE ? "TABLE" : pkf_check_name(check); }

const char* pkb_create_error(void) { return pkb::g_error.c_str(); }

unsigned pkb_count_lds_max_d(void) { return pkb::COUNT_LDS_MAX_D; }

int pkb_plan(const pkb_statement* stmt, pkb_digit_plan* plan_out) {
    std::string why;
    if (!plan_out) return pkb::refuse("null pointer");
    if (!pkb::statement_ok(stmt, why)) return pkb::refuse(why);
    const pkb::Plan P = pkb::plan_of(stmt->L);
    memset(plan_out, 0, sizeof *plan_out);
    plan_out->bits = stmt->L * stmt->d, plan_out->k = 2 * stmt->d, plan_out->c_groups = P.c;
    for (unsigned g = 0; g < P.c; g++) plan_out->digit_of[g] = P.digit_of[g];
    return PK_OK;
}

int pkb_io_pattern(const pkb_statement* stmt, uint8_t* buf, size_t cap, size_t* len) { return pk::pattern_out<pkb::Lib>(stmt, buf, cap, len); }

int pkb_proof_bytes(const pkb_statement* stmt, size_t* len) {
    std::string why;
    if (!len) return pkb::refuse("null pointer");
    if (!pkb::statement_ok(stmt, why)) return pkb::refuse(why);
    const pkt_statement look = pkb::lookup_of(*stmt);
    if (int rc = pkt_proof_bytes(&look, len)) return pkb::g_error = pkt_create_error(), rc;
    return PK_OK;
}

int pkb_verify(const pkb_statement* stmt, const uint8_t* io_pattern_or_null, size_t io_pattern_len, const uint64_t* bind, const uint8_t* proof, size_t len,
               pkb_claims* claims_out, int* side_out, unsigned* layer_out, pkv_result* result) {
    std::string why;
    if (!result || (!proof && len)) return pkb::refuse("null pointer");
    if (!pkb::statement_ok(stmt, why)) return pkb::refuse(why);
    const pkb_statement& st = *stmt;
    if (st.n_bind && !bind) return pkb::refuse("the statement binds elements: pass them");
    if (!pkb::elements_below_p(bind, st.n_bind, "bind", why)) return pkb::refuse(why);
    try {
        pkv::Statement ps;
        if (int rc = pk::parse_pattern(ps, io_pattern_or_null, io_pattern_len, pkb::io_pattern(st), pkb::g_error)) return rc;
        const pkt_statement look = pkb::lookup_of(st);
        size_t total = 0;
        if (int rc = pkt_proof_bytes(&look, &total)) return pkb::g_error = pkt_create_error(), rc;
        // where a verdict points: the side and the layer it is about
        auto about = [&](int side, unsigned layer) {
            if (side_out) *side_out = side;
            if (layer_out) *layer_out = layer;
        };
        about(PKT_SIDE_F, 0);
        // framing first: the one part has a fixed length, so a proof of another length is judged before it is read
        if (len < total) return verdict(result, PKV_CHECK_TRANSCRIPT_SHORT, len, "the proof is shorter than its lookup"), PK_OK;
        if (len > total) return verdict(result, PKV_CHECK_TRAILING_BYTES, total, "bytes left after the proof"), PK_OK;
        fe seed;
        if (!pk::squeeze_outer(ps, bind, st.n_bind, {{1, &seed}}, result)) return PK_OK;

        pkt_claims seen;
        int side = PKT_SIDE_F;
        unsigned layer = 0;
        if (int rc = pkt_verify(&look, nullptr, 0, (const uint64_t*)seed.v, proof, total, &seen, &side, &layer, result)) return pkb::g_error = pkt_create_error(), rc;
        about(side, layer);
        if (!result->accepted) return PK_OK;
        // the table is not committed: its claim is checked against the extension of the operation's table, which the verifier evaluates itself
        fe z_t[PKB_MAX_VARS];
        for (unsigned i = 0; i < 2 * st.d; i++) z_t[i] = pk::h_load(seen.z_t[i]);
        if (!pk::fe_eq(pk::h_load(seen.t_value), pkb::table_at(st.op, st.d, z_t, pk::h_load(seen.beta))))
            return about(PKT_SIDE_T, 0),
                   verdict(result, PKB_CHECK_TABLE, total, "the lookup's table claim is not U + beta V + beta^2 O at z_T: its table is not the operation's"), PK_OK;
        verdict(result, PKV_CHECK_NONE, total, "");
        about(PKT_SIDE_F, 0);
        if (claims_out) pkb::fill_claims(st, seen, claims_out);
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

int pkb_check_claims(const pkb_statement* stmt, const pkb_claims* claims, const uint64_t* abc_evals, const uint64_t* digit_evals, const uint64_t* m_eval,
                     int* which_out) {
    std::string why;
    if (!claims || !abc_evals || !digit_evals || !m_eval || !which_out) return pkb::refuse("null pointer");
    if (!pkb::statement_ok(stmt, why)) return pkb::refuse(why);
    const unsigned L = stmt->L;
    if (!pkb::elements_below_p(abc_evals, 3, "abc_evals", why) || !pkb::elements_below_p(digit_evals, 3 * L, "digit_evals", why) ||
        !pkb::elements_below_p(m_eval, 1, "m_eval", why) || !pkb::elements_below_p(&claims->z_lo[0][0], sizeof *claims / 32, "claims", why))
        return pkb::refuse(why);
    fe looked = pk::fe_zero(), whole[3];
    for (unsigned j = 0; j < 3; j++) {
        whole[j] = pk::fe_zero();
        for (unsigned i = 0; i < L; i++) {
            const fe digit = pk::h_load(digit_evals + 4 * (j * L + i));
            looked = pk::h_add(looked, pk::h_mul(pk::h_load(claims->digit_coeff[j][i]), digit));
            whole[j] = pk::h_add(whole[j], pk::h_mul(pk::h_load(claims->pow2[i]), digit));
        }
    }
    *which_out = PKB_CLAIM_NONE;
    if (!pk::fe_eq(looked, pk::h_load(claims->digits_value))) return *which_out = PKB_CLAIM_DIGITS, PK_OK;
    for (unsigned j = 0; j < 3; j++)
        if (!pk::fe_eq(whole[j], pk::h_load(abc_evals + 4 * j))) return *which_out = PKB_CLAIM_RECOMPOSE_A + (int)j, PK_OK;
    if (!pk::fe_eq(pk::h_load(m_eval), pk::h_load(claims->m_value))) *which_out = PKB_CLAIM_M;
    return PK_OK;
}

}  // extern "C"
