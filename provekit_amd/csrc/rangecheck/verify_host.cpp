// verify_host.cpp -- the host half of libprovekit_rangecheck.so's C ABI: the statement's rules and the plan, the outer IO pattern, the
// verifier with its table check and the three claims.  No device code and no HIP call; of other libraries it calls pkt_verify,
// pkt_proof_bytes, pkt_create_error and pkf_check_name.  This file and its headers are also what the sanitizer build (make asan,
// rangecheck/asan_main.cpp) compiles, next to the three host verifiers below it.
#include <vector>

#include "layout.hpp"

namespace pkr {
thread_local std::string g_error;
}

namespace {

using pk::fe;
using pk::verdict;

}  // namespace

extern "C" {

int pkr_abi_version(void) { return 1; }

const char* pkr_check_name(int check) { return check == PKR_CHECK_TABLE ? "TABLE" : pkf_check_name(check); }

const char* pkr_create_error(void) { return pkr::g_error.c_str(); }

unsigned pkr_count_lds_max_k(void) { return pkr::COUNT_LDS_MAX_K; }

int pkr_plan(const pkr_statement* stmt, pkr_limb_plan* plan_out) {
    std::string why;
    if (!plan_out) return pkr::refuse("null pointer");
    if (!pkr::statement_ok(stmt, why)) return pkr::refuse(why);
    const pkr::Plan P = pkr::plan_of(stmt->bits, stmt->k);
    memset(plan_out, 0, sizeof *plan_out);
    plan_out->limbs = P.L, plan_out->top_bits = P.r, plan_out->groups = P.G, plan_out->c = P.c;
    for (unsigned g = 0; g < P.c; g++) plan_out->limb_of[g] = P.limb_of[g], plan_out->shift_of[g] = P.shift_of[g];
    return PK_OK;
}

int pkr_io_pattern(const pkr_statement* stmt, uint8_t* buf, size_t cap, size_t* len) { return pk::pattern_out<pkr::Lib>(stmt, buf, cap, len); }

int pkr_proof_bytes(const pkr_statement* stmt, size_t* len) {
    std::string why;
    if (!len) return pkr::refuse("null pointer");
    if (!pkr::statement_ok(stmt, why)) return pkr::refuse(why);
    const pkt_statement look = pkr::lookup_of(*stmt);
    if (int rc = pkt_proof_bytes(&look, len)) return pkr::g_error = pkt_create_error(), rc;
    return PK_OK;
}

int pkr_verify(const pkr_statement* stmt, const uint8_t* io_pattern_or_null, size_t io_pattern_len, const uint64_t* bind, const uint8_t* proof, size_t len,
               pkr_claims* claims_out, int* side_out, unsigned* layer_out, pkv_result* result) {
    std::string why;
    if (!result || (!proof && len)) return pkr::refuse("null pointer");
    if (!pkr::statement_ok(stmt, why)) return pkr::refuse(why);
    const pkr_statement& st = *stmt;
    if (st.n_bind && !bind) return pkr::refuse("the statement binds elements: pass them");
    if (!pkr::elements_below_p(bind, st.n_bind, "bind", why)) return pkr::refuse(why);
    try {
        pkv::Statement ps;
        if (int rc = pk::parse_pattern(ps, io_pattern_or_null, io_pattern_len, pkr::io_pattern(st), pkr::g_error)) return rc;
        const pkt_statement look = pkr::lookup_of(st);
        size_t total = 0;
        if (int rc = pkt_proof_bytes(&look, &total)) return pkr::g_error = pkt_create_error(), rc;
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
        if (int rc = pkt_verify(&look, nullptr, 0, (const uint64_t*)seed.v, proof, total, &seen, &side, &layer, result)) return pkr::g_error = pkt_create_error(), rc;
        about(side, layer);
        if (!result->accepted) return PK_OK;
        // the table is not committed: its claim is checked against the extension of 0 .. 2^k - 1, which the verifier evaluates itself
        fe z_t[PKR_MAX_VARS];
        for (unsigned i = 0; i < st.k; i++) z_t[i] = pk::h_load(seen.z_t[i]);
        if (!pk::fe_eq(pk::h_load(seen.t_value), pk::index_at(z_t, st.k)))
            return about(PKT_SIDE_T, 0), verdict(result, PKR_CHECK_TABLE, total, "the lookup's table claim is not I(z_T): its table is not 0 .. 2^k - 1"), PK_OK;
        verdict(result, PKV_CHECK_NONE, total, "");
        about(PKT_SIDE_F, 0);
        if (claims_out) pkr::fill_claims(st, seen, claims_out);
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

int pkr_check_claims(const pkr_statement* stmt, const pkr_claims* claims, const uint64_t* f_eval, const uint64_t* limb_evals, const uint64_t* m_eval, int* which_out) {
    std::string why;
    if (!claims || !f_eval || !limb_evals || !m_eval || !which_out) return pkr::refuse("null pointer");
    if (!pkr::statement_ok(stmt, why)) return pkr::refuse(why);
    const pkr::Plan P = pkr::plan_of(stmt->bits, stmt->k);
    if (!pkr::elements_below_p(f_eval, 1, "f_eval", why) || !pkr::elements_below_p(limb_evals, P.L, "limb_evals", why) ||
        !pkr::elements_below_p(m_eval, 1, "m_eval", why) || !pkr::elements_below_p(&claims->z_lo[0][0], sizeof *claims / 32, "claims", why))
        return pkr::refuse(why);
    fe looked = pk::fe_zero(), whole = pk::fe_zero();
    for (unsigned i = 0; i < P.L; i++) {
        const fe limb = pk::h_load(limb_evals + 4 * i);
        looked = pk::h_add(looked, pk::h_mul(pk::h_load(claims->limb_coeff[i]), limb));
        whole = pk::h_add(whole, pk::h_mul(pk::h_load(claims->pow2[i]), limb));
    }
    *which_out = !pk::fe_eq(looked, pk::h_load(claims->limbs_value)) ? PKR_CLAIM_LIMBS
                 : !pk::fe_eq(whole, pk::h_load(f_eval))             ? PKR_CLAIM_RECOMPOSE
                 : !pk::fe_eq(pk::h_load(m_eval), pk::h_load(claims->m_value)) ? PKR_CLAIM_M
                                                                                : PKR_CLAIM_NONE;
    return PK_OK;
}

}  // extern "C"
