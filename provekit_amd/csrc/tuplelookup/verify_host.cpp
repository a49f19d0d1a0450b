// verify_host.cpp -- the host half of libprovekit_tuplelookup.so's C ABI: the statement's rules, the outer IO pattern, the verifier
// and the claims' three combinations.  No device code and no HIP call; of other libraries it calls pkf_verify, pkf_proof_bytes,
// pkf_check_name and pkf_create_error (provekit_fracsum.h).  This file and its headers are also what the sanitizer build (make asan,
// tuplelookup/asan_main.cpp) compiles, next to the fractional-sum and sumcheck libraries' host verifiers.
#include <vector>

#include "layout.hpp"

namespace pkt {
thread_local std::string g_error;
}

namespace {

using pk::fe;

using pk::verdict;

// the two sides' lengths; a pkf refusal of a statement this library made is passed on with its reason
int side_bytes(const pkt_statement& s, size_t out[2]) {
    const pkf_statement sides[2] = {pkt::side_f(s), pkt::side_t(s)};
    for (int which = 0; which < 2; which++)
        if (int rc = pkf_proof_bytes(&sides[which], &out[which])) return pkt::g_error = pkf_create_error(), rc;
    return PK_OK;
}

}  // namespace

extern "C" {

int pkt_abi_version(void) { return 1; }

const char* pkt_check_name(int check) { return pkf_check_name(check); }

const char* pkt_create_error(void) { return pkt::g_error.c_str(); }

unsigned pkt_count_lds_max_k(void) { return pkt::COUNT_LDS_MAX_K; }

int pkt_io_pattern(const pkt_statement* stmt, uint8_t* buf, size_t cap, size_t* len) { return pk::pattern_out<pkt::Lib>(stmt, buf, cap, len); }

int pkt_proof_bytes(const pkt_statement* stmt, size_t* len) {
    std::string why;
    if (!len) return pkt::refuse("null pointer");
    if (!pkt::statement_ok(stmt, why)) return pkt::refuse(why);
    size_t part[2];
    if (int rc = side_bytes(*stmt, part)) return rc;
    *len = part[0] + part[1];
    return PK_OK;
}

int pkt_verify(const pkt_statement* stmt, const uint8_t* io_pattern_or_null, size_t io_pattern_len, const uint64_t* bind, const uint8_t* proof, size_t len,
               pkt_claims* claims_out, int* side_out, unsigned* layer_out, pkv_result* result) {
    std::string why;
    if (!result || (!proof && len)) return pkt::refuse("null pointer");
    if (!pkt::statement_ok(stmt, why)) return pkt::refuse(why);
    const pkt_statement& s = *stmt;
    if (s.n_bind && !bind) return pkt::refuse("the statement binds elements: pass them");
    if (!pkt::elements_below_p(bind, s.n_bind, "bind", why)) return pkt::refuse(why);
    try {
        pkv::Statement st;
        if (int rc = pk::parse_pattern(st, io_pattern_or_null, io_pattern_len, pkt::io_pattern(s), pkt::g_error)) return rc;
        size_t part[2];
        if (int rc = side_bytes(s, part)) return rc;
        const pk::TwoSides sides(part[0], part[1], side_out, layer_out, result);
        if (!sides.framed(len)) return PK_OK;
        pkt::Challenges ch;
        ch.beta = pk::fe_one();
        if (!pk::squeeze_outer(st, bind, s.n_bind, {{1, &ch.alpha}, {s.w > 1, &ch.beta}, {2, ch.seeds}}, result)) return PK_OK;
        const pkf_statement side[2] = {pkt::side_f(s), pkt::side_t(s)};
        fe frac[2][2], z[2][PKT_MAX_VARS], cq[2], cp;
        if (int rc = sides.each([&](int which, unsigned& layer) {
                const int r = pkf_verify(&side[which], nullptr, 0, (const uint64_t*)ch.seeds[which].v, nullptr, proof + sides.at[which], part[which],
                                          (uint64_t*)frac[which], (uint64_t*)z[which], which == PKT_SIDE_T ? (uint64_t*)cp.v : nullptr, (uint64_t*)cq[which].v, &layer,
                                          result);
                if (r) pkt::g_error = pkf_create_error();
                return r;
            }))
            return rc;
        if (!result->accepted) return PK_OK;
        if (!pkt::same_fraction(frac[0][0], frac[0][1], frac[1][0], frac[1][1]))
            return verdict(result, PKF_CHECK_FRACTION, sides.at[1] + 128, "the two sides' fractions differ"), PK_OK;
        sides.accept();
        if (claims_out) pkt::fill_claims(s, ch, z[0], cq[0], z[1], cp, cq[1], claims_out);
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

int pkt_check_claims(const pkt_statement* stmt, const pkt_claims* claims, const uint64_t* f_evals, const uint64_t* t_evals, const uint64_t* m_eval, int* which_out) {
    std::string why;
    if (!claims || !f_evals || !t_evals || !m_eval || !which_out) return pkt::refuse("null pointer");
    if (!pkt::statement_ok(stmt, why)) return pkt::refuse(why);
    const pkt_statement& s = *stmt;
    if (!pkt::elements_below_p(f_evals, (size_t)s.c * s.w, "f_evals", why) || !pkt::elements_below_p(t_evals, s.w, "t_evals", why) ||
        !pkt::elements_below_p(m_eval, 1, "m_eval", why) || !pkt::elements_below_p(&claims->alpha[0], sizeof *claims / 32, "claims", why))
        return pkt::refuse(why);
    fe sum_f = pk::fe_zero(), sum_t = pk::fe_zero();
    for (unsigned j = 0; j < s.w; j++) {
        sum_t = pk::h_add(sum_t, pk::h_mul(pk::h_load(claims->t_coeff[j]), pk::h_load(t_evals + 4 * j)));
        for (unsigned g = 0; g < s.c; g++) sum_f = pk::h_add(sum_f, pk::h_mul(pk::h_load(claims->f_coeff[g][j]), pk::h_load(f_evals + 4 * (g * s.w + j))));
    }
    *which_out = !pk::fe_eq(sum_f, pk::h_load(claims->f_value))   ? PKT_CLAIM_F
                 : !pk::fe_eq(sum_t, pk::h_load(claims->t_value)) ? PKT_CLAIM_T
                 : !pk::fe_eq(pk::h_load(m_eval), pk::h_load(claims->m_value)) ? PKT_CLAIM_M
                                                                                : PKT_CLAIM_NONE;
    return PK_OK;
}

}  // extern "C"
