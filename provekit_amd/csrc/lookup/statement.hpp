// statement.hpp -- what the sources of libprovekit_lookup.so share on the host: which statements the library takes, the outer IO
// pattern, the two pks statements of a proof, the proof's framing and the derivation of the claims.  Host only; no device, no
// product call.
#pragma once
#include <string>

#include "../../../include/provekit_lookup.h"
#include "../argument.hpp"

namespace pkl {

using pk::fe;

extern thread_local std::string g_error;  // pkl_create_error
inline int refuse(const std::string& why) { return pk::refuse(g_error, why); }

inline bool statement_ok(const pkl_statement* s, std::string& why) {
    if (!s) return why = "null statement", false;
    if (s->n < 1 || s->n > PKL_MAX_VARS) return why = "n must be 1..28", false;
    if (s->k < 1 || s->k > PKL_MAX_VARS) return why = "k must be 1..28", false;
    if (s->n_bind > PKL_MAX_BIND) return why = "n_bind must be 0..16", false;
    if (s->n_bind2 > PKL_MAX_BIND) return why = "n_bind2 must be 0..16", false;
    return true;
}

inline std::string io_pattern(const pkl_statement& s) {
    std::string d = "provekit-hip/lookup/v1/n" + std::to_string(s.n) + "/k" + std::to_string(s.k);
    auto op = [&](char kind, size_t n, const char* label) { pk::pattern_op(d, kind, n, label); };
    op('A', s.n_bind, "bind");
    op('S', 1, "alpha");
    op('A', s.n_bind2, "helpers");
    op('A', 1, "sum");
    op('S', s.n, "tau_f");
    op('S', s.k, "tau_t");
    op('S', 1, "seed");
    return d;
}

// The two sumcheck statements: constant, so a prover creates its pks provers once.
//   F: sum_x eq(tau_f, x) h_f d_f = 1;   T: sum_y eq(tau_t, y) (h_t d_t - m) = 0;   each binds the outer transcript's seed
inline pks_statement side_statement(const pkl_statement& s, int side) {
    pks_statement st{};
    const fe one = pk::fe_one(), minus_one = pk::fe_neg(pk::fe_one());
    st.has_tau = 1, st.n_bind = 1;
    memcpy(st.coeffs[0], one.v, 32);
    if (side == PKL_SIDE_F) {
        st.n = s.n, st.m = 2, st.T = 1, st.masks[0] = 3;
    } else {
        st.n = s.k, st.m = 3, st.T = 2, st.masks[0] = 3, st.masks[1] = 4;
        memcpy(st.coeffs[1], minus_one.v, 32);
    }
    return st;
}
inline fe side_expected_sum(int side) { return side == PKL_SIDE_F ? pk::fe_one() : pk::fe_zero(); }

// the proof: s | pks proof F | pks proof T
struct Framing {
    size_t f_at = 32, f_len = 0, t_at = 0, t_len = 0, total = 0;
};
inline int framing(const pkl_statement& s, Framing& fr) {
    const pks_statement F = side_statement(s, PKL_SIDE_F), T = side_statement(s, PKL_SIDE_T);
    if (int rc = pks_proof_bytes(&F, &fr.f_len)) return rc;
    if (int rc = pks_proof_bytes(&T, &fr.t_len)) return rc;
    fr.t_at = fr.f_at + fr.f_len;
    fr.total = fr.t_at + fr.t_len;
    return PK_OK;
}

// 2^-vars
inline fe half_pow(unsigned vars) { return pk::h_pow(pk::h_half(), vars); }

// The seven claims from what both sides hold after the two sumchecks: finals_f = {h_f, d_f}(r_f), finals_t = {h_t, d_t, m}(r_t)
inline void derive_claims(const pkl_statement& st, const fe& alpha, const fe& s, const fe* r_f, const fe* r_t, const fe* finals_f, const fe* finals_t,
                          pkl_claims* c) {
    memset(c, 0, sizeof *c);
    const auto put = pk::put_fe;
    put(c->alpha, alpha);
    put(c->s, s);
    for (unsigned i = 0; i < st.n; i++) put(c->r_f[i], r_f[i]);
    for (unsigned i = 0; i < st.k; i++) put(c->r_t[i], r_t[i]);
    put(c->hf_at_rf, finals_f[0]);
    put(c->f_at_rf, pk::h_sub(alpha, finals_f[1]));
    put(c->ht_at_rt, finals_t[0]);
    put(c->t_at_rt, pk::h_sub(alpha, finals_t[1]));
    put(c->m_at_rt, finals_t[2]);
    put(c->hf_at_half, pk::h_mul(s, half_pow(st.n)));
    put(c->ht_at_half, pk::h_mul(s, half_pow(st.k)));
}

}  // namespace pkl
