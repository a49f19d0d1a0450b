// statement.hpp -- what the sources of libprovekit_grandproduct.so share on the host: which statements the library takes, the two
// outer IO patterns, the pks statement of a layer, the proof's framing, the step from one layer's claim to the next, and with them
// the rule of this library's chain (gkr/chain.hpp) as far as prover and verifier share it.  Host only; no device, no product call.
#pragma once
#include <string>

#include "../../../include/provekit_grandproduct.h"
#include "../gkr/chain.hpp"

namespace pkg {

using pk::fe;

static_assert(PKG_MAX_VARS == pk::gkr::MAX_VARS && PKG_MAX_BIND == pk::gkr::MAX_BIND, "gkr/chain.hpp sizes its arrays by these");

extern thread_local std::string g_error;  // pkg_create_error
inline int refuse(const std::string& why) { return pk::refuse(g_error, why); }

inline bool statement_ok(const pkg_statement* s, std::string& why) {
    if (!s) return why = "null statement", false;
    if (s->n < 1 || s->n > PKG_MAX_VARS) return why = "n must be 1..28", false;
    if (s->n_bind > PKG_MAX_BIND) return why = "n_bind must be 0..16", false;
    return true;
}
inline bool statement_ok(const pkg_multiset_statement* s, std::string& why) {
    if (!s) return why = "null statement", false;
    if (s->n < 1 || s->n > PKG_MAX_VARS) return why = "n must be 1..28", false;
    if (s->w < 1 || s->w > PKG_MAX_COLUMNS) return why = "w must be 1..4", false;
    if (s->n_bind > PKG_MAX_BIND) return why = "n_bind must be 0..16", false;
    return true;
}
using pk::elements_below_p;
using pk::pattern_op;
using pk::put_fe;

inline std::string io_pattern(const pkg_statement& s) {
    std::string d = "provekit-hip/grandproduct/v1/n" + std::to_string(s.n);
    pattern_op(d, 'A', s.n_bind, "bind");
    pattern_op(d, 'A', 2, "top");
    pattern_op(d, 'S', 1, "rho");
    for (unsigned layer = 1; layer < s.n; layer++) {
        pattern_op(d, 'S', 1, "seed");
        pattern_op(d, 'A', 2, "finals");
        pattern_op(d, 'S', 1, "rho");
    }
    return d;
}
inline std::string io_pattern(const pkg_multiset_statement& s) {
    std::string d = "provekit-hip/multiset/v1/n" + std::to_string(s.n) + "/w" + std::to_string(s.w);
    pattern_op(d, 'A', s.n_bind, "bind");
    pattern_op(d, 'S', 1, "gamma");
    pattern_op(d, 'S', s.w > 1 ? 1 : 0, "beta");
    pattern_op(d, 'S', 2, "seeds");
    return d;
}
// each side of a multiset proof is a grand product that binds its seed
inline pkg_statement side_statement(const pkg_multiset_statement& s) { return pkg_statement{s.n, 1}; }

// Layer d's sumcheck, sum_x eq(z_d, x) L_d(x) R_d(x) = c_d over d variables: constant, so a prover creates its pks provers once.
inline pks_statement layer_statement(unsigned d) {
    pks_statement st{};
    const fe one = pk::fe_one();
    st.n = d, st.m = 2, st.T = 1, st.masks[0] = 3, st.has_tau = 1, st.n_bind = 1;
    memcpy(st.coeffs[0], one.v, 32);
    return st;
}
// bytes of layer d's pks proof: s, d rounds of 3 values, 2 finals
inline size_t layer_bytes(unsigned d) { return (size_t)32 * (3 + 3 * (size_t)d); }
// where layer d's proof starts: top | layer 1 | .. ; layer_at(n) is the whole proof's length, 64 + 48 (n - 1)(n + 2)
inline size_t layer_at(unsigned d) { return 64 + (size_t)48 * (d - 1) * (d + 2); }
inline size_t proof_bytes(const pkg_statement& s) { return layer_at(s.n); }
inline size_t proof_bytes(const pkg_multiset_statement& s) { return 2 * layer_at(s.n); }

// c' = (1 - rho) l + rho r
inline fe next_claim(const fe& l, const fe& r, const fe& rho) { return pk::h_add(l, pk::h_mul(rho, pk::h_sub(r, l))); }

// The rule of this library's chain, the part both sides of the transcript share: two top values, the seed alone in front of a layer's
// sumcheck, two tables and so two finals (l, r) per layer, and one running claim: the value of V_d at z_d.
struct Chain {
    static constexpr unsigned TOP = 2, MAX_FINALS = 2, CHALLENGES = 1;
    const pkg_statement& s;
    fe claim;
    explicit Chain(const pkg_statement& st) : s(st) {}
    pks_statement layer_statement(unsigned d) const { return pkg::layer_statement(d); }
    size_t layer_at(unsigned d) const { return pkg::layer_at(d); }
    size_t layer_bytes(unsigned d) const { return pkg::layer_bytes(d); }
    unsigned finals(unsigned) const { return 2; }
    void start(const fe* top, const fe& rho) { claim = next_claim(top[0], top[1], rho); }
    fe expected(const fe*) const { return claim; }
    void step(unsigned, const fe* lr, const fe*, const fe& rho) { claim = next_claim(lr[0], lr[1], rho); }
};

// the library's overload sets, for argument.hpp's templates
struct Lib {
    static std::string& error() { return g_error; }
    template <class S>
    static bool ok(const S* s, std::string& why) { return statement_ok(s, why); }
    template <class S>
    static std::string pattern(const S& s) { return io_pattern(s); }
};

}  // namespace pkg
