// statement.hpp -- what the sources of libprovekit_fracsum.so share on the host: which statements the library takes, the two outer IO
// patterns, the pks statement of a layer, the proof's framing, the steps from the top and from one layer's finals to the next claims,
// and with them the rule of this library's chain (gkr/chain.hpp) as far as prover and verifier share it.  Host only; no device, no
// product call.
#pragma once
#include <string>

#include "../../../include/provekit_fracsum.h"
#include "../gkr/chain.hpp"

namespace pkf {

using pk::fe;

static_assert(PKF_MAX_VARS == pk::gkr::MAX_VARS && PKF_MAX_BIND == pk::gkr::MAX_BIND, "gkr/chain.hpp sizes its arrays by these");

extern thread_local std::string g_error;  // pkf_create_error
inline int refuse(const std::string& why) { return pk::refuse(g_error, why); }

inline bool statement_ok(const pkf_statement* s, std::string& why) {
    if (!s) return why = "null statement", false;
    if (s->n < 1 || s->n > PKF_MAX_VARS) return why = "n must be 1..28", false;
    if (s->n_bind > PKF_MAX_BIND) return why = "n_bind must be 0..16", false;
    if (s->unit > 1) return why = "unit must be 0 or 1", false;
    return true;
}
inline bool statement_ok(const pkf_lookup_statement* s, std::string& why) {
    if (!s) return why = "null statement", false;
    if (s->n < 1 || s->n > PKF_MAX_VARS) return why = "n must be 1..28", false;
    if (s->k < 1 || s->k > PKF_MAX_VARS) return why = "k must be 1..28", false;
    if (s->n_bind > PKF_MAX_BIND) return why = "n_bind must be 0..16", false;
    return true;
}
using pk::elements_below_p;
using pk::pattern_op;
using pk::put_fe;

// the layer whose children are unit leaves: three tables {qL, qR, u}, no numerators
inline bool unit_layer(const pkf_statement& s, unsigned d) { return s.unit && d + 1 == s.n; }
// tables, and so final values, of layer d's sumcheck
inline unsigned layer_tables(const pkf_statement& s, unsigned d) { return unit_layer(s, d) ? 3 : 4; }

inline std::string io_pattern(const pkf_statement& s) {
    std::string d = "provekit-hip/fracsum/v1/n" + std::to_string(s.n) + "/u" + std::to_string(s.unit);
    pattern_op(d, 'A', s.n_bind, "bind");
    pattern_op(d, 'A', 4, "top");
    pattern_op(d, 'S', 1, "rho");
    for (unsigned layer = 1; layer < s.n; layer++) {
        pattern_op(d, 'S', 1, "lambda");
        pattern_op(d, 'S', 1, "seed");
        pattern_op(d, 'A', layer_tables(s, layer), "finals");
        pattern_op(d, 'S', 1, "rho");
    }
    return d;
}
inline std::string io_pattern(const pkf_lookup_statement& s) {
    std::string d = "provekit-hip/logup-gkr/v1/n" + std::to_string(s.n) + "/k" + std::to_string(s.k);
    pattern_op(d, 'A', s.n_bind, "bind");
    pattern_op(d, 'S', 1, "alpha");
    pattern_op(d, 'S', 2, "seeds");
    return d;
}
// the two sides of a lookup proof: fractional sums that bind their seed
inline pkf_statement side_f(const pkf_lookup_statement& s) { return pkf_statement{s.n, 1, 1}; }
inline pkf_statement side_t(const pkf_lookup_statement& s) { return pkf_statement{s.k, 1, 0}; }

// Layer d's sumcheck over d variables, sum_x eq(z_d, x) (pL qR + qL u)(x) = cp_d + lambda_d cq_d with tables {pL, qL, qR, u}; over
// unit leaves sum_x eq(z_d, x) (qR + qL u)(x) with tables {qL, qR, u}.  Constant: lambda is inside u, so a prover creates its pks
// provers once.
inline pks_statement layer_statement(const pkf_statement& s, unsigned d) {
    pks_statement st{};
    const fe one = pk::fe_one();
    st.n = d, st.T = 2, st.has_tau = 1, st.n_bind = 1;
    if (unit_layer(s, d))
        st.m = 3, st.masks[0] = 2, st.masks[1] = 5;
    else
        st.m = 4, st.masks[0] = 5, st.masks[1] = 10;
    memcpy(st.coeffs[0], one.v, 32);
    memcpy(st.coeffs[1], one.v, 32);
    return st;
}
constexpr size_t TOP_BYTES = 128;
// bytes of layer d's pks proof (pks_proof_bytes of layer_statement): s, d rounds of 3 values, the finals
inline size_t layer_bytes(const pkf_statement& s, unsigned d) { return (size_t)32 * (1 + 3 * (size_t)d + layer_tables(s, d)); }
// where layer d's proof starts: top | layer 1 | .. ; layer_at(s, n) is the whole proof's length
inline size_t layer_at(const pkf_statement& s, unsigned d) {
    size_t at = TOP_BYTES;
    for (unsigned k = 1; k < d; k++) at += layer_bytes(s, k);
    return at;
}
inline size_t proof_bytes(const pkf_statement& s) { return layer_at(s, s.n); }
inline size_t proof_bytes(const pkf_lookup_statement& s) { return proof_bytes(side_f(s)) + proof_bytes(side_t(s)); }

// c' = (1 - rho) l + rho r
inline fe next_claim(const fe& l, const fe& r, const fe& rho) { return pk::h_add(l, pk::h_mul(rho, pk::h_sub(r, l))); }

// (P, Q) of the top values p_1[0], p_1[1], q_1[0], q_1[1]
inline void fraction_of(const fe top[4], fe& P, fe& Q) {
    P = pk::h_add(pk::h_mul(top[0], top[3]), pk::h_mul(top[1], top[2]));
    Q = pk::h_mul(top[2], top[3]);
}
// P_a Q_b = P_b Q_a
inline bool same_fraction(const fe& Pa, const fe& Qa, const fe& Pb, const fe& Qb) { return pk::fe_eq(pk::h_mul(Pa, Qb), pk::h_mul(Pb, Qa)); }

// The running claims of one chain, on either side of the transcript.
struct Claims {
    fe cp, cq;  // cp is meaningless once `has_p` is false
    bool has_p = true;
    void from_top(const fe top[4], const fe& rho) { cp = next_claim(top[0], top[1], rho), cq = next_claim(top[2], top[3], rho); }
    // the sum layer d's sumcheck must state
    fe expected(const fe& lambda) const { return pk::h_add(cp, pk::h_mul(lambda, cq)); }
    // after layer d's finals: (a, b, c, e), or (b, c, e) over unit leaves
    void step(bool unit_leaves, const fe* finals, const fe& lambda, const fe& rho) {
        if (unit_leaves) {
            cq = next_claim(finals[0], finals[1], rho), has_p = false;
        } else {
            const fe &a = finals[0], &b = finals[1], &c = finals[2], &e = finals[3];
            cp = next_claim(a, pk::h_sub(e, pk::h_mul(lambda, c)), rho), cq = next_claim(b, c, rho);
        }
    }
};
// over unit leaves the finals (b, c, e) must have e = 1 + lambda c: u is the table the statement says
inline bool unit_final_ok(const fe* finals, const fe& lambda) { return pk::fe_eq(finals[2], pk::h_add(pk::fe_one(), pk::h_mul(lambda, finals[1]))); }

// The rule of this library's chain, the part both sides of the transcript share: four top values, lambda and then the seed in front of
// a layer's sumcheck, four tables and so four finals per layer (three over unit leaves), and the running claims (cp, cq).
struct Chain {
    static constexpr unsigned TOP = 4, MAX_FINALS = 4, CHALLENGES = 2;  // ch[0]: lambda, ch[1]: the seed
    const pkf_statement& s;
    Claims claim;
    explicit Chain(const pkf_statement& st) : s(st) {}
    pks_statement layer_statement(unsigned d) const { return pkf::layer_statement(s, d); }
    size_t layer_at(unsigned d) const { return pkf::layer_at(s, d); }
    size_t layer_bytes(unsigned d) const { return pkf::layer_bytes(s, d); }
    unsigned finals(unsigned d) const { return layer_tables(s, d); }
    void start(const fe* top, const fe& rho) { claim.from_top(top, rho), claim.has_p = !(s.unit && s.n == 1); }
    fe expected(const fe* ch) const { return claim.expected(ch[0]); }
    void step(unsigned d, const fe* finals, const fe* ch, const fe& rho) { claim.step(unit_layer(s, d), finals, ch[0], rho); }
};

// the library's overload sets, for argument.hpp's templates
struct Lib {
    static std::string& error() { return g_error; }
    template <class S>
    static bool ok(const S* s, std::string& why) { return statement_ok(s, why); }
    template <class S>
    static std::string pattern(const S& s) { return io_pattern(s); }
};

}  // namespace pkf
