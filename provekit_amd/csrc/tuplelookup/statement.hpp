// statement.hpp -- what the sources of libprovekit_tuplelookup.so share on the host: which statements the library takes, the outer IO
// pattern, the two sides' pkf statements, the challenges' order and the coefficients of the claims.  Host only; no device, and of
// other libraries only what provekit_fracsum.h declares.
#pragma once
#include <string>

#include "../../../include/provekit_tuplelookup.h"
#include "../argument.hpp"

namespace pkt {

using pk::fe;

extern thread_local std::string g_error;  // pkt_create_error
inline int refuse(const std::string& why) { return pk::refuse(g_error, why); }

using pk::elements_below_p;
using pk::pattern_op;
using pk::put_fe;

inline bool groups_ok(unsigned c) { return c == 1 || c == 2 || c == 4; }
inline unsigned log2_groups(unsigned c) { return c == 4 ? 2 : c == 2 ? 1 : 0; }

inline bool statement_ok(const pkt_statement* s, std::string& why) {
    if (!s) return why = "null statement", false;
    if (s->n < 1 || s->n > PKT_MAX_VARS) return why = "n must be 1..28", false;
    if (s->k < 1 || s->k > PKT_MAX_VARS) return why = "k must be 1..28", false;
    if (s->w < 1 || s->w > PKT_MAX_WIDTH) return why = "w must be 1..4", false;
    if (!groups_ok(s->c)) return why = "c must be 1, 2 or 4", false;
    if (s->n + log2_groups(s->c) > PKT_MAX_VARS) return why = "n + log2 c must be at most 28", false;
    if (s->n_bind > PKT_MAX_BIND) return why = "n_bind must be 0..16", false;
    return true;
}

inline std::string io_pattern(const pkt_statement& s) {
    std::string d = "provekit-hip/tuple-lookup/v1/n" + std::to_string(s.n) + "/k" + std::to_string(s.k) + "/w" + std::to_string(s.w) + "/c" + std::to_string(s.c);
    pattern_op(d, 'A', s.n_bind, "bind");
    pattern_op(d, 'S', 1, "alpha");
    pattern_op(d, 'S', s.w > 1 ? 1 : 0, "beta");
    pattern_op(d, 'S', 2, "seeds");
    return d;
}

// the two sides of a proof: fractional sums that bind their seed; side F over the c stacked groups
inline unsigned stacked_vars(const pkt_statement& s) { return s.n + log2_groups(s.c); }
inline pkf_statement side_f(const pkt_statement& s) { return pkf_statement{stacked_vars(s), 1, 1}; }
inline pkf_statement side_t(const pkt_statement& s) { return pkf_statement{s.k, 1, 0}; }

// What the outer transcript gives, on either side of it
struct Challenges {
    fe alpha, beta, seeds[2];
};

// The claims of an accepted proof from the two chains' ends: z_f (n + log2 c coordinates) and cq_F; z_t (k) with cp_T and cq_T
inline void fill_claims(const pkt_statement& s, const Challenges& ch, const fe* z_f, const fe& cq_f, const fe* z_t, const fe& cp_t, const fe& cq_t, pkt_claims* out) {
    memset(out, 0, sizeof *out);
    const unsigned hi = log2_groups(s.c);
    put_fe(out->alpha, ch.alpha), put_fe(out->beta, ch.beta);
    for (unsigned i = 0; i < s.n; i++) put_fe(out->z_lo[i], z_f[hi + i]);
    for (unsigned i = 0; i < s.k; i++) put_fe(out->z_t[i], z_t[i]);
    fe power = pk::fe_one();
    for (unsigned j = 0; j < s.w; j++) {
        put_fe(out->t_coeff[j], power);
        for (unsigned g = 0; g < s.c; g++) {
            fe eq = power;  // eq(z_hi, g) beta^j: coordinate i of z_hi <-> bit hi - 1 - i of g
            for (unsigned i = 0; i < hi; i++) eq = pk::h_mul(eq, (g >> (hi - 1 - i)) & 1 ? z_f[i] : pk::h_sub(pk::fe_one(), z_f[i]));
            put_fe(out->f_coeff[g][j], eq);
        }
        power = pk::h_mul(power, ch.beta);
    }
    put_fe(out->f_value, pk::h_sub(ch.alpha, cq_f));
    put_fe(out->t_value, pk::h_sub(ch.alpha, cq_t));
    put_fe(out->m_value, cp_t);
}

// the library's overload sets, for argument.hpp's templates (the proof's length comes from the fractional-sum library's C ABI)
struct Lib {
    static std::string& error() { return g_error; }
    static bool ok(const pkt_statement* s, std::string& why) { return statement_ok(s, why); }
    static std::string pattern(const pkt_statement& s) { return io_pattern(s); }
};

// P_a Q_b = P_b Q_a
inline bool same_fraction(const fe& Pa, const fe& Qa, const fe& Pb, const fe& Qb) { return pk::fe_eq(pk::h_mul(Pa, Qb), pk::h_mul(Pb, Qa)); }

}  // namespace pkt
