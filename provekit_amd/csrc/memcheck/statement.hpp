// statement.hpp -- what the sources of libprovekit_memcheck.so share on the host: which statements the library takes, the outer IO
// pattern, the three sides' inner statements, the challenges' order, the index polynomial I and the coefficients of the claims.  Host
// only; no device, and of other libraries only what provekit_fracsum.h declares.
#pragma once
#include <string>

#include "../../../include/provekit_memcheck.h"
#include "../argument.hpp"

namespace pkm {

using pk::fe;

extern thread_local std::string g_error;  // pkm_create_error
inline int refuse(const std::string& why) { return pk::refuse(g_error, why); }

using pk::elements_below_p;
using pk::pattern_op;
using pk::put_fe;

inline bool statement_ok(const pkm_statement* s, std::string& why) {
    if (!s) return why = "null statement", false;
    if (s->n < 1 || s->n > PKM_MAX_VARS) return why = "n must be 1..27", false;
    if (s->k < 1 || s->k > PKM_MAX_VARS) return why = "k must be 1..27", false;
    if (s->n_bind > PKM_MAX_BIND) return why = "n_bind must be 0..16", false;
    return true;
}

inline std::string io_pattern(const pkm_statement& s) {
    std::string d = "provekit-hip/memcheck/v1/n" + std::to_string(s.n) + "/k" + std::to_string(s.k);
    pattern_op(d, 'A', s.n_bind, "bind");
    pattern_op(d, 'S', 1, "gamma");
    pattern_op(d, 'S', 1, "beta");
    pattern_op(d, 'S', 3, "seeds");
    return d;
}

// the three sides of a proof: two stacked fractional sums with the sign table as numerators, and the time side's lookup; each binds
// its seed
inline unsigned stacked_vars(const pkm_statement& s, int side) { return (side == PKM_SIDE_OPS ? s.n : s.k) + 1; }
inline pkf_statement side_sum(const pkm_statement& s, int side) { return pkf_statement{stacked_vars(s, side), 1, 0}; }
inline pkf_lookup_statement side_time(const pkm_statement& s) { return pkf_lookup_statement{s.n, s.n, 1}; }

// What the outer transcript gives, on either side of it
struct Challenges {
    fe gamma, beta, seeds[3];
};

// I(z) = sum_j z_j 2^(v-1-j): argument.hpp's, shared with the Spark library
using pk::index_at;
// the sign table's extension at a stacked point: +1 on the first half, -1 on the second
inline fe sign_at(const fe& z0) { return pk::h_sub(pk::fe_one(), pk::h_add(z0, z0)); }
// P_a / Q_a + P_b / Q_b = 0
inline bool balanced(const fe& Pa, const fe& Qa, const fe& Pb, const fe& Qb) { return pk::is_zero(pk::h_add(pk::h_mul(Pa, Qb), pk::h_mul(Pb, Qa))); }

// The claims of an accepted proof from the chains' ends: z[side] (the stacked points, n + 1 and k + 1 coordinates) with cq[side], and
// the time side's claims
inline void fill_claims(const pkm_statement& s, const Challenges& ch, const fe* z_ops, const fe& cq_ops, const fe* z_mem, const fe& cq_mem,
                        const pkf_lookup_claims& time, pkm_claims* out) {
    memset(out, 0, sizeof *out);
    put_fe(out->gamma, ch.gamma), put_fe(out->beta, ch.beta);
    for (unsigned i = 0; i < s.n; i++) put_fe(out->z_ops[i], z_ops[1 + i]);
    for (unsigned i = 0; i < s.k; i++) put_fe(out->z_mem[i], z_mem[1 + i]);
    memcpy(out->z_f, time.z_f, 32 * (size_t)s.n);
    memcpy(out->z_t, time.z_t, 32 * (size_t)s.n);
    const fe one = pk::fe_one(), beta2 = pk::h_mul(ch.beta, ch.beta);
    const fe &z0 = z_ops[0], &y0 = z_mem[0];
    put_fe(out->ops_coeff[0], one);
    put_fe(out->ops_coeff[1], pk::h_mul(ch.beta, pk::h_sub(one, z0)));
    put_fe(out->ops_coeff[2], pk::h_mul(ch.beta, z0));
    put_fe(out->ops_coeff[3], pk::h_mul(beta2, z0));
    put_fe(out->mem_coeff[0], pk::h_mul(ch.beta, pk::h_sub(one, y0)));
    put_fe(out->mem_coeff[1], pk::h_mul(ch.beta, y0));
    put_fe(out->mem_coeff[2], pk::h_mul(beta2, y0));
    const fe time_term = pk::h_mul(pk::h_mul(beta2, pk::h_sub(one, z0)), pk::h_add(index_at(z_ops + 1, s.n), one));
    put_fe(out->ops_value, pk::h_sub(pk::h_sub(ch.gamma, cq_ops), time_term));
    put_fe(out->mem_value, pk::h_sub(pk::h_sub(ch.gamma, cq_mem), index_at(z_mem + 1, s.k)));
    fe z_f[PKM_MAX_VARS];
    for (unsigned i = 0; i < s.n; i++) z_f[i] = pk::h_load(time.z_f[i]);
    put_fe(out->rt_value, pk::h_sub(index_at(z_f, s.n), pk::h_load(time.f_value)));
    memcpy(out->m_value, time.m_value, 32);
}

// the library's overload sets, for argument.hpp's templates (the proof's length comes from the fractional-sum library's C ABI)
struct Lib {
    static std::string& error() { return g_error; }
    static bool ok(const pkm_statement* s, std::string& why) { return statement_ok(s, why); }
    static std::string pattern(const pkm_statement& s) { return io_pattern(s); }
};

}  // namespace pkm
