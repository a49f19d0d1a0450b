// statement.hpp -- what the sources of libprovekit_bitwise.so share: the plan and the operation (one __host__ __device__ rule each that
// prover, verifier, kernels and claims read), which statements the library takes, the outer IO pattern, the inner lookup's statement,
// the table's extension and the claims.  Of other libraries only what provekit_tuplelookup.h declares.
#pragma once
#include <string>

#include "../../../include/provekit_bitwise.h"
#include "../argument.hpp"

namespace pkb {

using pk::fe;

// THE PLAN.  Group i < L is the digit row (a_i, b_i, c_i); c the smallest of {1, 2, 4} with c >= L, the spare group of L = 3 being
// digit 0 again.  Valid for 1 <= L <= 4.
struct Plan {
    unsigned c;
    unsigned digit_of[PKB_MAX_DIGITS];
};
__host__ __device__ inline Plan plan_of(unsigned L) {
    Plan P{};
    P.c = L == 3 ? 4 : L;
    for (unsigned g = 0; g < PKB_MAX_DIGITS; g++) P.digit_of[g] = g < L ? g : 0;  // the spare group: digit 0 again
    return P;
}
// THE OPERATION on integers, for the kernels and the table
__host__ __device__ inline uint64_t apply(unsigned op, uint64_t a, uint64_t b) { return op == PKB_AND ? a & b : op == PKB_XOR ? a ^ b : a | b; }

extern thread_local std::string g_error;  // pkb_create_error
inline int refuse(const std::string& why) { return pk::refuse(g_error, why); }

using pk::elements_below_p;
using pk::pattern_op;
using pk::put_fe;

inline unsigned log2_groups(unsigned c) { return c == 4 ? 2 : c == 2 ? 1 : 0; }
inline const char* op_name(unsigned op) { return op == PKB_AND ? "and" : op == PKB_XOR ? "xor" : "or"; }

inline bool statement_ok(const pkb_statement* s, std::string& why) {
    if (!s) return why = "null statement", false;
    if (s->n < 1 || s->n > PKB_MAX_VARS) return why = "n must be 1..28", false;
    if (s->op >= PKB_OP_COUNT) return why = "op must be PKB_AND, PKB_XOR or PKB_OR", false;
    if (s->d < 1 || s->d > PKB_MAX_DIGIT_BITS) return why = "d must be 1..12", false;
    if (s->L < 1 || s->L > PKB_MAX_DIGITS) return why = "L must be 1..4", false;
    if (s->n_bind > PKB_MAX_BIND) return why = "n_bind must be 0..16", false;
    const Plan P = plan_of(s->L);
    if (s->n + log2_groups(P.c) > PKB_MAX_VARS) return why = "n + log2 c must be at most 28 (c = " + std::to_string(P.c) + " groups)", false;
    return true;
}

inline std::string io_pattern(const pkb_statement& s) {
    std::string d = std::string("provekit-hip/bitwise/v1/") + op_name(s.op) + "/n" + std::to_string(s.n) + "/d" + std::to_string(s.d) + "/l" + std::to_string(s.L);
    pattern_op(d, 'A', s.n_bind, "bind");
    pattern_op(d, 'S', 1, "seed");
    return d;
}

// the one inner proof: c groups of three columns in the operation's table, binding the seed
inline pkt_statement lookup_of(const pkb_statement& s) { return pkt_statement{s.n, 2 * s.d, 3, plan_of(s.L).c, 1}; }

// 2^e as an element, e < 64
inline fe pow2(unsigned e) { return pk::h_from_u64((uint64_t)1 << e); }

// The extension of the table's compressed row at z (2 d coordinates, variable 0 the most significant bit): U + beta V + beta^2 O,
// U = I_d(z[0..d)), V = I_d(z[d..2d)), O = sum_j 2^(d-1-j) o(z[j], z[d+j]); o(s, t) = s t, s + t - 2 s t, s + t - s t
inline fe table_at(unsigned op, unsigned d, const fe* z, const fe& beta) {
    fe o = pk::fe_zero();
    for (unsigned j = 0; j < d; j++) {  // Horner in 2
        const fe st = pk::h_mul(z[j], z[d + j]), sum = pk::h_add(z[j], z[d + j]);
        const fe bit = op == PKB_AND ? st : op == PKB_XOR ? pk::h_sub(sum, pk::h_add(st, st)) : pk::h_sub(sum, st);
        o = pk::h_add(pk::h_add(o, o), bit);
    }
    return pk::h_add(pk::index_at(z, d), pk::h_mul(beta, pk::h_add(pk::index_at(z + d, d), pk::h_mul(beta, o))));
}

// The claims of an accepted proof from the lookup's: coeff[j][i] = the sum over the groups g of digit i of eq(z_hi, g) beta^j, which
// is the lookup's f_coeff[g][j]
inline void fill_claims(const pkb_statement& s, const pkt_claims& look, pkb_claims* out) {
    memset(out, 0, sizeof *out);
    const Plan P = plan_of(s.L);
    memcpy(out->z_lo, look.z_lo, 32 * (size_t)s.n);
    memcpy(out->z_t, look.z_t, 32 * (size_t)(2 * s.d));
    for (unsigned j = 0; j < 3; j++) {
        fe coeff[PKB_MAX_DIGITS];
        for (fe& c : coeff) c = pk::fe_zero();
        for (unsigned g = 0; g < P.c; g++) coeff[P.digit_of[g]] = pk::h_add(coeff[P.digit_of[g]], pk::h_load(look.f_coeff[g][j]));
        for (unsigned i = 0; i < s.L; i++) put_fe(out->digit_coeff[j][i], coeff[i]);
    }
    for (unsigned i = 0; i < s.L; i++) put_fe(out->pow2[i], pow2(s.d * i));
    memcpy(out->digits_value, look.f_value, 32);
    memcpy(out->m_value, look.m_value, 32);
}

// the library's overload sets, for argument.hpp's templates (the proof's length comes from the tuple-lookup library's C ABI)
struct Lib {
    static std::string& error() { return g_error; }
    static bool ok(const pkb_statement* s, std::string& why) { return statement_ok(s, why); }
    static std::string pattern(const pkb_statement& s) { return io_pattern(s); }
};

}  // namespace pkb
