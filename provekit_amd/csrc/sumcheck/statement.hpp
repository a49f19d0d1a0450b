// statement.hpp -- what the sources of libprovekit_sumcheck.so share on the host: which statements the library takes, the IO pattern
// of a proof, the terms' value at a point and the round polynomial's value at a challenge.  Host only; no device, no product call.
#pragma once
#include <string>

#include "../../../include/provekit_sumcheck.h"
#include "../argument.hpp"

namespace pks {

using pk::fe;

extern thread_local std::string g_error;  // pks_create_error
inline int refuse(const std::string& why) { return pk::refuse(g_error, why); }

inline unsigned popcount4(unsigned mask) { return (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1); }

// D = max |S_t|; after statement_ok
inline unsigned degree(const pks_statement& s) {
    unsigned d = 0;
    for (unsigned t = 0; t < s.T; t++) d = std::max(d, popcount4(s.masks[t]));
    return d;
}

inline bool statement_ok(const pks_statement* s, std::string& why) {
    if (!s) return why = "null statement", false;
    if (s->n < 1 || s->n > PKS_MAX_VARS) return why = "n must be 1..28", false;
    if (s->m < 1 || s->m > PKS_MAX_TABLES) return why = "m must be 1..4", false;
    if (s->T < 1 || s->T > PKS_MAX_TERMS) return why = "T must be 1..4", false;
    if (s->has_tau > 1) return why = "has_tau must be 0 or 1", false;
    if (s->n_bind > PKS_MAX_BIND) return why = "n_bind must be 0..16", false;
    unsigned used = 0;
    for (unsigned t = 0; t < s->T; t++) {
        const unsigned mask = s->masks[t];
        if (!mask) return why = "term " + std::to_string(t) + " has an empty mask", false;
        if (mask >> s->m) return why = "term " + std::to_string(t) + " names a table >= m", false;
        if (popcount4(mask) > PKS_MAX_TERM_TABLES) return why = "term " + std::to_string(t) + " has more than 3 tables", false;
        if (!pk::is_canonical(pk::h_load(s->coeffs[t]))) return why = "coefficient " + std::to_string(t) + " is not below p", false;
        used |= mask;
    }
    if (used != (1u << s->m) - 1) return why = "a table is used by no term", false;
    return true;
}

// the proof: s, n x (D + 1) round values, m final values
inline size_t proof_elems(const pks_statement& s) { return 1 + (size_t)s.n * (degree(s) + 1) + s.m; }
// what both sides absorb before it: bind, tau, the coefficients
inline size_t public_elems(const pks_statement& s) { return (size_t)s.n_bind + (s.has_tau ? s.n : 0) + s.T; }

// the operations behind a label, for every statement of this library (pks and the wide pksw): absorb n_bind caller elements, tau if
// given, the T coefficients and s; per round absorb D + 1 values and squeeze one challenge; absorb the m final values
inline void pattern_ops(std::string& d, unsigned n, unsigned m, unsigned T, unsigned has_tau, unsigned n_bind, unsigned D) {
    auto A = [&](size_t k, const char* label) { pk::pattern_op(d, 'A', k, label); };
    A(n_bind, "bind");
    if (has_tau) A(n, "tau");
    A(T, "coefficients");
    A(1, "sum");
    for (unsigned i = 0; i < n; i++) {
        A(D + 1, "round_values");
        d.push_back('\0');
        d += "S1challenge";
    }
    A(m, "final_values");
}

inline std::string io_pattern(const pks_statement& s) {
    std::string d = "provekit-hip/sumcheck/v1/n" + std::to_string(s.n) + "/m" + std::to_string(s.m) + "/T" + std::to_string(s.T) + "/tau" +
                    std::to_string(s.has_tau) + "/masks";
    for (unsigned t = 0; t < s.T; t++) d += (t ? "." : "") + std::to_string(s.masks[t]);
    pattern_ops(d, s.n, s.m, s.T, s.has_tau, s.n_bind, degree(s));
    return d;
}

// sum_t c_t prod_{j in S_t} v_j
inline fe terms_at(const pks_statement& s, const fe* v) {
    fe g = pk::fe_zero();
    for (unsigned t = 0; t < s.T; t++) {
        fe prod = pk::h_load(s.coeffs[t]);
        for (unsigned j = 0; j < s.m; j++)
            if ((s.masks[t] >> j) & 1) prod = pk::h_mul(prod, v[j]);
        g = pk::h_add(g, prod);
    }
    return g;
}

// the most values a round sends: D + 1 at the wide statements' D = 5 (provekit_sumcheck_wide.h)
constexpr unsigned MAX_ROUND_VALUES = 6;

// the polynomial of degree <= D through h(0) .. h(D) at x, D = 1 .. 5 (Lagrange over the nodes 0 .. D)
inline fe round_poly_at(const fe* h, unsigned D, const fe& x) {
    // 1/6 canonical: (5 p + 1) / 6
    static const uint64_t INV6[4] = {0xb891a1fb48000001ULL, 0x4c2b4191bac53323ULL, 0xc442e4c2c1411ef8ULL, 0x285396b510feb022ULL};
    const fe one = pk::fe_one(), half = pk::h_half(), sixth = pk::h_from_canon(pk::h_load(INV6));
    const fe x1 = pk::h_sub(x, one), x2 = pk::h_sub(x1, one), x3 = pk::h_sub(x2, one);
    if (D == 1) return pk::h_add(h[0], pk::h_mul(x, pk::h_sub(h[1], h[0])));
    if (D == 2) {
        // h0 (x-1)(x-2)/2 - h1 x (x-2) + h2 x (x-1)/2
        const fe a = pk::h_mul(pk::h_mul(h[0], half), pk::h_mul(x1, x2)), b = pk::h_mul(h[1], pk::h_mul(x, x2)),
                 c = pk::h_mul(pk::h_mul(h[2], half), pk::h_mul(x, x1));
        return pk::h_add(pk::h_sub(a, b), c);
    }
    if (D == 3) {
        // -h0 (x-1)(x-2)(x-3)/6 + h1 x (x-2)(x-3)/2 - h2 x (x-1)(x-3)/2 + h3 x (x-1)(x-2)/6
        const fe a = pk::h_mul(pk::h_mul(h[0], sixth), pk::h_mul(pk::h_mul(x1, x2), x3)), b = pk::h_mul(pk::h_mul(h[1], half), pk::h_mul(pk::h_mul(x, x2), x3)),
                 c = pk::h_mul(pk::h_mul(h[2], half), pk::h_mul(pk::h_mul(x, x1), x3)), e = pk::h_mul(pk::h_mul(h[3], sixth), pk::h_mul(pk::h_mul(x, x1), x2));
        return pk::h_add(pk::h_sub(b, a), pk::h_sub(e, c));
    }
    // D = 4, 5: sum_k h_k (-1)^(D-k) / (k! (D-k)!) prod_{j != k} (x - j).  1/5 canonical: (2 p + 1) / 5
    static const uint64_t INV5[4] = {0xe7f3fbd4c6666667ULL, 0xa9ae5ce9ca4a2d06ULL, 0x49b9b57c33cd568bULL, 0x135b52945a13d9aaULL};
    fe inv_fact[MAX_ROUND_VALUES] = {one, one, half, sixth, pk::h_mul(sixth, pk::h_mul(half, half)), one};
    inv_fact[5] = pk::h_mul(inv_fact[4], pk::h_from_canon(pk::h_load(INV5)));
    fe xs[MAX_ROUND_VALUES] = {x, x1, x2, x3, pk::h_sub(x3, one), one};
    xs[5] = pk::h_sub(xs[4], one);
    fe total = pk::fe_zero();
    for (unsigned k = 0; k <= D; k++) {
        fe term = pk::h_mul(h[k], pk::h_mul(inv_fact[k], inv_fact[D - k]));
        for (unsigned j = 0; j <= D; j++)
            if (j != k) term = pk::h_mul(term, xs[j]);
        total = (D - k) & 1 ? pk::h_sub(total, term) : pk::h_add(total, term);
    }
    return total;
}

// eq(t, r) = t r + (1 - t)(1 - r)
inline fe eq1(const fe& t, const fe& r) {
    const fe tr = pk::h_mul(t, r);
    return pk::h_sub(pk::h_add(pk::h_add(tr, tr), pk::fe_one()), pk::h_add(t, r));
}

}  // namespace pks
