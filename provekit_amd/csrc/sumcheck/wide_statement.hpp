// wide_statement.hpp -- the wide statements (include/provekit_sumcheck_wide.h) next to statement.hpp's: which ones the library takes,
// their label, their terms' value at a point.  The same names as statement.hpp's, overloaded on the statement, so that what is written
// once for both (the verifier's walk in verify_host.cpp, the prover's round loop in prover.cpp) reads either.  Host only.
#pragma once
#include "../../../include/provekit_sumcheck_wide.h"
#include "statement.hpp"

namespace pks {

extern thread_local std::string g_wide_error;  // pksw_create_error
inline int refuse_wide(const std::string& why) { return pk::refuse(g_wide_error, why); }

// D = the longest list; after statement_ok
inline unsigned degree(const pksw_statement& s) {
    unsigned d = 0;
    for (unsigned t = 0; t < s.T; t++) d = std::max(d, s.lens[t]);
    return d;
}

inline bool statement_ok(const pksw_statement* s, std::string& why) {
    if (!s) return why = "null statement", false;
    if (s->n < 1 || s->n > PKS_MAX_VARS) return why = "n must be 1..28", false;
    if (s->m < 1 || s->m > PKSW_MAX_TABLES) return why = "m must be 1..16", false;
    if (s->T < 1 || s->T > PKSW_MAX_TERMS) return why = "T must be 1..16", false;
    if (s->has_tau > 1) return why = "has_tau must be 0 or 1", false;
    if (s->n_bind > PKS_MAX_BIND) return why = "n_bind must be 0..16", false;
    unsigned used = 0;
    for (unsigned t = 0; t < s->T; t++) {
        const std::string term = "term " + std::to_string(t);
        if (!s->lens[t]) return why = term + " has an empty list", false;
        if (s->lens[t] > PKSW_MAX_DEGREE) return why = term + " has more than 5 factors", false;
        for (unsigned i = 0; i < s->lens[t]; i++) {
            if (s->factors[t][i] >= s->m) return why = term + " names a table >= m", false;
            if (i && s->factors[t][i] < s->factors[t][i - 1]) return why = term + "'s list is not non-decreasing", false;
            used |= 1u << s->factors[t][i];
        }
        if (!pk::is_canonical(pk::h_load(s->coeffs[t]))) return why = "coefficient " + std::to_string(t) + " is not below p", false;
    }
    if (used != (1u << s->m) - 1) return why = "a table is used by no term", false;
    return true;
}

inline size_t proof_elems(const pksw_statement& s) { return 1 + (size_t)s.n * (degree(s) + 1) + s.m; }
inline size_t public_elems(const pksw_statement& s) { return (size_t)s.n_bind + (s.has_tau ? s.n : 0) + s.T; }

inline std::string io_pattern(const pksw_statement& s) {
    std::string d = "provekit-hip/sumcheck-wide/v1/n" + std::to_string(s.n) + "/m" + std::to_string(s.m) + "/T" + std::to_string(s.T) + "/tau" +
                    std::to_string(s.has_tau) + "/terms";
    for (unsigned t = 0; t < s.T; t++)
        for (unsigned i = 0; i < s.lens[t]; i++) d += (i ? "." : t ? "-" : "") + std::to_string(s.factors[t][i]);
    pattern_ops(d, s.n, s.m, s.T, s.has_tau, s.n_bind, degree(s));
    return d;
}

// sum_t c_t prod_i v_{f_{t,i}}
inline fe terms_at(const pksw_statement& s, const fe* v) {
    fe g = pk::fe_zero();
    for (unsigned t = 0; t < s.T; t++) {
        fe prod = pk::h_load(s.coeffs[t]);
        for (unsigned i = 0; i < s.lens[t]; i++) prod = pk::h_mul(prod, v[s.factors[t][i]]);
        g = pk::h_add(g, prod);
    }
    return g;
}

}  // namespace pks
