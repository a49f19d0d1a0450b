// wide_lane.hpp -- what one lane of the wide round kernel (wide.hip) does with one pair: term by term, the term's tables loaded and
// stepped through X = 0 .. D, the factors multiplied, c_t times the product added into D + 1 per-pair values, and those, times the eq
// weight, into the D + 1 running sums.  __host__ __device__: the suite runs it on the CPU at the value bound (pks_verify_asan wide lane).
//
// lane.hpp keeps every table of the statement in registers and picks a term's factors by compile-time index, which is why it is
// specialised on m and stops at 4 tables.  Here only one term's factors are live: at most D values and D steps, whatever m and T are,
// and the registers are indexed by the POSITION in the term's list (compile time), never by the table (run time).  A table that stands
// in k terms is loaded k times, the first time from memory and then from cache; a repeated index (a power) is loaded once.
//
// Every value stays below p, as in lane.hpp: fe_add / fe_sub / fe_mulx take and give reduced values.
#pragma once
#include "../../../include/provekit_sumcheck_wide.h"
#include "lane.hpp"

namespace pks {

// the statement's terms as the kernel takes them: the same for every lane (kernel arguments: scalar registers)
struct WideTerms {
    unsigned T;
    unsigned len[PKSW_MAX_TERMS];   // 1 .. D factors
    unsigned fac[PKSW_MAX_TERMS];   // factor i's table in bits 4 i .. 4 i + 3, non-decreasing in i
    unsigned kind[PKSW_MAX_TERMS];  // lane.hpp's COEFF_*
    fe coeff[PKSW_MAX_TERMS];       // Montgomery
};

// Host only; after statement_ok
inline WideTerms wide_terms(const pksw_statement& st) {
    WideTerms tm{};
    tm.T = st.T;
    for (unsigned t = 0; t < st.T; t++) {
        tm.len[t] = st.lens[t];
        for (unsigned i = 0; i < st.lens[t]; i++) tm.fac[t] |= st.factors[t][i] << (4 * i);
        memcpy(tm.coeff[t].v, st.coeffs[t], 32);
        tm.kind[t] = coeff_kind(tm.coeff[t]);
    }
    return tm;
}

// acc[X] += w * sum_t c_t prod_i f_{t,i}(X) for X = 0 .. D, f_j(X) = lo_j + X (hi_j - lo_j); load(j, lo, hi) gives table j's pair.
// weighted = false: w = 1.  Every branch on tm is uniform
template <int D, class Load>
PK_HD void wide_lane_accumulate(const WideTerms& tm, Load&& load, bool weighted, const fe& w, fe (&acc)[D + 1]) {
    fe pv[D + 1];
#pragma unroll
    for (int X = 0; X <= D; X++) pv[X] = pk::fe_zero();
#pragma unroll 1
    for (unsigned t = 0; t < tm.T; t++) {
        const unsigned len = tm.len[t], fac = tm.fac[t], kind = tm.kind[t];
        fe cur[D], step[D];
#pragma unroll
        for (int i = 0; i < D; i++) {
            if ((unsigned)i < len) {
                const unsigned j = (fac >> (4 * i)) & 15u;
                if (i > 0 && j == ((fac >> (4 * (i > 0 ? i - 1 : 0))) & 15u)) {  // a power: the same table again
                    cur[i] = cur[i > 0 ? i - 1 : 0];
                    step[i] = step[i > 0 ? i - 1 : 0];
                } else {
                    fe hi;
                    load(j, cur[i], hi);
                    step[i] = pk::fe_sub(hi, cur[i]);
                }
            }
        }
#pragma unroll
        for (int X = 0; X <= D; X++) {
            if (X > 0) {
#pragma unroll
                for (int i = 0; i < D; i++)
                    if ((unsigned)i < len) cur[i] = pk::fe_add(cur[i], step[i]);
            }
            fe prod = cur[0];
#pragma unroll
            for (int i = 1; i < D; i++)
                if ((unsigned)i < len) prod = pk::fe_mulx(prod, cur[i]);
            if (kind == COEFF_ONE)
                pv[X] = pk::fe_add(pv[X], prod);
            else if (kind == COEFF_MINUS_ONE)
                pv[X] = pk::fe_sub(pv[X], prod);
            else
                pv[X] = pk::fe_add(pv[X], pk::fe_mulx(tm.coeff[t], prod));
        }
    }
#pragma unroll
    for (int X = 0; X <= D; X++) acc[X] = pk::fe_add(acc[X], weighted ? pk::fe_mulx(pv[X], w) : pv[X]);
}

}  // namespace pks
