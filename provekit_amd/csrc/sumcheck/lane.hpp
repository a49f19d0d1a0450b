// lane.hpp -- what one lane of the round kernel (round.hip) does with one pair: the m tables' values stepped through X = 0 .. D, the
// terms formed at each X, the eq weight, the D + 1 running sums.  __host__ __device__: the suite runs it on the CPU at the value bound
// (tests/test_prodcheck_host.py through pks_verify_asan).
//
// Every value stays below p: fe_add / fe_sub / fe_mulx take and give reduced values, so a stepped value f(X) = f(X-1) + (hi - lo) is
// reduced at each step and nothing here relies on dot29's lazily reduced column sums (whose first factor must be below p).
#pragma once
#include "../fe29.hpp"

namespace pks {

using pk::fe;

// the statement's terms as the kernel takes them: the same for every lane (kernel arguments: scalar registers).  kind: how the
// coefficient enters -- most statements have only 1 and -1, which cost no product
enum { COEFF_ANY = 0, COEFF_ONE = 1, COEFF_MINUS_ONE = 2 };
struct Terms {
    unsigned T;
    unsigned masks[4];
    unsigned kind[4];
    fe coeff[4];  // Montgomery
};

// the kind of a coefficient (Montgomery, below p), stated once for the kernel's caller (round.hip) and the sanitizer driver.  Host only
inline unsigned coeff_kind(const fe& c) {
    return pk::fe_eq(c, pk::fe_one()) ? COEFF_ONE : pk::fe_eq(c, pk::fe_neg(pk::fe_one())) ? COEFF_MINUS_ONE : COEFF_ANY;
}

// acc[X] += w * sum_t c_t prod_{j in S_t} f_j(X) for X = 0 .. D, f_j(X) = lo[j] + X (hi[j] - lo[j]).  weighted = false: w = 1
template <int D, int M>
PK_HD void lane_accumulate(const fe (&lo)[M], const fe (&hi)[M], const Terms& tm, bool weighted, const fe& w, fe (&acc)[D + 1]) {
    fe cur[M], step[M];
#pragma unroll
    for (int j = 0; j < M; j++) {
        cur[j] = lo[j];
        step[j] = pk::fe_sub(hi[j], lo[j]);
    }
#pragma unroll
    for (int X = 0; X <= D; X++) {
        if (X > 0) {
#pragma unroll
            for (int j = 0; j < M; j++) cur[j] = pk::fe_add(cur[j], step[j]);
        }
        fe g = pk::fe_zero();
#pragma unroll 1
        for (unsigned t = 0; t < tm.T; t++) {  // uniform: the masks and kinds are the same in every lane
            const unsigned mask = tm.masks[t];
            fe prod = pk::fe_zero();
            bool first = true;
#pragma unroll
            for (int j = 0; j < M; j++) {
                if ((mask >> j) & 1) {
                    prod = first ? cur[j] : pk::fe_mulx(prod, cur[j]);
                    first = false;
                }
            }
            const unsigned kind = tm.kind[t];
            if (kind == COEFF_ONE)
                g = pk::fe_add(g, prod);
            else if (kind == COEFF_MINUS_ONE)
                g = pk::fe_sub(g, prod);
            else
                g = pk::fe_add(g, pk::fe_mulx(tm.coeff[t], prod));
        }
        if (weighted) g = pk::fe_mulx(g, w);
        acc[X] = pk::fe_add(acc[X], g);
    }
}

// one variable bound: lo + r (hi - lo)
PK_HD fe fold_pair(const fe& lo, const fe& hi, const fe& r) { return pk::fe_add(lo, pk::fe_mulx(r, pk::fe_sub(hi, lo))); }

}  // namespace pks
