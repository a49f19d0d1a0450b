// wide.hip -- the round kernel of the wide statements (include/provekit_sumcheck_wide.h): "fold the previous round's variable and
// evaluate this round" over up to 16 tables and 16 terms of degree up to 5, in one pass.
//
// round.hip's kernel keeps lo and hi of every table in registers and is specialised on (D, m); at (3, 4) it already stands at the
// register file's edge, so sixteen tables need another shape.  This one is specialised on D and on whether the lane folds, and takes m,
// T, the factor lists, the coefficients and their kinds and the table pointers as kernel arguments (scalar registers).  Per pair:
//   1. with a fold, a loop over the tables: the four quarter-points x, x + pairs, x + 2 pairs, x + 3 pairs are loaded, folded by the
//      previous challenge into lo and hi and stored to the output tables.  A lane writes only what it alone reads, so the output may be
//      the input, as in round.hip (the prover folds its arena in place; the caller's tables are only ever an input);
//   2. a loop over the terms (wide_lane.hpp): the term's distinct tables are loaded -- from the output tables the lane has just
//      written, or from the caller's without a fold --, stepped through X = 0 .. D, multiplied, and c_t times the product is added into
//      D + 1 per-pair values.  Only one term's factors are live, and no register is picked by a run-time index;
//   3. one product by the split eq weight per X (round.hpp).
// Every loop over tables and terms runs under uniform control.  A table that stands in k terms is read k times per round, once from
// memory and then from cache.
//
// Reduction: round.hip's.  A workgroup adds its lanes' D + 1 sums with reduce.hpp's block_reduce_fe and stores one partial per sum;
// round.hip's finish kernel adds the partials.  No atomics, no ticket: the bits depend neither on the grid nor on the order.
#include <hip/hip_runtime.h>

#include "../reduce.hpp"
#include "round.hpp"
#include "wide_lane.hpp"

using namespace pk;

namespace pks {

namespace {

constexpr unsigned THREADS = RED_THREADS;

struct WideTables {
    const fe* in[PKSW_MAX_TABLES];
    fe* out[PKSW_MAX_TABLES];  // fold only
    unsigned m;
};

// partial[k * gridDim.x + blockIdx.x] = this workgroup's share of sum k = h(k), k <= D
template <int D, bool FOLD>
__global__ __launch_bounds__(THREADS) void wide_round_kernel(WideTables tb, WideTerms tm, const fe* __restrict__ eq_hi, const fe* __restrict__ eq_lo,
                                                             unsigned lo_bits, size_t pairs, fe alpha, fe* __restrict__ partial) {
    fe acc[D + 1];
#pragma unroll
    for (int k = 0; k <= D; k++) acc[k] = fe_zero();
    const bool weighted = eq_hi != nullptr;
    const size_t lo_mask = ((size_t)1 << lo_bits) - 1;
    const size_t stride = (size_t)gridDim.x * THREADS;
    for (size_t x = (size_t)blockIdx.x * THREADS + threadIdx.x; x < pairs; x += stride) {
        if (FOLD) {
#pragma unroll 1
            for (unsigned j = 0; j < tb.m; j++) {
                const fe* f = tb.in[j] + x;
                const fe x0 = fe_load(f), x1 = fe_load(f + pairs), x2 = fe_load(f + 2 * pairs), x3 = fe_load(f + 3 * pairs);
                fe* o = tb.out[j] + x;
                fe_store(o, fold_pair(x0, x2, alpha));
                fe_store(o + pairs, fold_pair(x1, x3, alpha));
            }
        }
        fe w = fe_zero();
        if (weighted) w = fe_mulx(fe_load(eq_hi + (x >> lo_bits)), fe_load(eq_lo + (x & lo_mask)));
        auto load = [&](unsigned j, fe& lo, fe& hi) {
            const fe* f = (FOLD ? tb.out[j] : tb.in[j]) + x;
            lo = fe_load(f);
            hi = fe_load(f + pairs);
        };
        wide_lane_accumulate<D>(tm, load, weighted, w, acc);
    }
    const fe mine = block_reduce_fe<D + 1>(acc);  // thread k holds sum k
    if (threadIdx.x <= D) fe_store(partial + (size_t)threadIdx.x * gridDim.x + blockIdx.x, mine);
}

template <int D>
void launch_d(bool fold, unsigned grid, hipStream_t stream, const WideTables& tb, const WideTerms& tm, const fe* eq_hi, const fe* eq_lo, unsigned lo_bits,
              size_t pairs, const fe& alpha, fe* partial) {
    if (fold)
        wide_round_kernel<D, true><<<grid, THREADS, 0, stream>>>(tb, tm, eq_hi, eq_lo, lo_bits, pairs, alpha, partial);
    else
        wide_round_kernel<D, false><<<grid, THREADS, 0, stream>>>(tb, tm, eq_hi, eq_lo, lo_bits, pairs, alpha, partial);
}

}  // namespace

int round_launch(hipStream_t stream, const pksw_statement& st, const RoundTables& rt, size_t pairs, const uint64_t* fold_or_null, const uint64_t* d_eq_hi,
                 const uint64_t* d_eq_lo, unsigned lo_bits, unsigned grid, uint64_t* d_scratch) {
    if (!pairs || grid < 1 || grid > PKS_MAX_GRID) return PK_ERR_BAD_ARG;
    WideTables tb{};
    tb.m = st.m;
    for (unsigned j = 0; j < st.m; j++) {
        tb.in[j] = (const fe*)rt.in[j];
        tb.out[j] = (fe*)rt.out[j];
    }
    const WideTerms tm = wide_terms(st);
    const fe alpha = fold_or_null ? h_load(fold_or_null) : fe_zero();
    fe* const partial = (fe*)d_scratch;
    const fe *hi = (const fe*)d_eq_hi, *lo = (const fe*)d_eq_lo;
    const unsigned D = degree(st);
    const bool fold = fold_or_null != nullptr;
#define PKSW_DEGREE(DEG) \
    if (D == DEG) launch_d<DEG>(fold, grid, stream, tb, tm, hi, lo, lo_bits, pairs, alpha, partial); else
    PKSW_DEGREE(1) PKSW_DEGREE(2) PKSW_DEGREE(3) PKSW_DEGREE(4) PKSW_DEGREE(5)
    return PK_ERR_BAD_ARG;
#undef PKSW_DEGREE
    return finish_launch(stream, d_scratch, grid, D + 1, d_scratch + 4 * results_at(st));
}

}  // namespace pks
