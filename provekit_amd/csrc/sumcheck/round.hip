// round.hip -- the one HIP kernel family libprovekit_sumcheck.so adds: "fold the previous round's variable and evaluate this round" of
// a product sumcheck over up to 4 tables in one pass (the fold_or_null shape of pk_sumcheck_cubic_round).
//
// A lane takes index x of the lower half and loads lo = f_j[x], hi = f_j[x + pairs] of each of the m tables (32 bytes each: two 16-byte
// loads).  With a fold challenge it loads both halves of the level above instead -- x, x + pairs, x + 2 pairs, x + 3 pairs -- folds them
// into lo and hi and writes those to the output tables, so each table is read once per round at its current length and written once at
// half; a lane writes only what it alone reads, so the output may be the input (the prover folds its arena in place; the caller's
// tables are only ever an input).  lane.hpp then steps every table through X = 0 .. D, forms the terms under wave-uniform control
// (masks, coefficient kinds and coefficients are kernel arguments: scalar registers) and multiplies by the lane's eq weight, the
// product of one entry of each of the two split tables (round.hpp).
//
// Reduction: the partials-plus-finish pattern of whir_pcs/evaluate.hip.  A workgroup adds its lanes' D + 1 sums with reduce.hpp's
// block_reduce_fe (column sums through LDS) and stores one partial per sum with ordinary vector stores; finish_kernel, one workgroup per
// sum, adds the partials.  No atomics, no ticket: field addition is exact, so the result's bits depend neither on the grid nor on
// the order.
//
// Specialised at compile time on what changes register pressure: D, m and whether the lane folds.  The term structure is uniform data.
//
// Device sets (shard.hpp): round_kernel_sharded is one rank's slice of a round, a sibling entry point of the same body (round_body)
// so that the lone instantiations' arguments and registers stay what they were.  Its lane index y runs over the rank's compacted
// pairs, and a slice policy states the two places where it differs: the input is either the caller's full tables, read at the rank's
// own indices expand(y) (rounds 0 and 1), or the rank's compacted arena, read at y (from round 2 on); and the eq weight is that of the
// global pair index expand(y).  Output and partials are the lone kernel's.
#include <hip/hip_runtime.h>

#include "../reduce.hpp"
#include "lane.hpp"
#include "round.hpp"
#include "shard.hpp"

using namespace pk;

namespace pks {

namespace {

constexpr unsigned THREADS = RED_THREADS;

struct DevTables {
    const fe* in[PKS_MAX_TABLES];
    fe* out[PKS_MAX_TABLES];
};

// Where a slice's pairs lie.  The lane index y runs over the slice's `pairs`; a policy gives the global pair index x (the eq weight's),
// the index the input tables are read at, the step between their halves (quarters, with a fold) and the index the output tables are
// stored at, their halves `pairs` apart.  The lone round is the identity
struct WholeRound {
    size_t pairs;
    __device__ size_t global(size_t y) const { return y; }
    __device__ size_t load(size_t y, size_t) const { return y; }
    __device__ size_t step() const { return pairs; }
    __device__ size_t store(size_t y) const { return y; }
};
// One rank's slice: `pairs` are the rank's own (the round's pairs / G), g and rank the ownership rule's.  in_global: the input tables
// are full tables at the round's global length, read at expand(y) with the halves G * pairs apart; otherwise compacted ones, read at y.
// The output tables are compacted either way
struct RankSlice {
    size_t pairs;
    unsigned g, rank;
    bool in_global;
    __device__ size_t global(size_t y) const { return pkss::expand(y, g, rank); }
    __device__ size_t load(size_t y, size_t x) const { return in_global ? x : y; }
    __device__ size_t step() const { return in_global ? pairs << g : pairs; }
    __device__ size_t store(size_t y) const { return y; }
};

// partial[k * gridDim.x + blockIdx.x] = this workgroup's share of sum k = h(k), k <= D
template <int D, int M, bool FOLD, class Slice>
__device__ __forceinline__ void round_body(const DevTables& tb, const Terms& tm, const fe* __restrict__ eq_hi, const fe* __restrict__ eq_lo, unsigned lo_bits,
                                           const Slice sl, const fe& alpha, fe* __restrict__ partial) {
    fe acc[D + 1];
#pragma unroll
    for (int k = 0; k <= D; k++) acc[k] = fe_zero();
    const bool weighted = eq_hi != nullptr;
    const size_t lo_mask = ((size_t)1 << lo_bits) - 1;
    const size_t stride = (size_t)gridDim.x * THREADS;
    const size_t step = sl.step();
    for (size_t y = (size_t)blockIdx.x * THREADS + threadIdx.x; y < sl.pairs; y += stride) {
        const size_t x = sl.global(y);
        const size_t at = sl.load(y, x), to = sl.store(y);
        fe lo[M], hi[M];
#pragma unroll
        for (int j = 0; j < M; j++) {
            const fe* f = tb.in[j] + at;
            fe x0 = fe_load(f), x1 = fe_load(f + step);
            if (FOLD) {
                const fe x2 = fe_load(f + 2 * step), x3 = fe_load(f + 3 * step);
                x0 = fold_pair(x0, x2, alpha);
                x1 = fold_pair(x1, x3, alpha);
                fe_store(tb.out[j] + to, x0);
                fe_store(tb.out[j] + to + sl.pairs, x1);
            }
            lo[j] = x0;
            hi[j] = x1;
        }
        fe w = fe_zero();
        if (weighted) w = fe_mulx(fe_load(eq_hi + (x >> lo_bits)), fe_load(eq_lo + (x & lo_mask)));
        lane_accumulate<D, M>(lo, hi, tm, weighted, w, acc);
    }
    const fe mine = block_reduce_fe<D + 1>(acc);  // thread k holds sum k
    if (threadIdx.x <= D) fe_store(partial + (size_t)threadIdx.x * gridDim.x + blockIdx.x, mine);
}

template <int D, int M, bool FOLD>
__global__ __launch_bounds__(THREADS) void round_kernel(DevTables tb, Terms tm, const fe* __restrict__ eq_hi, const fe* __restrict__ eq_lo, unsigned lo_bits,
                                                        size_t pairs, fe alpha, fe* __restrict__ partial) {
    round_body<D, M, FOLD>(tb, tm, eq_hi, eq_lo, lo_bits, WholeRound{pairs}, alpha, partial);
}

template <int D, int M, bool FOLD>
__global__ __launch_bounds__(THREADS) void round_kernel_sharded(DevTables tb, Terms tm, const fe* __restrict__ eq_hi, const fe* __restrict__ eq_lo,
                                                                unsigned lo_bits, size_t pairs, unsigned g, unsigned rank, bool in_global, fe alpha,
                                                                fe* __restrict__ partial) {
    round_body<D, M, FOLD>(tb, tm, eq_hi, eq_lo, lo_bits, RankSlice{pairs, g, rank, in_global}, alpha, partial);
}

// The hand-over: gathered = G blocks of m tables of 2^(c+1) elements, block r rank r's lower-half and upper-half chunks; out = the m
// tables in global order, `out_stride` elements apart.  One lane per element
__global__ __launch_bounds__(THREADS) void handover_kernel(const fe* __restrict__ gathered, unsigned m, unsigned g, fe* __restrict__ out, size_t out_stride) {
    const size_t local = (size_t)2 << pkss::C, total = ((size_t)m * local) << g;
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const size_t y = i % local, j = (i / local) % m;
    const unsigned r = (unsigned)(i / (local * m));
    fe_store(out + j * out_stride + pkss::expand(y, g, r), fe_load(gathered + i));
}

// out[k] = the sum of partial[k * n_wg ..+ n_wg); one workgroup per sum, lane j adds the partials j, j + 256, ...
__global__ __launch_bounds__(THREADS) void finish_kernel(const fe* __restrict__ partial, unsigned n_wg, fe* __restrict__ out) {
    const fe* p = partial + (size_t)blockIdx.x * n_wg;
    fe acc = fe_zero();
    for (unsigned j = threadIdx.x; j < n_wg; j += THREADS) acc = fe_add(acc, fe_load(p + j));
    acc = block_sum(acc);
    if (threadIdx.x == 0) fe_store(out + blockIdx.x, acc);
}

// `sh` null: the lone round
template <int D, int M, bool FOLD>
void launch_dmf(unsigned grid, hipStream_t stream, const DevTables& tb, const Terms& tm, const fe* eq_hi, const fe* eq_lo, unsigned lo_bits, size_t pairs,
                const ShardSlice* sh, const fe& alpha, fe* partial) {
    if (sh)
        round_kernel_sharded<D, M, FOLD><<<grid, THREADS, 0, stream>>>(tb, tm, eq_hi, eq_lo, lo_bits, pairs, sh->g, sh->rank, sh->in_global, alpha, partial);
    else
        round_kernel<D, M, FOLD><<<grid, THREADS, 0, stream>>>(tb, tm, eq_hi, eq_lo, lo_bits, pairs, alpha, partial);
}

}  // namespace

unsigned round_grid(size_t pairs) {
    const size_t need = (pairs + 2 * THREADS - 1) / (2 * THREADS);
    return (unsigned)(need < 1 ? 1 : need > PKS_MAX_GRID ? PKS_MAX_GRID : need);
}

namespace {

// the two launches' common part: `shard` null is the lone round
int launch(hipStream_t stream, const pks_statement& st, const RoundTables& rt, size_t pairs, const uint64_t* fold_or_null, const uint64_t* d_eq_hi,
           const uint64_t* d_eq_lo, unsigned lo_bits, unsigned grid, uint64_t* d_scratch, const ShardSlice* shard) {
    if (!pairs || grid < 1 || grid > PKS_MAX_GRID) return PK_ERR_BAD_ARG;
    DevTables tb{};
    for (unsigned j = 0; j < st.m; j++) {
        tb.in[j] = (const fe*)rt.in[j];
        tb.out[j] = (fe*)rt.out[j];
    }
    Terms tm{};
    tm.T = st.T;
    for (unsigned t = 0; t < st.T; t++) {
        tm.masks[t] = st.masks[t];
        tm.coeff[t] = h_load(st.coeffs[t]);
        tm.kind[t] = coeff_kind(tm.coeff[t]);
    }
    const fe alpha = fold_or_null ? h_load(fold_or_null) : fe_zero();
    fe* const partial = (fe*)d_scratch;
    const fe *hi = (const fe*)d_eq_hi, *lo = (const fe*)d_eq_lo;
    const unsigned D = degree(st);
    const bool fold = fold_or_null != nullptr;
#define PKS_CASE(DEG, TABLES)                                                                                    \
    if (D == DEG && st.m == TABLES) {                                                                            \
        if (fold)                                                                                                \
            launch_dmf<DEG, TABLES, true>(grid, stream, tb, tm, hi, lo, lo_bits, pairs, shard, alpha, partial);  \
        else                                                                                                     \
            launch_dmf<DEG, TABLES, false>(grid, stream, tb, tm, hi, lo, lo_bits, pairs, shard, alpha, partial); \
    } else
    PKS_CASE(1, 1) PKS_CASE(1, 2) PKS_CASE(1, 3) PKS_CASE(1, 4) PKS_CASE(2, 2) PKS_CASE(2, 3) PKS_CASE(2, 4) PKS_CASE(3, 3) PKS_CASE(3, 4)
    return PK_ERR_BAD_ARG;  // D <= m: a term's tables are distinct
#undef PKS_CASE
    return finish_launch(stream, d_scratch, grid, D + 1, d_scratch + 4 * results_at(st));
}

}  // namespace

int finish_launch(hipStream_t stream, const uint64_t* d_partial, unsigned n_wg, unsigned sums, uint64_t* d_out) {
    finish_kernel<<<sums, THREADS, 0, stream>>>((const fe*)d_partial, n_wg, (fe*)d_out);
    return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP;
}

int round_launch(hipStream_t stream, const pks_statement& st, const RoundTables& rt, size_t pairs, const uint64_t* fold_or_null, const uint64_t* d_eq_hi,
                 const uint64_t* d_eq_lo, unsigned lo_bits, unsigned grid, uint64_t* d_scratch) {
    return launch(stream, st, rt, pairs, fold_or_null, d_eq_hi, d_eq_lo, lo_bits, grid, d_scratch, nullptr);
}

int round_shard_launch(hipStream_t stream, const pks_statement& st, const RoundTables& rt, size_t pairs, const uint64_t* fold_or_null, const uint64_t* d_eq_hi,
                       const uint64_t* d_eq_lo, unsigned lo_bits, unsigned grid, uint64_t* d_scratch, const ShardSlice& shard) {
    // whole chunks only: every index the slice reads lies inside the round's tables because expand() of a whole chunk does
    if (shard.g < 1 || shard.g > PKSS_MAX_WORLD_LOG2 || shard.rank >> shard.g || pairs % ((size_t)1 << pkss::C)) return PK_ERR_BAD_ARG;
    return launch(stream, st, rt, pairs, fold_or_null, d_eq_hi, d_eq_lo, lo_bits, grid, d_scratch, &shard);
}

int handover_launch(hipStream_t stream, const uint64_t* d_gathered, unsigned m, unsigned g, uint64_t* d_out, size_t out_stride) {
    if (m < 1 || m > PKS_MAX_TABLES || g < 1 || g > PKSS_MAX_WORLD_LOG2 || out_stride < pkss::handover_len(g)) return PK_ERR_BAD_ARG;
    const size_t total = ((size_t)m * ((size_t)2 << pkss::C)) << g;
    handover_kernel<<<(unsigned)(total / THREADS), THREADS, 0, stream>>>((const fe*)d_gathered, m, g, (fe*)d_out, out_stride);
    return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP;
}

}  // namespace pks
