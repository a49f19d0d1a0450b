// round.hpp -- the launches of round.hip and the host half of the split eq weights, for prover.cpp (pks_prove, pks_round).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "wide_statement.hpp"

namespace pks {

// ---- the split eq weights ------------------------------------------------------------------------------------------------------
// The weight of pair x' in the round that binds variable i is eq(tau_{>i}, x').  With t = tau_{>0} (R = n - 1 coordinates), H = R - L
// leading and L = R / 2 trailing ones, it is  HI_i[x' >> lo_bits] * LO_i[x' & (2^lo_bits - 1)]  where
//     i <= H:  HI_i = eq(t[i .. H), .),  LO_i = eq(t[H .. R), .),      lo_bits = L
//     i >  H:  HI_i = {1},               LO_i = eq(t[i .. R), .),      lo_bits = R - i.
// So the suffix levels of the two halves are all a proof needs: 2^(H+1) + 2^(L+1) - 2 elements -- 48 Ki for n = 28, where one
// full-size table would be 2^27 -- built on the host per proof and never folded.  The levels of a k-coordinate point sit back to back,
// level j (over coordinates j .. k) at 2^(k+1) - 2^(k-j+1), the last one {1}.
struct EqSplit {
    unsigned R = 0, H = 0, L = 0;
    size_t fes() const { return ((size_t)2 << H) + ((size_t)2 << L) - 2; }
    size_t level(unsigned k, unsigned j) const { return ((size_t)2 << k) - ((size_t)2 << (k - j)); }
    // offsets (in elements) of round i's tables inside the buffer, and its lo_bits
    void round(unsigned i, size_t& hi, size_t& lo, unsigned& lo_bits) const {
        const size_t lo_base = ((size_t)2 << H) - 1;
        if (i <= H) {
            hi = level(H, i), lo = lo_base + level(L, 0), lo_bits = L;
        } else {
            hi = level(H, H), lo = lo_base + level(L, i - H), lo_bits = R - i;
        }
    }
};
inline EqSplit eq_split(unsigned R) {
    EqSplit s;
    s.R = R, s.L = R / 2, s.H = R - s.L;
    return s;
}
inline void eq_levels(const fe* x, unsigned k, fe* out) {  // 2^(k+1) - 1 elements
    const size_t total = ((size_t)2 << k) - 1;
    out[total - 1] = pk::fe_one();
    for (unsigned j = k; j >= 1; j--) {  // level j - 1 from level j
        const size_t h = (size_t)1 << (k - j);
        const fe* in = out + (((size_t)2 << k) - ((size_t)2 << (k - j)));
        fe* o = out + (((size_t)2 << k) - ((size_t)2 << (k - j + 1)));
        for (size_t y = 0; y < h; y++) {
            const fe up = pk::h_mul(in[y], x[j - 1]);
            o[h + y] = up;
            o[y] = pk::h_sub(in[y], up);
        }
    }
}
inline void eq_split_build(const EqSplit& s, const fe* t, std::vector<fe>& buf) {
    buf.resize(s.fes());
    eq_levels(t, s.H, buf.data());
    eq_levels(t + s.H, s.L, buf.data() + (((size_t)2 << s.H) - 1));
}

// ---- the kernel ----------------------------------------------------------------------------------------------------------------
struct RoundTables {  // of either statement: the first m
    const uint64_t* in[PKSW_MAX_TABLES];
    uint64_t* out[PKSW_MAX_TABLES];  // fold only
};
// the library's grid for a round of `pairs` pairs: two pairs per lane, at most PKS_MAX_GRID workgroups of 256
unsigned round_grid(size_t pairs);
// scratch for one round's partial sums and its results, in field elements
constexpr size_t ROUND_SCRATCH_FES = (size_t)4 * PKS_MAX_GRID + 8;
// a lone prover's arena in field elements: the m folded copies of half length, one round's scratch and the split eq weights.  What
// pks_prover_create allocates; libprovekit_lookup.so states its two provers' share from the same rule (pkl_prover_arena_bytes).
inline size_t lone_arena_fes(unsigned n, unsigned m) { return (size_t)m * ((size_t)1 << (n - 1)) + ROUND_SCRATCH_FES + eq_split(n - 1).fes(); }
// Enqueue on `stream`: the round of `pairs` pairs (tables of 2 * pairs elements; with a fold: of 4 * pairs, folded first into tb.out),
// the D + 1 sums to d_scratch[4 * PKS_MAX_GRID ..).  d_eq_hi == nullptr: weight 1.  The sums are the workgroups' partials
// (d_scratch[k * grid + workgroup]) added by a finish kernel: field addition is exact, so the bits do not depend on the grid.
int round_launch(hipStream_t stream, const pks_statement& st, const RoundTables& tb, size_t pairs, const uint64_t* fold_or_null, const uint64_t* d_eq_hi,
                 const uint64_t* d_eq_lo, unsigned lo_bits, unsigned grid, uint64_t* d_scratch);

// out[k] = the sum of d_partial[k * n_wg ..+ n_wg) for k < sums: the finish of every round launch, round.hip's and wide.hip's
int finish_launch(hipStream_t stream, const uint64_t* d_partial, unsigned n_wg, unsigned sums, uint64_t* d_out);

// ---- the wide statements (wide.hip) ----------------------------------------------------------------------------------------------
// a wide round's scratch: up to MAX_ROUND_VALUES partial sums per workgroup, then the results
constexpr size_t WIDE_SCRATCH_FES = (size_t)MAX_ROUND_VALUES * PKS_MAX_GRID + 8;
// Where a round's D + 1 sums arrive inside its scratch, in field elements; the scratch's size
inline size_t results_at(const pks_statement&) { return (size_t)4 * PKS_MAX_GRID; }
inline size_t results_at(const pksw_statement&) { return (size_t)MAX_ROUND_VALUES * PKS_MAX_GRID; }
inline size_t scratch_fes(const pks_statement&) { return ROUND_SCRATCH_FES; }
inline size_t scratch_fes(const pksw_statement&) { return WIDE_SCRATCH_FES; }
// round_launch for a wide statement: the same arguments, the sums to d_scratch[results_at ..)
int round_launch(hipStream_t stream, const pksw_statement& st, const RoundTables& tb, size_t pairs, const uint64_t* fold_or_null, const uint64_t* d_eq_hi,
                 const uint64_t* d_eq_lo, unsigned lo_bits, unsigned grid, uint64_t* d_scratch);

// ---- device sets (shard.hpp) -----------------------------------------------------------------------------------------------------
// one rank's slice of a round: G = 2^g ranks, this is `rank`; in_global: the input tables are full tables at the round's global
// length (the caller's, rounds 0 and 1), read at the rank's own indices; otherwise the rank's compacted ones.  Output tables are compacted
struct ShardSlice {
    unsigned g, rank;
    bool in_global;
};
// round_launch for a slice: `pairs` the rank's own pairs (the round's / G, whole chunks), eq tables the round's, indexed by the global
// pair index; the rank's D + 1 partial sums to d_scratch[4 * PKS_MAX_GRID ..)
int round_shard_launch(hipStream_t stream, const pks_statement& st, const RoundTables& tb, size_t pairs, const uint64_t* fold_or_null, const uint64_t* d_eq_hi,
                       const uint64_t* d_eq_lo, unsigned lo_bits, unsigned grid, uint64_t* d_scratch, const ShardSlice& shard);
// a wide statement has no slices (provekit_sumcheck_wide.h: device sets are out of scope); the round loop never asks for one
inline int round_shard_launch(hipStream_t, const pksw_statement&, const RoundTables&, size_t, const uint64_t*, const uint64_t*, const uint64_t*, unsigned, unsigned,
                              uint64_t*, const ShardSlice&) {
    return PK_ERR_BAD_ARG;
}
// the hand-over: d_gathered = G blocks (rank order) of m tables of 2^(c+1) elements -> d_out[j * out_stride + x], the m tables of
// 2^(c+g+1) in global order
int handover_launch(hipStream_t stream, const uint64_t* d_gathered, unsigned m, unsigned g, uint64_t* d_out, size_t out_stride);

}  // namespace pks
