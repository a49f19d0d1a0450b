// linear.hpp -- the launches of linear.hip: the weighted sums of a linear statement and the one-pass combination of its weight
// tables, for pcs.cpp (pkw_open_linear runs them on the scheme's stream with arena scratch) and for tools/probes.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/provekit_whir.h"

namespace pkw {

constexpr unsigned WSUM_LOW_VARS = 8;  // a workgroup covers 2^8 contiguous elements per step, one per lane
constexpr unsigned WSUM_MAX_WG = 512;  // the grid's x extent: two resident workgroups per compute unit at two waves per SIMD
constexpr unsigned WSUM_PASS = 8;      // weights per launch: the partials of a pass are batch * WSUM_PASS * grid elements
constexpr unsigned WSUM_MAX_BATCH = 4;
constexpr unsigned WSUM_TILE_B = 2, WSUM_TILE_W = 2;  // the register tile for batch >= 2; one polynomial takes 1 x 4
constexpr unsigned COMB_TILE = 16;     // weights per pass of the combination kernel (= PKW_MAX_WEIGHTS: pkw_open_linear makes one)

// the grid pkw_weighted_sums takes for 2^n_vars elements: min(2^n_vars / 2^8, WSUM_MAX_WG), at least 1
unsigned wsum_grid(unsigned n_vars);
// scratch for the partial sums of one pass, in field elements
size_t wsum_partial_fes(unsigned batch, unsigned n_vars);
// enqueue on `stream`: d_out[b * l + i] = sum_x d_weights[i][x] * d_evals[b][x] (Montgomery in, Montgomery out; weights < p).
// d_evals / d_weights: HOST arrays of device pointers.  grid = 0: wsum_grid(n_vars); any other grid gives the same bits.
// tile: 0 = what ships: WSUM_TILE_B x WSUM_TILE_W, and 1 x 4 for batch = 1; 1 = 1 x 4, 2 = 2 x 1 always (the alternatives, to be measured
// against it: tools/whir_pcs_linear_bench.py).  Tile 3 = 2 x 2 always.
int wsum_launch(hipStream_t stream, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* const* d_weights, unsigned l,
                uint64_t* d_partial, uint64_t* d_out, unsigned grid = 0, int tile = 0);
// One pass (L <= WSUM_PASS weights) of the same kernel over the workgroups [first_wg, first_wg + count) of a grid of `grid` alone: what a
// rank of a device set runs (pcs.cpp) and tools/probes measures.  d_partial[(b * L + i) * count + j] = the share of workgroup
// first_wg + j: batch * L * count elements, to be finished with chunk = count next to the other slices' blocks
int wsum_slice_launch(hipStream_t stream, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* const* d_weights, unsigned L,
                      unsigned first_wg, unsigned count, uint64_t* d_partial, unsigned grid = 0, int tile = 0);
// enqueue on `stream`: d_w[x] = (accumulate ? d_w[x] : 0) + sum_i scales[i] * d_weights[i][x] over `len` elements; scales: l HOST
// elements (Montgomery, < p).  Each weight is read once; d_w is read (when accumulating) and written once per COMB_TILE weights.
int combine_launch(hipStream_t stream, uint64_t* d_w, size_t len, const uint64_t* const* d_weights, const uint64_t* scales, unsigned l, int accumulate);

}  // namespace pkw
