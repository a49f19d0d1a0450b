// evaluate.hpp -- the launches of evaluate.hip: the evaluation kernel, for pcs.cpp (pkw_open runs it on the scheme's stream with arena
// scratch), and the finish kernel and grid cap that linear.hip and sparse.hip share with it
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/provekit_whir.h"

namespace pkw {

constexpr unsigned EVAL_LOW_VARS = 8;  // a tile = 2^8 contiguous evaluations, one per lane of a workgroup
constexpr unsigned EVAL_MAX_MID = 6;   // a workgroup streams at most 2^6 tiles
constexpr unsigned EVAL_PASS = 8;      // points per pass over a polynomial
constexpr unsigned EVAL_MAX_BATCH = 4;

// the evaluation kernel's grid for 2^n_vars evaluations: its workgroups, a power of two
unsigned eval_grid(unsigned n_vars);
// scratch for the partial sums, in field elements
size_t eval_partial_fes(unsigned batch, unsigned n_vars);
// enqueue on `stream`: d_out[b * q + i] = MLE(d_evals[b])(d_points[i]); d_points = q * n_vars elements on the device
int eval_launch(hipStream_t stream, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* d_points, unsigned q,
                uint64_t* d_partial, uint64_t* d_out);
// One pass (Q <= EVAL_PASS points) of the same kernel over the workgroups [first_wg, first_wg + count) of eval_grid(n_vars) alone: what a
// rank of a device set runs (pcs.cpp) and tools/probes measures.  d_partial[(b * EVAL_PASS + i) * count + j] = the share of workgroup
// first_wg + j: batch * EVAL_PASS * count elements, to be finished with chunk = count next to the other slices' blocks
int eval_slice_launch(hipStream_t stream, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* d_points, unsigned Q,
                      unsigned first_wg, unsigned count, uint64_t* d_partial);
// The library's one finish kernel, for every kernel that leaves one partial per (output, workgroup).  Enqueue on `stream`:
// d_out[y * out_stride + i] = the sum of the n_wg partials d_partial[(y * row_stride + i) * n_wg ..] for y < rows, i < count <= row_stride.
// row_stride is the pass width of the partial layout: EVAL_PASS here, SPARSE_PASS in sparse.hip, the pass's own count in linear.hip.
// chunk != 0: the partials are the gathered blocks of n_wg / chunk slices of `chunk` workgroups each, block_stride elements apart, each
// laid out as above with chunk in the place of n_wg (a device set's exchange, pcs.cpp)
void finish_launch(hipStream_t stream, const uint64_t* d_partial, unsigned n_wg, unsigned rows, unsigned count, unsigned row_stride, uint64_t* d_out,
                   unsigned out_stride, unsigned chunk = 0, size_t block_stride = 0);
// a grid over n items, one per lane of 256-lane workgroups, at most 2048 workgroups (the kernels that take it stride by the grid)
inline unsigned capped_grid(size_t n) {
    const size_t blocks = (n + 255) / 256;
    return (unsigned)(blocks < 2048 ? blocks : 2048);
}

}  // namespace pkw
