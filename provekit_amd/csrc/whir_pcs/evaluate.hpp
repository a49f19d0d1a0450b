// evaluate.hpp -- the evaluation kernel's launch, for pcs.hip (pkw_open runs it on the scheme's stream with arena scratch)
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/provekit_whir.h"

namespace pkw {

constexpr unsigned EVAL_LOW_VARS = 8;  // a tile = 2^8 contiguous evaluations, one per lane of a workgroup
constexpr unsigned EVAL_MAX_MID = 6;   // a workgroup streams at most 2^6 tiles
constexpr unsigned EVAL_PASS = 8;      // points per pass over a polynomial
constexpr unsigned EVAL_MAX_BATCH = 4;

// scratch for the partial sums, in field elements
size_t eval_partial_fes(unsigned batch, unsigned n_vars);
// enqueue on `stream`: d_out[b * q + i] = MLE(d_evals[b])(d_points[i]); d_points = q * n_vars elements on the device
int eval_launch(hipStream_t stream, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* d_points, unsigned q,
                uint64_t* d_partial, uint64_t* d_out);
// enqueue on `stream`: d_out[y * out_stride + i] = the sum of the n_wg partials d_partial[(y * EVAL_PASS + i) * n_wg ..] for y < rows,
// i < count <= EVAL_PASS: the second half of eval_launch, for kernels that leave their partials in the same layout (sparse.hip)
int eval_finish_launch(hipStream_t stream, const uint64_t* d_partial, unsigned n_wg, unsigned rows, unsigned count, uint64_t* d_out, unsigned out_stride);

}  // namespace pkw
