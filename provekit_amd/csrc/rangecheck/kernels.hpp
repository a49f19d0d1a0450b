// kernels.hpp -- the launches of range.hip, for prover.cpp.  Everything is enqueued on `stream`; grids are 1 .. PKR_MAX_GRID workgroups
// of 256 (grid_or_0 = 0: the library's rule); no bit of a result depends on the grid.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.hpp"

namespace pkr {

// what a prover's arena holds that depends on the statement alone: d_out[y] = y for y < 2^k
int index_launch(hipStream_t stream, unsigned k, uint64_t* d_out, unsigned grid_or_0);

// range_decompose_kernel and the Montgomery pass over the counts.  (bits, k) must have a plan.  Every entry of d_f (2^n elements) is
// checked against 2^bits (a failure lowers *d_bad, set to all ones here, to the entry x; the entry is not counted), its L limbs are
// stored to d_limbs[i] (2^n elements each) and all c groups' bins are counted into d_counts (2^k u32, zeroed here), which d_m_out
// (2^k elements) then holds as elements.  Writes nothing else.
int decompose_launch(hipStream_t stream, unsigned n, unsigned bits, unsigned k, const uint64_t* d_f, uint64_t* const d_limbs[PKR_MAX_GROUPS], uint32_t* d_counts,
                     unsigned long long* d_bad, uint64_t* d_m_out, unsigned grid_or_0);

// range_scale_kernel: d_out[x] = 2^shift d_limb[x], 2^n elements, shift < 28
int scale_launch(hipStream_t stream, unsigned n, unsigned shift, const uint64_t* d_limb, uint64_t* d_out, unsigned grid_or_0);

}  // namespace pkr
