// kernels.hpp -- the launches of tuple.hip, for prover.cpp.  Everything is enqueued on `stream`; grids are 1 .. PKT_MAX_GRID
// workgroups of 256 per group (the launch's y dimension is the group); no bit of a result depends on the grid.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.hpp"

namespace pkt {

// the columns of up to four groups of rows, as the kernels take them: col[g][j] = group g's column j (device pointers)
struct Columns {
    const uint64_t* col[PKT_MAX_GROUPS][PKT_MAX_WIDTH];
    const uint32_t* idx[PKT_MAX_GROUPS];  // count_launch only: group g's indices into t
};

// d_leaf[g 2^n + x] = alpha - sum_j beta^j col[g][j][x] for g < c, x < 2^n: tuple_leaf_kernel<w>, one launch.  grid_or_0: the
// workgroups per group; 0: LEAF_ITEMS rows per lane.
int leaf_launch(hipStream_t stream, unsigned n, unsigned w, unsigned c, const Columns& cols, const uint64_t alpha[4], const uint64_t beta[4], uint64_t* d_leaf,
                unsigned grid_or_0);

// The multiplicities of the table t (w columns of 2^k) under the c groups of f with their indices: zeroes d_counts (2^k u32) and sets
// *d_bad to all ones, tuple_count_kernel<w, k <= COUNT_LDS_MAX_K> counts the valid rows of every group into d_counts and lowers *d_bad
// to the smallest failing stacked index g 2^n + x, a mont pass writes d_m_out (2^k elements).  grid_or_0: the workgroups per group;
// 0: COUNT_ITEMS rows per lane.
int count_launch(hipStream_t stream, unsigned n, unsigned k, unsigned w, unsigned c, const Columns& f, const uint64_t* const d_t[PKT_MAX_WIDTH],
                 uint32_t* d_counts, unsigned long long* d_bad, uint64_t* d_m_out, unsigned grid_or_0);

}  // namespace pkt
