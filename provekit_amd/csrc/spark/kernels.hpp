// kernels.hpp -- the launches of spark.hip, for prover.cpp.  Everything is enqueued on `stream`; grids are 1 .. PKX_MAX_GRID workgroups
// of 256 (grid_or_0 = 0: the library's rule); no bit of a result depends on the grid.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.hpp"

namespace pkx {

// what a prover's arena holds that depends on the statement alone: d_out[x] = x for x < 2^v
int iota_launch(hipStream_t stream, unsigned v, uint64_t* d_out, unsigned grid_or_0);

// spark_count_kernel, once per index array: validates every entry (row_idx[k] < 2^s, col_idx[k] < 2^t; a failure lowers *d_bad to the
// entry k and the entry is not counted) and counts the valid ones into d_counts_row (2^s u32) and d_counts_col (2^t u32), both zeroed
// here, as is *d_bad (all ones: none).  Writes nothing else.
int count_launch(hipStream_t stream, unsigned n, unsigned s, unsigned t, const uint32_t* d_row_idx, const uint32_t* d_col_idx, uint32_t* d_counts_row,
                 uint32_t* d_counts_col, unsigned long long* d_bad, unsigned grid_or_0);
// spark_columns_kernel and the Montgomery pass over the counts: d_row_out[k] = row_idx[k], d_col_out[k] = col_idx[k] as elements, and
// the two multiplicity tables.  Follows count_launch when it found every entry valid; follows no index itself
int columns_launch(hipStream_t stream, unsigned n, unsigned s, unsigned t, const uint32_t* d_row_idx, const uint32_t* d_col_idx, const uint32_t* d_counts_row,
                   const uint32_t* d_counts_col, uint64_t* d_row_out, uint64_t* d_col_out, uint64_t* d_m_row_out, uint64_t* d_m_col_out, unsigned grid_or_0);
// spark_gather_kernel: d_e_row_out[k] = d_eq_row[row_idx[k]], d_e_col_out[k] = d_eq_col[col_idx[k]], every index validated before it is
// followed; a failure lowers *d_bad (set to all ones here) to the entry and is read as index 0
int gather_launch(hipStream_t stream, unsigned n, unsigned s, unsigned t, const uint32_t* d_row_idx, const uint32_t* d_col_idx, const uint64_t* d_eq_row,
                  const uint64_t* d_eq_col, uint64_t* d_e_row_out, uint64_t* d_e_col_out, unsigned long long* d_bad, unsigned grid_or_0);

}  // namespace pkx
