// kernels.hpp -- the launches of bitwise.hip, for prover.cpp.  Everything is enqueued on `stream`; grids are 1 .. PKB_MAX_GRID workgroups
// of 256 (grid_or_0 = 0: the library's rule); no bit of a result depends on the grid.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.hpp"

namespace pkb {

// what the cell of the first bad entry holds: (x << 2) | case, so that the smallest x wins an atomicMin and its case comes with it.  An
// entry has one case: the first of these that applies.  All ones: no entry failed
enum BadCase : unsigned { BAD_A = 0, BAD_B = 1, BAD_C = 2 };
constexpr unsigned long long NO_BAD = ~0ull;

// what a prover's arena holds that depends on the statement alone: row y = (u << d) | v of the table is (u, v, u op v), y < 2^(2d)
int table_launch(hipStream_t stream, unsigned op, unsigned d, uint64_t* const d_cols[3], unsigned grid_or_0);

// bitwise_decompose_kernel and the Montgomery pass over the counts.  Every entry of d_a and d_b (2^n elements) is checked against
// 2^(L d); c_given: d_c (2^n elements) is read and compared with a op b, else it is written.  A failure lowers *d_bad, set to all ones
// here; the entry is not counted.  The 3 L digit columns go to d_digits[j * L + i] (2^n elements each) and all c groups' bins are
// counted into d_counts (2^(2d) u32, zeroed here), which d_m_out (2^(2d) elements) then holds as elements.  Writes nothing else.
int decompose_launch(hipStream_t stream, unsigned n, unsigned op, unsigned d, unsigned L, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, bool c_given,
                     uint64_t* const* d_digits, uint32_t* d_counts, unsigned long long* d_bad, uint64_t* d_m_out, unsigned grid_or_0);

}  // namespace pkb
