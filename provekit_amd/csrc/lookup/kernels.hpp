// kernels.hpp -- the launches of lookup.hip, for prover.cpp.  Everything is enqueued on `stream`; grids are 1 .. PKL_MAX_GRID
// workgroups of 256 and no bit of any result depends on them.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.hpp"

namespace pkl {

// Step 1: validate every x < 2^n (idx[x] < 2^k and f[x] == t[idx[x]] on the stored words) and count.  d_counts (2^k u32) and d_bad
// (one u64) are reset here; d_bad ends as the smallest failing x or UINT64_MAX.  Then m_out[y] = counts[y] as a Montgomery element.
// Tables of k <= COUNT_LDS_MAX_K count in LDS, larger ones in device memory.
int count_launch(hipStream_t stream, unsigned n, unsigned k, const uint64_t* d_f, const uint64_t* d_t, const uint32_t* d_idx, uint32_t* d_counts,
                 unsigned long long* d_bad, uint64_t* d_m_out, unsigned grid_or_0);

// Step 3, the table side: d_t_out = alpha - t, g = 1 / d_t_out, h_t = counts * g, and *d_sum = sum_y h_t[y] through d_partials
// (grid elements) and a finish kernel.  d_flags[0] is reset here and raised when a denominator is zero.
int table_launch(hipStream_t stream, unsigned k, const uint64_t* d_t, const uint32_t* d_counts, const uint64_t* alpha, uint64_t* d_dt, uint64_t* d_g,
                 uint64_t* d_ht, uint64_t* d_partials, uint64_t* d_sum, uint32_t* d_flags, unsigned grid_or_0);

// What the staged gather's launch needs of the device: asked once, by gather_prepare on the current device (a prover does it at its
// creation), not per launch.
struct GatherPlan {
    int cus = 0;  // compute units; 0: not prepared
};
// Fills the plan and lets the staged kernel ask for its LDS (more than a kernel gets without asking).  No launch.
int gather_prepare(GatherPlan& plan);

// Step 3, the column side: h_f[x] = g[idx[x]], d_f[x] = d_t[idx[x]].  d_flags[1] is reset here and raised by an index >= 2^k, which
// is not followed.  staging: < 0 the library's rule (the LDS-staged kernel for k <= GATHER_LDS_MAX_K), 0 the kernel that reads through
// L2 whatever k is, > 0 the staged kernel (k <= GATHER_LDS_MAX_K): the last two are the benchmark's yardstick (tools/probes/lookup.hip).
// The staged kernel needs a prepared plan (PK_ERR_BAD_ARG otherwise).
int gather_launch(hipStream_t stream, const GatherPlan& plan, unsigned n, unsigned k, const uint32_t* d_idx, const uint64_t* d_g, const uint64_t* d_dt,
                  uint64_t* d_hf, uint64_t* d_df, uint32_t* d_flags, unsigned grid_or_0, int staging = -1);

}  // namespace pkl
