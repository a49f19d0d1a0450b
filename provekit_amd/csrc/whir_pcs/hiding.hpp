// hiding.hpp -- the launch of hiding.hip: the masks and g of a hiding commitment drawn in one launch, for pcs.cpp (pkw_commit_hiding
// runs it on the scheme's stream) and for tools/probes.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/provekit_whir.h"

namespace pkw {

constexpr unsigned HIDING_MAX_POLYS = 3;       // B: the caller's polynomials; g makes the batch B + 1 <= 4
constexpr unsigned HIDING_THREADS = 256;
constexpr unsigned HIDING_PAIRS_PER_LANE = 8;  // what the default grid gives a lane, so that the retries of its pairs average out

// the pairs of the index space [mask_0 | .. | mask_{B-1} | g] for polynomials of n >= 1 variables: (B + 2) * 2^(n-1)
size_t hiding_pairs(unsigned polys, unsigned n);
// the grid the library takes: one workgroup per HIDING_THREADS * HIDING_PAIRS_PER_LANE pairs, rounded up, at least one
unsigned hiding_grid(unsigned polys, unsigned n);
// enqueue on `stream`: d_tables[b][2^n + i] = element i of stream PKW_RNG_MASK0 + b, i < 2^n, for b < polys, and
// d_tables[polys][i] = element i of stream PKW_RNG_G, i < 2^(n+1).  d_tables: HOST array of polys + 1 device tables of 2^(n+1)
// elements; the lower halves of the first `polys` are not touched.  polys 1..HIDING_MAX_POLYS, n 1..29.  grid = 0: hiding_grid;
// any other grid gives the same bits.  PK_ERR_HIP: the launch failed, and *launch_error (if given) says how.
int hiding_fill_launch(hipStream_t stream, uint64_t* const* d_tables, unsigned polys, unsigned n, const uint8_t key32[32], unsigned grid = 0,
                       hipError_t* launch_error = nullptr);

}  // namespace pkw
