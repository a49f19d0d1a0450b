// kernels.hpp -- the launches of mem.hip, for prover.cpp.  Everything is enqueued on `stream`; grids are 1 .. PKM_MAX_GRID workgroups
// of 256 (grid_or_0 = 0: the library's rule); no bit of a result depends on the grid.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.hpp"

namespace pkm {

// the bytes of temporary storage one radix sort of 2^n keys over n + k bits asks for (host only, no launch); 0: the query failed
size_t sort_tmp_bytes(unsigned n, unsigned k);

// what a prover's arena holds that depends on the statement alone: sign[x] = +1 for x < 2^v, -1 for 2^v <= x < 2^(v+1)
int sign_launch(hipStream_t stream, unsigned v, uint64_t* d_sign, unsigned grid_or_0);
// ... and t[x] = x for x < 2^n
int iota_launch(hipStream_t stream, unsigned n, uint64_t* d_t, unsigned grid_or_0);

// The arena's parts the trace builder works in (layout.hpp)
struct TraceScratch {
    unsigned long long *keys, *sorted;  // 2^n each; after the sort `keys` holds the 2^n u32 values of f
    uint32_t* counts;                   // 2^n
    void* sort_tmp;
    size_t sort_tmp_bytes;
    unsigned long long* bad;  // the smallest operation index whose address is >= 2^k; all ones: none
};
struct TraceTables {
    const uint32_t* addr;       // 2^n
    const uint64_t *wv, *init;  // 2^n, 2^k
    uint64_t *a, *rv, *rt, *m;  // 2^n each
    uint64_t *fin, *ft;         // 2^k each
};
// The trace builder's four phases; ev[0 .. 4] (NULL: no events) are recorded around them: key (validate every address, a[i], the
// keys (addr << n | i), fin = init and ft = 0), sort (one radix sort over bits 0 .. n + k), resolve (rv, rt, the runs' ends into
// fin and ft, f's integer values), count (f's histogram, m).  An address >= 2^k lowers *bad and is followed as address 0.
int trace_launch(hipStream_t stream, unsigned n, unsigned k, const TraceTables& t, const TraceScratch& s, unsigned grid_or_0, hipEvent_t* ev);

// the columns the leaf kernels read
struct LeafColumns {
    const uint64_t *a, *wv, *rv, *rt, *init, *fin, *ft;
};
// mem_ops_leaf_kernel: d_q[i] = gamma - (a_i + beta wv_i + beta^2 (i + 1)), d_q[2^n + i] = gamma - (a_i + beta rv_i + beta^2 rt_i)
// and, where d_f_or_null is given, d_f[i] = i - rt_i, in one pass over a, wv, rv, rt
int ops_leaf_launch(hipStream_t stream, unsigned n, const LeafColumns& c, const uint64_t gamma[4], const uint64_t beta[4], uint64_t* d_q, uint64_t* d_f_or_null,
                    unsigned grid_or_0);
// mem_cells_leaf_kernel: d_q[j] = gamma - (j + beta init_j), d_q[2^k + j] = gamma - (j + beta fin_j + beta^2 ft_j)
int cells_leaf_launch(hipStream_t stream, unsigned k, const LeafColumns& c, const uint64_t gamma[4], const uint64_t beta[4], uint64_t* d_q, unsigned grid_or_0);

}  // namespace pkm
