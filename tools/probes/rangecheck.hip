// rangecheck.hip -- libprovekit_rangecheck.so where its C ABI does not reach.  Its decomposition pass by itself over tables the caller
// holds, with the grid the library's rule would choose itself, and its device time, so that tools/rangecheck_bench.py can time the hot
// pass alone.  And a prover's knob and profile (csrc/rangecheck/prover.hpp): the grid of every kernel of its calls, and where its last
// calls' time went.
#include <hip/hip_runtime.h>

#include "pk_probes.h"
#include "rangecheck/prover.hpp"

extern "C" {

int pk_probe_range_decompose(pk_ctx* ctx, unsigned n, unsigned bits, unsigned k, const uint64_t* d_f, uint64_t* const* d_limbs, uint32_t* d_counts,
                             unsigned long long* d_bad, uint64_t* d_m, unsigned grid, float* ms) {
    if (!ctx || !d_limbs) return PK_ERR_BAD_ARG;
    const pkr_statement st{n, bits, k, 0};
    std::string why;
    if (!pkr::statement_ok(&st, why)) return PK_ERR_BAD_ARG;
    uint64_t* limbs[PKR_MAX_GROUPS] = {};
    for (unsigned i = 0; i < pkr::plan_of(bits, k).L; i++) limbs[i] = d_limbs[i];
    int rc = pk_ctx_sync(ctx);  // also selects the context's device
    if (rc) return rc;
    hipEvent_t ev[2];
    for (hipEvent_t& e : ev)
        if (hipEventCreate(&e) != hipSuccess) return PK_ERR_HIP;
    (void)hipEventRecord(ev[0], nullptr);
    rc = pkr::decompose_launch(nullptr, n, bits, k, d_f, limbs, d_counts, d_bad, d_m, grid);
    (void)hipEventRecord(ev[1], nullptr);
    if (hipStreamSynchronize(nullptr) != hipSuccess) rc = PK_ERR_HIP;
    float t_ms = 0;
    if (!rc && hipEventElapsedTime(&t_ms, ev[0], ev[1]) != hipSuccess) rc = PK_ERR_HIP;
    if (ms) *ms = t_ms;
    for (hipEvent_t& e : ev) (void)hipEventDestroy(e);
    return rc;
}

int pk_probe_range_set_grid(pkr_prover* p, unsigned grid) {
    if (!p || grid > PKR_MAX_GRID) return PK_ERR_BAD_ARG;
    p->grid = grid;
    return PK_OK;
}

int pk_probe_range_profile(const pkr_prover* p, double* decompose_ms, double* scale_ms, double* lookup_ms) {
    if (!p || !decompose_ms || !scale_ms || !lookup_ms) return PK_ERR_BAD_ARG;
    *decompose_ms = p->prof.decompose_ms, *scale_ms = p->prof.scale_ms, *lookup_ms = p->prof.lookup_ms;
    return PK_OK;
}

// the workgroups the library's rule gives each kernel at a statement: decompose, scale (0: none, r = k), index, m
int pk_probe_range_grids(unsigned n, unsigned bits, unsigned k, unsigned* grids4) {
    const pkr_statement st{n, bits, k, 0};
    std::string why;
    if (!grids4 || !pkr::statement_ok(&st, why)) return PK_ERR_BAD_ARG;
    grids4[0] = pkr::rows_grid((size_t)1 << n, pkr::DECOMPOSE_ITEMS);
    grids4[1] = pkr::plan_of(bits, k).r < k ? pkr::rows_grid((size_t)1 << n, pkr::PLAIN_ITEMS) : 0;
    grids4[2] = grids4[3] = pkr::rows_grid((size_t)1 << k, pkr::PLAIN_ITEMS);
    return PK_OK;
}

unsigned pk_probe_range_decompose_items(void) { return pkr::DECOMPOSE_ITEMS; }

}  // extern "C"
