// lookup.hip -- libprovekit_lookup.so where its C ABI does not reach.  Either of its two gather kernels by itself, whatever the
// library's rule would pick, so that tools/lookup_bench.py can time the LDS-staged kernel against the one that reads through L2 on the
// same box, alternating.  And a prover's two test and benchmark knobs (csrc/lookup/prover.hpp): the grid of its kernels, for the tests
// that no bit depends on it, and where its last proof's time went.
#include <hip/hip_runtime.h>

#include "pk_probes.h"
#include "lookup/prover.hpp"

extern "C" {

int pk_probe_lookup_gather(pk_ctx* ctx, const uint32_t* d_idx, const uint64_t* d_g, const uint64_t* d_dt, unsigned n, unsigned k, uint64_t* d_hf,
                           uint64_t* d_df, int staged, unsigned grid, float* ms) {
    if (!ctx || !d_idx || !d_g || !d_dt || !d_hf || !d_df) return PK_ERR_BAD_ARG;
    int rc = pk_ctx_sync(ctx);  // also selects the context's device
    if (rc) return rc;
    pkl::GatherPlan plan;  // outside the timed pair, as a prover's is
    if ((rc = pkl::gather_prepare(plan))) return rc;
    hipEvent_t a, b;
    uint32_t* d_flags = nullptr;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess || hipMalloc((void**)&d_flags, 8) != hipSuccess) return PK_ERR_HIP;
    (void)hipEventRecord(a, nullptr);
    rc = pkl::gather_launch(nullptr, plan, n, k, d_idx, d_g, d_dt, d_hf, d_df, d_flags, grid, staged ? 1 : 0);
    (void)hipEventRecord(b, nullptr);
    if (hipStreamSynchronize(nullptr) != hipSuccess) rc = PK_ERR_HIP;
    float t = 0;
    if (!rc && hipEventElapsedTime(&t, a, b) != hipSuccess) rc = PK_ERR_HIP;
    if (ms) *ms = t;
    (void)hipEventDestroy(a), (void)hipEventDestroy(b), (void)hipFree(d_flags);
    return rc;
}

int pk_probe_lookup_set_grid(pkl_prover* p, unsigned grid) {
    if (!p || grid > PKL_MAX_GRID) return PK_ERR_BAD_ARG;
    p->grid = grid;
    return PK_OK;
}

int pk_probe_lookup_profile(const pkl_prover* p, double* ms5) {
    if (!p || !ms5) return PK_ERR_BAD_ARG;
    const pkl::Profile& f = p->prof;
    ms5[0] = f.count_ms, ms5[1] = f.table_ms, ms5[2] = f.gather_ms, ms5[3] = f.sumcheck_f_ms, ms5[4] = f.sumcheck_t_ms;
    return PK_OK;
}

}  // extern "C"
