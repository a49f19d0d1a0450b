// spark.hip -- libprovekit_spark.so where its C ABI does not reach.  Its gather kernel by itself over tables the caller holds, with the
// grid the library's rule would choose itself, and its device time, so that tools/spark_bench.py can time the per-query hot pass alone.
// And a prover's knob and profile (csrc/spark/prover.hpp): the grid of every kernel of its calls, and where its last calls' time went.
#include <hip/hip_runtime.h>

#include "pk_probes.h"
#include "spark/prover.hpp"

extern "C" {

int pk_probe_spark_gather(pk_ctx* ctx, unsigned n, unsigned s, unsigned t, const uint32_t* d_row_idx, const uint32_t* d_col_idx, const uint64_t* d_eq_row,
                          const uint64_t* d_eq_col, uint64_t* d_e_row, uint64_t* d_e_col, unsigned long long* d_bad, unsigned grid, float* ms) {
    if (!ctx) return PK_ERR_BAD_ARG;
    int rc = pk_ctx_sync(ctx);  // also selects the context's device
    if (rc) return rc;
    hipEvent_t ev[2];
    for (hipEvent_t& e : ev)
        if (hipEventCreate(&e) != hipSuccess) return PK_ERR_HIP;
    (void)hipEventRecord(ev[0], nullptr);
    rc = pkx::gather_launch(nullptr, n, s, t, d_row_idx, d_col_idx, d_eq_row, d_eq_col, d_e_row, d_e_col, d_bad, grid);
    (void)hipEventRecord(ev[1], nullptr);
    if (hipStreamSynchronize(nullptr) != hipSuccess) rc = PK_ERR_HIP;
    float t_ms = 0;
    if (!rc && hipEventElapsedTime(&t_ms, ev[0], ev[1]) != hipSuccess) rc = PK_ERR_HIP;
    if (ms) *ms = t_ms;
    for (hipEvent_t& e : ev) (void)hipEventDestroy(e);
    return rc;
}

int pk_probe_spark_set_grid(pkx_prover* p, unsigned grid) {
    if (!p || grid > PKX_MAX_GRID) return PK_ERR_BAD_ARG;
    p->grid = grid;
    return PK_OK;
}

int pk_probe_spark_profile(const pkx_prover* p, double* matrix_ms2, double* gather_ms, double* eq_ms, double* side_ms3) {
    if (!p || !matrix_ms2 || !gather_ms || !eq_ms || !side_ms3) return PK_ERR_BAD_ARG;
    matrix_ms2[0] = p->prof.count_ms, matrix_ms2[1] = p->prof.columns_ms;
    *gather_ms = p->prof.gather_ms, *eq_ms = p->prof.eq_ms;
    for (int side = 0; side < 3; side++) side_ms3[side] = p->prof.side_ms[side];
    return PK_OK;
}

unsigned pk_probe_spark_gather_items(void) { return pkx::GATHER_ITEMS; }
unsigned pk_probe_spark_matrix_items(void) { return pkx::MATRIX_ITEMS; }

}  // extern "C"
