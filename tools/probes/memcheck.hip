// memcheck.hip -- libprovekit_memcheck.so where its C ABI does not reach.  Its two leaf kernels by themselves with the grid the library's
// rule would choose itself, and their device time, so that the tests can check that no bit depends on the grid and
// tools/memcheck_bench.py can time them.  And a prover's knob and profile (csrc/memcheck/prover.hpp): the grid of every kernel of its
// traces and proofs, and where its last calls' time went.
#include <hip/hip_runtime.h>

#include "pk_probes.h"
#include "memcheck/prover.hpp"

extern "C" {

int pk_probe_mem_leaves(pk_ctx* ctx, unsigned n, unsigned k, const pkm_columns* cols, const uint64_t* gamma, const uint64_t* beta, uint64_t* d_ops, uint64_t* d_mem,
                        uint64_t* d_f_or_null, unsigned grid, float* ms2) {
    if (!ctx || !cols || !gamma || !beta || !d_ops || !d_mem) return PK_ERR_BAD_ARG;
    const pkm::LeafColumns c{cols->a, cols->wv, cols->rv, cols->rt, cols->init, cols->fin, cols->ft};
    int rc = pk_ctx_sync(ctx);  // also selects the context's device
    if (rc) return rc;
    hipEvent_t ev[3];
    for (hipEvent_t& e : ev)
        if (hipEventCreate(&e) != hipSuccess) return PK_ERR_HIP;
    (void)hipEventRecord(ev[0], nullptr);
    rc = pkm::ops_leaf_launch(nullptr, n, c, gamma, beta, d_ops, d_f_or_null, grid);
    (void)hipEventRecord(ev[1], nullptr);
    if (!rc) rc = pkm::cells_leaf_launch(nullptr, k, c, gamma, beta, d_mem, grid);
    (void)hipEventRecord(ev[2], nullptr);
    if (hipStreamSynchronize(nullptr) != hipSuccess) rc = PK_ERR_HIP;
    float t[2] = {0, 0};
    if (!rc && (hipEventElapsedTime(&t[0], ev[0], ev[1]) != hipSuccess || hipEventElapsedTime(&t[1], ev[1], ev[2]) != hipSuccess)) rc = PK_ERR_HIP;
    if (ms2) ms2[0] = t[0], ms2[1] = t[1];
    for (hipEvent_t& e : ev) (void)hipEventDestroy(e);
    return rc;
}

int pk_probe_mem_set_grid(pkm_prover* p, unsigned grid) {
    if (!p || grid > PKM_MAX_GRID) return PK_ERR_BAD_ARG;
    p->grid = grid;
    return PK_OK;
}

int pk_probe_mem_profile(const pkm_prover* p, double* trace_ms4, double* leaf_ms, double* side_ms3) {
    if (!p || !trace_ms4 || !leaf_ms || !side_ms3) return PK_ERR_BAD_ARG;
    trace_ms4[0] = p->prof.key_ms, trace_ms4[1] = p->prof.sort_ms, trace_ms4[2] = p->prof.resolve_ms, trace_ms4[3] = p->prof.count_ms;
    *leaf_ms = p->prof.leaf_ms;
    for (int side = 0; side < 3; side++) side_ms3[side] = p->prof.side_ms[side];
    return PK_OK;
}

unsigned pk_probe_mem_leaf_items(void) { return pkm::LEAF_ITEMS; }
unsigned pk_probe_mem_trace_items(void) { return pkm::TRACE_ITEMS; }
unsigned pk_probe_mem_count_lds_max_n(void) { return pkm::COUNT_LDS_MAX_N; }

}  // extern "C"
