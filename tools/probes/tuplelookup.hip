// tuplelookup.hip -- libprovekit_tuplelookup.so where its C ABI does not reach.  Its leaf kernel by itself with the grid the library's
// rule would choose itself, and its device time, so that the tests can check that no bit depends on the grid and
// tools/tuplelookup_bench.py can time it.  And a prover's knob and profile (csrc/tuplelookup/prover.hpp): the grid of both kernels for
// its proofs and multiplicities, and where its last calls' time went.
#include <hip/hip_runtime.h>

#include "pk_probes.h"
#include "tuplelookup/prover.hpp"

extern "C" {

int pk_probe_tuple_leaves(pk_ctx* ctx, unsigned n, unsigned w, unsigned c, const uint64_t* const* d_cols, const uint64_t* alpha, const uint64_t* beta,
                          uint64_t* d_leaf, unsigned grid, float* ms) {
    if (!ctx || !d_cols || !alpha || !beta || !d_leaf || w < 1 || w > PKT_MAX_WIDTH || !pkt::groups_ok(c)) return PK_ERR_BAD_ARG;
    pkt::Columns cols{};
    for (unsigned g = 0; g < c; g++)
        for (unsigned j = 0; j < w; j++) cols.col[g][j] = d_cols[g * w + j];
    int rc = pk_ctx_sync(ctx);  // also selects the context's device
    if (rc) return rc;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return PK_ERR_HIP;
    (void)hipEventRecord(a, nullptr);
    rc = pkt::leaf_launch(nullptr, n, w, c, cols, alpha, beta, d_leaf, grid);
    (void)hipEventRecord(b, nullptr);
    if (hipStreamSynchronize(nullptr) != hipSuccess) rc = PK_ERR_HIP;
    float t = 0;
    if (!rc && hipEventElapsedTime(&t, a, b) != hipSuccess) rc = PK_ERR_HIP;
    if (ms) *ms = t;
    (void)hipEventDestroy(a), (void)hipEventDestroy(b);
    return rc;
}

int pk_probe_tuple_set_grid(pkt_prover* p, unsigned grid) {
    if (!p || grid > PKT_MAX_GRID) return PK_ERR_BAD_ARG;
    p->grid = grid;
    return PK_OK;
}

int pk_probe_tuple_profile(const pkt_prover* p, double* leaf_ms, double* count_ms, double* side_ms2) {
    if (!p || !leaf_ms || !count_ms || !side_ms2) return PK_ERR_BAD_ARG;
    *leaf_ms = p->prof.leaf_ms, *count_ms = p->prof.count_ms;
    side_ms2[0] = p->prof.side_ms[0], side_ms2[1] = p->prof.side_ms[1];
    return PK_OK;
}

unsigned pk_probe_tuple_leaf_items(void) { return pkt::LEAF_ITEMS; }

}  // extern "C"
