// grandproduct.hip -- libprovekit_grandproduct.so where its C ABI does not reach.  Its tree and leaf kernels by themselves with the two
// knobs the library's rule would choose itself -- the layers per launch and the grid -- and their device time, so that the tests can
// check that no bit depends on either and tools/grandproduct_bench.py can time S = 1, 2, 3 on the same box, alternating.  And a
// prover's knobs and profile (csrc/grandproduct/prover.hpp): the same two knobs for its proofs, and where its last proof's time went.
#include <hip/hip_runtime.h>

#include "pk_probes.h"
#include "grandproduct/prover.hpp"

namespace {

template <class Launch>
int timed(pk_ctx* ctx, float* ms, Launch launch) {
    int rc = pk_ctx_sync(ctx);  // also selects the context's device
    if (rc) return rc;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return PK_ERR_HIP;
    (void)hipEventRecord(a, nullptr);
    rc = launch();
    (void)hipEventRecord(b, nullptr);
    if (hipStreamSynchronize(nullptr) != hipSuccess) rc = PK_ERR_HIP;
    float t = 0;
    if (!rc && hipEventElapsedTime(&t, a, b) != hipSuccess) rc = PK_ERR_HIP;
    if (ms) *ms = t;
    (void)hipEventDestroy(a), (void)hipEventDestroy(b);
    return rc;
}

}  // namespace

extern "C" {

int pk_probe_grandproduct_tree(pk_ctx* ctx, unsigned n, const uint64_t* d_v, uint64_t* d_tree, unsigned layers, unsigned grid, float* ms) {
    if (!ctx || !d_v || !d_tree) return PK_ERR_BAD_ARG;
    return timed(ctx, ms, [&] { return pkg::tree_launch(nullptr, n, d_v, d_tree, layers, grid); });
}

int pk_probe_grandproduct_leaf_tree(pk_ctx* ctx, unsigned n, unsigned w, const uint64_t* const* d_cols, const uint64_t* gamma, const uint64_t* beta,
                                    uint64_t* d_leaf, uint64_t* d_tree, unsigned layers, unsigned grid, float* ms) {
    if (!ctx || !d_cols || !gamma || !beta || !d_leaf || !d_tree || w < 1 || w > PKG_MAX_COLUMNS) return PK_ERR_BAD_ARG;
    pkg::Leaves lv{};
    lv.w = w;
    for (unsigned j = 0; j < w; j++) lv.col[j] = d_cols[j];
    memcpy(lv.gamma, gamma, 32);
    memcpy(lv.beta, beta, 32);
    return timed(ctx, ms, [&] { return pkg::leaf_tree_launch(nullptr, n, lv, d_leaf, d_tree, layers, grid); });
}

int pk_probe_grandproduct_set_knobs(pkg_prover* p, unsigned layers, unsigned grid) {
    if (!p || layers > pkg::TREE_MAX_LAYERS || grid > PKG_MAX_GRID) return PK_ERR_BAD_ARG;
    p->layers = layers, p->grid = grid;
    return PK_OK;
}

int pk_probe_grandproduct_profile(const pkg_prover* p, double* tree_ms, double* layer_ms28) {
    if (!p || !tree_ms || !layer_ms28) return PK_ERR_BAD_ARG;
    *tree_ms = p->prof.tree_ms;
    for (unsigned d = 0; d < PKG_MAX_VARS; d++) layer_ms28[d] = p->prof.layer_ms[d];
    return PK_OK;
}

pkg_prover* pk_probe_multiset_inner(pkg_multiset_prover* p) { return p ? p->inner : nullptr; }

unsigned pk_probe_grandproduct_default_layers(void) { return pkg::TREE_LAYERS; }

}  // extern "C"
