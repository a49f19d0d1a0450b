// fracsum.hip -- libprovekit_fracsum.so where its C ABI does not reach.  Its tree, lookup-leaf and combine kernels by themselves with the
// two knobs the library's rule would choose itself -- the layers per launch and the grid -- and their device time, so that the tests can
// check that no bit depends on either and tools/fracsum_bench.py can time S = 1, 2, 3 on the same box, alternating.  And a prover's
// knobs and profile (csrc/fracsum/prover.hpp): the same two knobs for its proofs, and where its last proof's time went.
#include <hip/hip_runtime.h>

#include "pk_probes.h"
#include "fracsum/prover.hpp"

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

int pk_probe_fracsum_tree(pk_ctx* ctx, unsigned n, const uint64_t* d_p_or_null, const uint64_t* d_q, uint64_t* d_ptree, uint64_t* d_qtree, unsigned layers,
                          unsigned grid, float* ms) {
    if (!ctx || !d_q || !d_ptree || !d_qtree) return PK_ERR_BAD_ARG;
    return timed(ctx, ms, [&] { return pkf::tree_launch(nullptr, n, d_p_or_null, d_q, d_ptree, d_qtree, layers, grid); });
}

int pk_probe_fracsum_lookup_leaf(pk_ctx* ctx, unsigned n, const uint64_t* d_table, const uint64_t* d_m_or_null, const uint64_t* alpha, uint64_t* d_leaf,
                                 uint64_t* d_ptree, uint64_t* d_qtree, unsigned layers, unsigned grid, float* ms) {
    if (!ctx || !d_table || !alpha || !d_leaf || !d_ptree || !d_qtree) return PK_ERR_BAD_ARG;
    return timed(ctx, ms, [&] { return pkf::lookup_leaf_launch(nullptr, n, d_table, d_m_or_null, alpha, d_leaf, d_ptree, d_qtree, layers, grid); });
}

int pk_probe_fracsum_combine(pk_ctx* ctx, size_t count, const uint64_t* d_pR_or_null, const uint64_t* d_qR, const uint64_t* lambda, uint64_t* d_u, unsigned grid,
                             float* ms) {
    if (!ctx || !d_qR || !lambda || !d_u) return PK_ERR_BAD_ARG;
    return timed(ctx, ms, [&] { return pkf::combine_launch(nullptr, count, d_pR_or_null, d_qR, lambda, d_u, grid); });
}

int pk_probe_fracsum_set_knobs(pkf_prover* p, unsigned layers, unsigned grid) {
    if (!p || layers > pkf::TREE_MAX_LAYERS || grid > PKF_MAX_GRID) return PK_ERR_BAD_ARG;
    p->layers = layers, p->grid = grid;
    return PK_OK;
}

int pk_probe_fracsum_profile(const pkf_prover* p, double* tree_ms, double* combine_ms28, double* layer_ms28) {
    if (!p || !tree_ms || !combine_ms28 || !layer_ms28) return PK_ERR_BAD_ARG;
    *tree_ms = p->prof.tree_ms;
    for (unsigned d = 0; d < PKF_MAX_VARS; d++) combine_ms28[d] = p->prof.combine_ms[d], layer_ms28[d] = p->prof.layer_ms[d];
    return PK_OK;
}

pkf_prover* pk_probe_fracsum_lookup_side(pkf_lookup_prover* p, int side) { return p && (side == PKF_SIDE_F || side == PKF_SIDE_T) ? p->side[side] : nullptr; }

unsigned pk_probe_fracsum_default_layers(void) { return pkf::TREE_LAYERS; }

}  // extern "C"
