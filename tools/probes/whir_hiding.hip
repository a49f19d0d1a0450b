// whir_hiding.hip -- libprovekit_whir.so's hiding stage (csrc/whir_pcs/hiding.hip) where the C ABI does not reach: the one launch that
// draws the masks and g, on a grid of the caller's choice (the bits must not depend on it), and the grid rule itself.
#include <hip/hip_runtime.h>

#include "pk_probes.h"
#include "whir_pcs/hiding.hpp"

extern "C" {

int pk_probe_whir_hiding_fill(pk_ctx* ctx, uint64_t* const* d_tables, unsigned polys, unsigned n, const uint8_t key32[32], unsigned grid) {
    if (!ctx || !d_tables || !key32) return PK_ERR_BAD_ARG;
    int rc = pk_ctx_sync(ctx);  // also selects the context's device
    if (!rc) rc = pkw::hiding_fill_launch(nullptr, d_tables, polys, n, key32, grid);
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = PK_ERR_HIP;
    return rc;
}

unsigned pk_probe_whir_hiding_grid(unsigned polys, unsigned n) { return polys >= 1 && n >= 1 && n <= 29 ? pkw::hiding_grid(polys, n) : 0; }
unsigned pk_probe_whir_hiding_threads(void) { return pkw::HIDING_THREADS; }
unsigned pk_probe_whir_hiding_pairs_per_lane(void) { return pkw::HIDING_PAIRS_PER_LANE; }

}  // extern "C"
