// whir_linear.hip -- libprovekit_whir.so's linear-statement kernels (csrc/whir_pcs/linear.hip) where the C ABI does not reach: the
// combination kernel, which only pkw_open_linear uses; the weighted-sums kernel on a grid and with a register tile of the caller's
// choice (the result must not depend on either); and the tile's accumulate / flush / result code run on the HOST, for the CPU suite.
#include <hip/hip_runtime.h>

#include <cstring>

#include "pk_probes.h"
#include "whir_pcs/linear.hpp"
#include "whir_pcs/linear_tile.hpp"

extern "C" {

int pk_probe_whir_combine(pk_ctx* ctx, uint64_t* d_w, size_t len, const uint64_t* const* d_weights, const uint64_t* scales, unsigned l, int accumulate) {
    if (!ctx || !d_w || (l && (!d_weights || !scales))) return PK_ERR_BAD_ARG;
    int rc = pk_ctx_sync(ctx);  // also selects the context's device
    if (!rc) rc = pkw::combine_launch(nullptr, d_w, len, d_weights, scales, l, accumulate);
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = PK_ERR_HIP;
    return rc;
}

int pk_probe_whir_weighted_sums(pk_ctx* ctx, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* const* d_weights, unsigned l,
                                unsigned grid, int tile, uint64_t* out) {
    if (!ctx || !d_evals || !d_weights || !out || batch < 1 || batch > pkw::WSUM_MAX_BATCH || n_vars > 30 || l < 1 || l > 64) return PK_ERR_BAD_ARG;
    const size_t part = pkw::wsum_partial_fes(batch, n_vars), res = (size_t)batch * l;
    void* d = nullptr;
    int rc = pk_malloc(ctx, 32 * (part + res), &d);
    if (rc) return rc;
    uint64_t* d_part = (uint64_t*)d;
    uint64_t* d_res = d_part + 4 * part;
    rc = pk_ctx_sync(ctx);
    if (!rc) rc = pkw::wsum_launch(nullptr, d_evals, batch, n_vars, d_weights, l, d_part, d_res, grid, tile);
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = PK_ERR_HIP;
    if (!rc) rc = pk_memcpy_d2h(ctx, out, d_res, 32 * res);
    pk_free(ctx, d);
    return rc;
}

unsigned pk_probe_whir_wsum_grid(unsigned n_vars) { return pkw::wsum_grid(n_vars); }

int pk_probe_wsum_tile_host(const uint64_t* f, const uint64_t* w, unsigned terms, uint64_t* out) {
    if (!f || !w || !out) return PK_ERR_BAD_ARG;
    constexpr int TB = pkw::WSUM_TILE_B, TW = pkw::WSUM_TILE_W;
    pkw::WsumTile<TB, TW> t;
    pkw::wsum_tile_init(t);
    for (unsigned s = 0; s < terms; s++) {
        pk::fe fv[TB], wv[TW];
        for (int u = 0; u < TB; u++) memcpy(fv[u].v, f + 4 * ((size_t)u * terms + s), 32);
        for (int v = 0; v < TW; v++) memcpy(wv[v].v, w + 4 * ((size_t)v * terms + s), 32);
        pkw::wsum_tile_step(t, fv, wv);
    }
    for (int u = 0; u < TB; u++)
        for (int v = 0; v < TW; v++) {
            const pk::fe r = pkw::wsum_tile_result(t, u, v);
            memcpy(out + 4 * (u * TW + v), r.v, 32);
        }
    return PK_OK;
}

}  // extern "C"
