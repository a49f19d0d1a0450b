// whir_linear.hip -- libprovekit_whir.so's linear-statement kernels (csrc/whir_pcs/linear.hip) where the C ABI does not reach: the
// combination kernel, which only pkw_open_linear uses; the weighted-sums kernel on a grid and with a register tile of the caller's
// choice (the result must not depend on either); the tile's accumulate / flush / result code run on the HOST, for the CPU suite; and
// the two reductions on a slice of their workgroups with the finish kernel over gathered blocks, as a rank of a device set runs them.
#include <hip/hip_runtime.h>

#include <cstring>

#include "pk_probes.h"
#include "whir_pcs/evaluate.hpp"
#include "whir_pcs/linear.hpp"
#include "whir_pcs/linear_tile.hpp"

// `fes` elements of device scratch at d; prepare(d) readies it; launch(d) enqueues on the null stream, timed by two events into *ms when
// ms is not null; then `n_out` elements from d + out_at to out
template <class Prepare, class Launch>
static int slice_probe(pk_ctx* ctx, size_t fes, size_t out_at, size_t n_out, uint64_t* out, float* ms, Prepare prepare, Launch launch) {
    void* d = nullptr;
    int rc = pk_malloc(ctx, 32 * (fes ? fes : 1), &d);
    if (rc) return rc;
    hipEvent_t ev[2] = {};
    if (ms && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)) rc = PK_ERR_HIP;
    if (!rc) rc = prepare((uint64_t*)d);
    if (!rc) rc = pk_ctx_sync(ctx);  // the operands are the context's work: finished before the launch
    if (!rc && ms && hipEventRecord(ev[0], nullptr) != hipSuccess) rc = PK_ERR_HIP;
    if (!rc) rc = launch((uint64_t*)d);
    if (!rc && ms && hipEventRecord(ev[1], nullptr) != hipSuccess) rc = PK_ERR_HIP;
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = PK_ERR_HIP;
    if (!rc && ms && hipEventElapsedTime(ms, ev[0], ev[1]) != hipSuccess) rc = PK_ERR_HIP;
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    if (!rc) rc = pk_memcpy_d2h(ctx, out, (uint64_t*)d + 4 * out_at, 32 * n_out);
    pk_free(ctx, d);
    return rc;
}

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

unsigned pk_probe_whir_eval_grid(unsigned n_vars) { return pkw::eval_grid(n_vars); }

int pk_probe_whir_eval_slice(pk_ctx* ctx, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* points, unsigned Q,
                             unsigned first_wg, unsigned count, uint64_t* partial_out, float* ms) {
    if (!ctx || !d_evals || !points || !partial_out || batch < 1 || batch > pkw::EVAL_MAX_BATCH || n_vars < 1 || n_vars > 30 || Q < 1 ||
        Q > pkw::EVAL_PASS || !count || count > pkw::eval_grid(n_vars) || first_wg > pkw::eval_grid(n_vars) - count)
        return PK_ERR_BAD_ARG;
    const size_t pts = (size_t)Q * n_vars, part = (size_t)batch * pkw::EVAL_PASS * count;
    return slice_probe(
        ctx, pts + part, pts, part, partial_out, ms,
        [&](uint64_t* d) {
            const int rc = pk_memcpy_h2d(ctx, d, points, 32 * pts);
            return rc ? rc : pk_memset_zero(ctx, d + 4 * pts, 32 * part);  // the slots of the points beyond Q are never written
        },
        [&](uint64_t* d) { return pkw::eval_slice_launch(nullptr, d_evals, batch, n_vars, d, Q, first_wg, count, d + 4 * pts); });
}

int pk_probe_whir_wsum_slice(pk_ctx* ctx, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* const* d_weights, unsigned L,
                             unsigned grid, unsigned first_wg, unsigned count, int tile, uint64_t* partial_out, float* ms) {
    if (!ctx || !d_evals || !d_weights || !partial_out || n_vars > 30) return PK_ERR_BAD_ARG;  // the launch refuses the rest
    const size_t part = (size_t)batch * L * count;
    return slice_probe(
        ctx, part, 0, part, partial_out, ms, [&](uint64_t*) { return (int)PK_OK; },
        [&](uint64_t* d) { return pkw::wsum_slice_launch(nullptr, d_evals, batch, n_vars, d_weights, L, first_wg, count, d, grid, tile); });
}

int pk_probe_whir_finish(pk_ctx* ctx, const uint64_t* partials, size_t total, unsigned n_wg, unsigned chunk, size_t block_stride, unsigned rows,
                         unsigned count, unsigned row_stride, uint64_t* out) {
    if (!ctx || !partials || !out || !n_wg || !chunk || n_wg % chunk || !rows || !count || count > row_stride) return PK_ERR_BAD_ARG;
    // the last element the kernel reads: block n_wg / chunk - 1, output (rows - 1, count - 1), workgroup chunk - 1
    const size_t last = (size_t)(n_wg / chunk - 1) * block_stride + ((size_t)(rows - 1) * row_stride + (count - 1)) * chunk + (chunk - 1);
    if (last >= total) return PK_ERR_BAD_ARG;
    const size_t res = (size_t)rows * count;
    return slice_probe(
        ctx, total + res, total, res, out, nullptr, [&](uint64_t* d) { return pk_memcpy_h2d(ctx, d, partials, 32 * total); },
        [&](uint64_t* d) {
            pkw::finish_launch(nullptr, d, n_wg, rows, count, row_stride, d + 4 * total, count, chunk, block_stride);
            return hipGetLastError() == hipSuccess ? (int)PK_OK : (int)PK_ERR_HIP;
        });
}

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
