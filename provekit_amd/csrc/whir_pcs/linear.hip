// linear.hip -- the two kernels of a LINEAR statement <w_i, f_b> = s_{b,i} over dense weight tables (pkw_open_linear, pkw_weighted_sums).
//
// Weighted sums.  The public route to the batch * l sums is batch * l calls of pk_dot: every polynomial read l times, every weight
// batch times, 81 multiply-adds per 64 loaded bytes.  Here a lane keeps a register tile of TB polynomials x TW weights, one dot29
// (fe29.hpp: 17 column accumulators, one Montgomery reduction per DOT29_GROUP products) per pair: per step it loads ONE element of
// each tiled operand (32 bytes as two 16-byte loads, 8 KiB contiguous per workgroup and operand) and makes TB * TW products of them,
// so each polynomial is read ceil(l / TW) times and each weight ceil(batch / TB) times.  Workgroup x of the grid takes the elements
// x * 256 + lane, then strides by the grid: no cross-lane traffic per step, one workgroup reduction per output at the end, one
// partial per (output, workgroup), and evaluate.hip's finish kernel adds them.  Every partial is a fully
// reduced field element and field addition is exact, so the result does not depend on the grid.  Tile slots beyond batch or l
// repeat the tile's first operand and are not stored; a single polynomial therefore takes a 1 x 4 tile, not 2 x 2 (wsum_launch).
//
// Combination.  W[x] (+)= sum_i s_i w_i[x] in one pass: folding l weights into the sumcheck weight table by l calls of pk_fe_axpy
// moves 96 l bytes per element, this moves 32 (l + 2).  The scalars sit in LDS pre-shifted (unpack29<5>) and are read as a
// broadcast; a lane owns one element per step and one dot29.
#include <hip/hip_runtime.h>

#include <cstring>

#include "block_sum.hpp"
#include "blocking.hpp"
#include "evaluate.hpp"
#include "linear.hpp"
#include "linear_tile.hpp"

using namespace pk;

namespace pkw {

namespace {

constexpr unsigned THREADS = 256;

struct WsumArgs {
    const fe* f[WSUM_MAX_BATCH];
    const fe* w[WSUM_PASS];
};

// partial[((b * L + i) * gridDim.x + blockIdx.x] = the share of workgroup first_wg + blockIdx.x of a grid of n_wg of <w_i, f_b>, b < batch,
// i < L (the pass's weights).  The whole grid is first_wg = 0 and gridDim.x = n_wg; a rank of a device set launches its slice
template <int TB, int TW>
__global__ __launch_bounds__(THREADS) void weighted_sums_kernel(WsumArgs a, unsigned batch, unsigned L, size_t N, unsigned first_wg, unsigned n_wg,
                                                                fe* __restrict__ partial) {
    __shared__ fe red[TB * TW][4];
    const unsigned tid = threadIdx.x, wg = first_wg + blockIdx.x;
    const unsigned w_tiles = (L + TW - 1) / TW;
    const unsigned b0 = (blockIdx.y / w_tiles) * TB, i0 = (blockIdx.y % w_tiles) * TW;
    const fe* f[TB];
    const fe* w[TW];
#pragma unroll
    for (int u = 0; u < TB; u++) f[u] = a.f[b0 + u < batch ? b0 + u : b0];
#pragma unroll
    for (int v = 0; v < TW; v++) w[v] = a.w[i0 + v < L ? i0 + v : i0];
    WsumTile<TB, TW> t;
    wsum_tile_init(t);
    for (size_t x = (size_t)wg * THREADS + tid; x < N; x += (size_t)n_wg * THREADS) {
        fe fv[TB], wv[TW];
#pragma unroll
        for (int u = 0; u < TB; u++) fv[u] = fe_load(f[u] + x);
#pragma unroll
        for (int v = 0; v < TW; v++) wv[v] = fe_load(w[v] + x);
        wsum_tile_step(t, fv, wv);
    }
#pragma unroll
    for (int u = 0; u < TB; u++)
#pragma unroll
        for (int v = 0; v < TW; v++) {
            const fe s = block_sum(wsum_tile_result(t, u, v), red[u * TW + v]);
            if (tid == 0 && b0 + u < batch && i0 + v < L) fe_store(partial + ((size_t)(b0 + u) * L + (i0 + v)) * gridDim.x + blockIdx.x, s);
        }
}

struct CombArgs {
    const fe* w[COMB_TILE];
    fe s[COMB_TILE];
};

__global__ __launch_bounds__(THREADS) void combine_kernel(fe* __restrict__ dst, size_t len, CombArgs a, unsigned L, int accumulate) {
    __shared__ fe29 sc[COMB_TILE];
    if (threadIdx.x < L) sc[threadIdx.x] = unpack29<5>(a.s[threadIdx.x]);
    __syncthreads();
    for (size_t x = (size_t)blockIdx.x * THREADS + threadIdx.x; x < len; x += (size_t)gridDim.x * THREADS) {
        dot29 d;
        dot29_init(d);
        for (unsigned i = 0; i < L; i++) dot29_add(d, unpack29<0>(fe_load(a.w[i] + x)), sc[i]);
        fe r = dot29_result(d);
        if (accumulate) r = fe_add(r, fe_load(dst + x));
        fe_store(dst + x, r);
    }
}

template <int TB, int TW>
void wsum_pass(hipStream_t stream, const WsumArgs& a, unsigned batch, unsigned L, size_t N, unsigned grid, unsigned first_wg, unsigned count, fe* partial) {
    const unsigned tiles = ((batch + TB - 1) / TB) * ((L + TW - 1) / TW);
    weighted_sums_kernel<TB, TW><<<dim3(count, tiles), THREADS, 0, stream>>>(a, batch, L, N, first_wg, grid, partial);
}
// tile 0: 2 x 2, except that ONE polynomial takes 1 x 4 -- half of a 2 x 2 tile's products would repeat its first row
void wsum_pass_tiled(hipStream_t stream, const WsumArgs& a, unsigned batch, unsigned L, size_t N, unsigned grid, unsigned first_wg, unsigned count,
                     fe* partial, int tile) {
    if (tile == 1 || (tile == 0 && batch == 1))
        wsum_pass<1, 4>(stream, a, batch, L, N, grid, first_wg, count, partial);
    else if (tile == 2)
        wsum_pass<2, 1>(stream, a, batch, L, N, grid, first_wg, count, partial);
    else
        wsum_pass<(int)WSUM_TILE_B, (int)WSUM_TILE_W>(stream, a, batch, L, N, grid, first_wg, count, partial);
}

}  // namespace

unsigned wsum_grid(unsigned n_vars) {
    if (n_vars <= WSUM_LOW_VARS) return 1;
    const unsigned steps = n_vars - WSUM_LOW_VARS;
    return steps >= 9 ? WSUM_MAX_WG : 1u << steps;
}

size_t wsum_partial_fes(unsigned batch, unsigned n_vars) { return (size_t)batch * WSUM_PASS * wsum_grid(n_vars); }

int wsum_launch(hipStream_t stream, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* const* d_weights, unsigned l,
                uint64_t* d_partial, uint64_t* d_out, unsigned grid, int tile) {
    if (batch < 1 || batch > WSUM_MAX_BATCH || grid > wsum_grid(n_vars)) return PK_ERR_BAD_ARG;  // the scratch is sized for wsum_grid
    if (!grid) grid = wsum_grid(n_vars);
    const size_t N = (size_t)1 << n_vars;
    WsumArgs a{};
    for (unsigned b = 0; b < batch; b++) a.f[b] = (const fe*)d_evals[b];
    for (unsigned i0 = 0; i0 < l; i0 += WSUM_PASS) {  // stream order keeps a pass's partials until the finish kernel has read them
        const unsigned L = l - i0 < WSUM_PASS ? l - i0 : WSUM_PASS;
        for (unsigned i = 0; i < L; i++) a.w[i] = (const fe*)d_weights[i0 + i];
        wsum_pass_tiled(stream, a, batch, L, N, grid, 0, grid, (fe*)d_partial, tile);
        finish_launch(stream, d_partial, grid, batch, L, L, d_out + 4 * (size_t)i0, l);
    }
    return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP;
}

int wsum_slice_launch(hipStream_t stream, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* const* d_weights, unsigned L,
                      unsigned first_wg, unsigned count, uint64_t* d_partial, unsigned grid, int tile) {
    if (!grid) grid = wsum_grid(n_vars);
    if (batch < 1 || batch > WSUM_MAX_BATCH || L < 1 || L > WSUM_PASS || grid > wsum_grid(n_vars) || !count || count > grid || first_wg > grid - count)
        return PK_ERR_BAD_ARG;
    WsumArgs a{};
    for (unsigned b = 0; b < batch; b++) a.f[b] = (const fe*)d_evals[b];
    for (unsigned i = 0; i < L; i++) a.w[i] = (const fe*)d_weights[i];
    wsum_pass_tiled(stream, a, batch, L, (size_t)1 << n_vars, grid, first_wg, count, (fe*)d_partial, tile);
    return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP;
}

int combine_launch(hipStream_t stream, uint64_t* d_w, size_t len, const uint64_t* const* d_weights, const uint64_t* scales, unsigned l, int accumulate) {
    if (!len) return PK_OK;
    const unsigned grid = capped_grid(len);
    if (!l && !accumulate) return hipMemsetAsync(d_w, 0, 32 * len, stream) == hipSuccess ? PK_OK : PK_ERR_HIP;
    for (unsigned i0 = 0; i0 < l; i0 += COMB_TILE) {
        const unsigned L = l - i0 < COMB_TILE ? l - i0 : COMB_TILE;
        CombArgs a{};
        for (unsigned i = 0; i < L; i++) {
            a.w[i] = (const fe*)d_weights[i0 + i];
            memcpy(a.s[i].v, scales + 4 * (size_t)(i0 + i), 32);
        }
        combine_kernel<<<grid, THREADS, 0, stream>>>((fe*)d_w, len, a, L, accumulate || i0 > 0);
    }
    return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP;
}

}  // namespace pkw

extern "C" {

int pkw_weighted_sums(pk_ctx* ctx, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* const* d_weights, unsigned l,
                      uint64_t* out) {
    if (!ctx || !d_evals || !d_weights || !out || batch < 1 || batch > pkw::WSUM_MAX_BATCH || n_vars > 30 || l < 1) return PK_ERR_BAD_ARG;
    for (unsigned b = 0; b < batch; b++)
        if (!d_evals[b]) return PK_ERR_BAD_ARG;
    for (unsigned i = 0; i < l; i++)
        if (!d_weights[i]) return PK_ERR_BAD_ARG;
    const size_t part = pkw::wsum_partial_fes(batch, n_vars), res = (size_t)batch * l;
    pkw::Scratch d(ctx, part + res);
    if (d.rc) return d.rc;
    uint64_t *d_part = d.take(part), *d_res = d.take(res);
    // the operands are the context's work: finished before the kernel reads them
    if (int rc = pkw::run_blocking(ctx, [&] { return pkw::wsum_launch(nullptr, d_evals, batch, n_vars, d_weights, l, d_part, d_res); })) return rc;
    return pk_memcpy_d2h(ctx, out, d_res, 32 * res);
}

}  // extern "C"
