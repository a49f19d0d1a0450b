// evaluate.hip -- the one HIP kernel pair libprovekit_whir.so adds: the multilinear extensions of up to 4 polynomials at up to 8
// points in ONE pass over each polynomial (pkw_evaluate; a further pass per 8 points beyond that).
//
// The route through the product's public API is q x (pk_eq_table + pk_dot) per polynomial: q tables of 2^n elements written and
// read back, the polynomial read q times.  Here an index splits as  i = (wg : g : t)  with t the LOW_VARS = 8 low bits (a tile of
// 256 contiguous evaluations), g the next c <= 6 bits (the 2^c tiles one workgroup streams) and wg the rest, and
//     f(z) = sum_wg eq_top(wg) * sum_t eq_lo(t) * [ sum_g eq_mid(g) * f[wg : g : t] ] .
// Lane t of a 256-lane workgroup owns position t of every tile: it loads f[wg : g : t] for four tiles at a time (32 contiguous
// bytes per lane as two 16-byte loads, 8 KiB contiguous per workgroup and tile), and for each point adds the four products with
// eq_mid(g) into the 17 column accumulators of fe29.hpp's 9 x 29-bit form before ONE Montgomery reduction (dot29's scheme: 81
// multiply-adds per element and point plus a quarter of a reduction, against two full products per element on the table route).
// eq_mid(g) is the same for all lanes: it sits in LDS pre-shifted (unpack29<5>) and is read as a broadcast.  The bracket stays
// in registers (9 limbs per point); eq_lo(t), which every lane needs once, is the product of two 16-entry tables (4 + 4 variables)
// in LDS, eq_top(wg) one element per point.  So no cross-lane traffic happens per tile: one workgroup reduction per point at the end,
// one partial per (polynomial, point, workgroup), and finish_kernel adds the partials -- here and for every other kernel of the
// library that leaves one partial per (output, workgroup): linear.hip's sums, sparse.hip's sums and evaluation.
// LDS: 18 KiB eq_mid + 8 KiB eq_lo halves + 1.3 KiB -- not the 64 KiB that whole 2^8-entry tables for 8 points would take -- so LDS
// never limits occupancy; the registers do (DESIGN.md 11 records the compiled numbers).
//
// Sizes below 2^8: the same kernel with the tile clamped to 2^n_vars (lanes beyond it idle).
#include <hip/hip_runtime.h>

#include "../fe29.hpp"
#include "block_sum.hpp"
#include "blocking.hpp"
#include "evaluate.hpp"

using namespace pk;

namespace pkw {

namespace {

struct Split {
    unsigned b, bl, bh;  // low variables (tile = 2^b), split bl + bh for the two halves of eq_lo
    unsigned c;          // tiles per workgroup = 2^c
    unsigned top;        // workgroups = 2^top
};
Split split_for(unsigned n) {
    Split s;
    s.b = n < EVAL_LOW_VARS ? n : EVAL_LOW_VARS;
    s.bl = s.b / 2;
    s.bh = s.b - s.bl;
    const unsigned rest = n - s.b;
    // enough workgroups to fill 256 CUs twice over before a workgroup takes more tiles; at most 2^6 tiles (18 KiB of eq_mid)
    s.c = rest > 9 ? (rest - 9 < EVAL_MAX_MID ? rest - 9 : EVAL_MAX_MID) : 0;
    s.top = rest - s.c;
    return s;
}

struct Polys {
    const fe* p[EVAL_MAX_BATCH];
};

// prod_k (bit k of idx ? r : 1 - r) with r = pt[var0 - k]: the eq factor of `nbits` variables, variable var0 <-> bit 0
__device__ __forceinline__ fe eq_bits(const fe* pt, int var0, unsigned nbits, unsigned idx) {
    fe acc = fe_one();
    for (unsigned k = 0; k < nbits; k++) {
        const fe r = fe_load(pt + (var0 - (int)k));
        acc = fe_mulx(acc, (idx >> k) & 1 ? r : fe_sub(fe_one(), r));
    }
    return acc;
}

constexpr unsigned THREADS = 256, MID_SLOTS = 1u << EVAL_MAX_MID;

// partial[(blockIdx.y * EVAL_PASS + i) * gridDim.x + blockIdx.x] = the share of workgroup first_wg + blockIdx.x of the 2^s.top at point
// i < Q of poly blockIdx.y.  The whole grid is first_wg = 0 and gridDim.x = 2^s.top; a rank of a device set launches its slice
__global__ __launch_bounds__(THREADS) void mle_eval_kernel(Polys polys, const fe* __restrict__ points, unsigned Q, unsigned n, Split s, unsigned first_wg,
                                                           fe* __restrict__ partial) {
    __shared__ fe29 mid[EVAL_PASS][MID_SLOTS];
    __shared__ fe lo[EVAL_PASS][2][16];
    __shared__ fe top[EVAL_PASS];
    __shared__ fe red[EVAL_PASS][4];
    const unsigned tid = threadIdx.x, wg = first_wg + blockIdx.x;
    const unsigned n_mid = 1u << s.c, n_lo = 1u << s.bl, n_hi = 1u << s.bh, per = 1 + n_mid + n_lo + n_hi;
    for (unsigned item = tid; item < Q * per; item += THREADS) {
        const unsigned i = item / per, e = item % per;
        const fe* pt = points + (size_t)i * n;
        if (e == 0)
            top[i] = eq_bits(pt, (int)n - 1 - (int)(s.b + s.c), s.top, wg);
        else if (e < 1 + n_mid)
            mid[i][e - 1] = unpack29<5>(eq_bits(pt, (int)n - 1 - (int)s.b, s.c, e - 1));
        else if (e < 1 + n_mid + n_lo)
            lo[i][0][e - 1 - n_mid] = eq_bits(pt, (int)n - 1, s.bl, e - 1 - n_mid);
        else
            lo[i][1][e - 1 - n_mid - n_lo] = eq_bits(pt, (int)n - 1 - (int)s.bl, s.bh, e - 1 - n_mid - n_lo);
    }
    if (n_mid < 4 && tid < Q * 4 && (tid & 3) >= n_mid) {  // the tiles come four at a time: the missing ones count as zero
        fe29 z;
#pragma unroll
        for (int k = 0; k < 9; k++) z.v[k] = 0;
        mid[tid >> 2][tid & 3] = z;
    }
    __syncthreads();

    const fe* f = polys.p[blockIdx.y] + ((size_t)wg << (s.c + s.b));
    const bool live = tid < (1u << s.b);
    fe29 run[EVAL_PASS];
#pragma unroll
    for (int i = 0; i < (int)EVAL_PASS; i++)
#pragma unroll
        for (int k = 0; k < 9; k++) run[i].v[k] = 0;
    for (unsigned g0 = 0; g0 < n_mid; g0 += 4) {
        fe29 x[4];
#pragma unroll
        for (unsigned u = 0; u < 4; u++) {
            fe v = fe_zero();
            if (live && g0 + u < n_mid) v = fe_load(f + (((size_t)(g0 + u)) << s.b) + tid);
            x[u] = unpack29<0>(v);
        }
#pragma unroll
        for (unsigned i = 0; i < EVAL_PASS; i++) {
            if (i < Q) {  // uniform
                u64 acc[17];
#pragma unroll
                for (int k = 0; k < 17; k++) acc[k] = 0;
#pragma unroll
                for (unsigned u = 0; u < 4; u++) {
                    const fe29 y = mid[i][g0 + u];
#pragma unroll
                    for (int a = 0; a < 9; a++)
#pragma unroll
                        for (int c = 0; c < 9; c++) acc[a + c] += (u64)x[u].v[a] * y.v[c];
                }
                // four terms of < 0.19 p each after the reduction, plus p: < 1.76 p; the running sum stays almost reduced (dot29_flush)
                run[i] = add29(run[i], reduce261_29(acc));
                reduce_almost29(run[i]);
            }
        }
    }
#pragma unroll
    for (unsigned i = 0; i < EVAL_PASS; i++) {
        if (i < Q) {  // uniform
            const fe w = fe_mulx(lo[i][1][(tid >> s.bl) & (n_hi - 1)], lo[i][0][tid & (n_lo - 1)]);
            fe v = live ? fe_mulx(pack_canon29(run[i]), w) : fe_zero();
            v = block_sum(v, red[i]);
            if (tid == 0) fe_store(partial + ((size_t)blockIdx.y * EVAL_PASS + i) * gridDim.x + blockIdx.x, fe_mulx(v, top[i]));
        }
    }
}

// out[y * out_stride + i] = sum of the n_wg partials of output (y, i), i < count; one workgroup per output.  The partials lie in
// n_wg / chunk blocks, block_stride elements apart, of `chunk` workgroups each: partial j of the output is element
// (y * row_stride + i) * chunk + j % chunk of block j / chunk.  One block (chunk = n_wg) is a grid's own output; G blocks are what the
// ranks of a device set gathered from their slices.  Lane j adds the partials j, j + 256, ...: field addition is exact, so the
// result depends neither on n_wg nor on how the blocks cut it
__global__ __launch_bounds__(THREADS) void finish_kernel(const fe* __restrict__ partial, unsigned n_wg, unsigned chunk, size_t block_stride, unsigned count,
                                                         unsigned row_stride, fe* __restrict__ out, unsigned out_stride) {
    __shared__ fe red[4];
    const unsigned y = blockIdx.x / count, i = blockIdx.x % count;
    const fe* p = partial + ((size_t)y * row_stride + i) * chunk;
    fe acc = fe_zero();
    for (unsigned j = threadIdx.x; j < n_wg; j += THREADS) acc = fe_add(acc, fe_load(p + (j / chunk) * block_stride + j % chunk));
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) fe_store(out + (size_t)y * out_stride + i, acc);
}

}  // namespace

unsigned eval_grid(unsigned n_vars) { return 1u << split_for(n_vars).top; }

size_t eval_partial_fes(unsigned batch, unsigned n_vars) { return (size_t)batch * EVAL_PASS * eval_grid(n_vars); }

int eval_slice_launch(hipStream_t stream, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* d_points, unsigned Q,
                      unsigned first_wg, unsigned count, uint64_t* d_partial) {
    const Split s = split_for(n_vars);
    if (batch < 1 || batch > EVAL_MAX_BATCH || Q < 1 || Q > EVAL_PASS || !count || first_wg > (1u << s.top) - count) return PK_ERR_BAD_ARG;
    Polys polys{};
    for (unsigned b = 0; b < batch; b++) polys.p[b] = (const fe*)d_evals[b];
    mle_eval_kernel<<<dim3(count, batch), THREADS, 0, stream>>>(polys, (const fe*)d_points, Q, n_vars, s, first_wg, (fe*)d_partial);
    return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP;
}

int eval_launch(hipStream_t stream, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* d_points, unsigned q,
                uint64_t* d_partial, uint64_t* d_out) {
    const Split s = split_for(n_vars);
    const unsigned n_wg = 1u << s.top;
    Polys polys{};
    for (unsigned b = 0; b < batch; b++) polys.p[b] = (const fe*)d_evals[b];
    for (unsigned q0 = 0; q0 < q; q0 += EVAL_PASS) {  // stream order keeps a pass's partials until its finish kernel has read them
        const unsigned Q = q - q0 < EVAL_PASS ? q - q0 : EVAL_PASS;
        mle_eval_kernel<<<dim3(n_wg, batch), THREADS, 0, stream>>>(polys, (const fe*)d_points + (size_t)q0 * n_vars, Q, n_vars, s, 0, (fe*)d_partial);
        finish_launch(stream, d_partial, n_wg, batch, Q, EVAL_PASS, d_out + 4 * (size_t)q0, q);
    }
    return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP;
}

void finish_launch(hipStream_t stream, const uint64_t* d_partial, unsigned n_wg, unsigned rows, unsigned count, unsigned row_stride, uint64_t* d_out,
                   unsigned out_stride, unsigned chunk, size_t block_stride) {
    finish_kernel<<<rows * count, THREADS, 0, stream>>>((const fe*)d_partial, n_wg, chunk ? chunk : n_wg, block_stride, count, row_stride, (fe*)d_out,
                                                        out_stride);
}

}  // namespace pkw

extern "C" {

unsigned pkw_evaluate_low_vars(void) { return pkw::EVAL_LOW_VARS; }

int pkw_evaluate(pk_ctx* ctx, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* points, unsigned q, uint64_t* out) {
    if (!ctx || !d_evals || !points || !out || batch < 1 || batch > pkw::EVAL_MAX_BATCH || n_vars < 1 || n_vars > 30 || q < 1 || q > (1u << 16))
        return PK_ERR_BAD_ARG;
    for (unsigned b = 0; b < batch; b++)
        if (!d_evals[b]) return PK_ERR_BAD_ARG;
    const size_t pts = (size_t)q * n_vars, part = pkw::eval_partial_fes(batch, n_vars), res = (size_t)batch * q;
    pkw::Scratch d(ctx, pts + part + res);
    if (d.rc) return d.rc;
    uint64_t *d_pts = d.take(pts), *d_part = d.take(part), *d_res = d.take(res);
    if (int rc = pk_memcpy_h2d(ctx, d_pts, points, 32 * pts)) return rc;
    // the polynomials are the context's work: finished before the kernel reads them
    if (int rc = pkw::run_blocking(ctx, [&] { return pkw::eval_launch(nullptr, d_evals, batch, n_vars, d_pts, q, d_part, d_res); })) return rc;
    return pk_memcpy_d2h(ctx, out, d_res, 32 * res);
}

}  // extern "C"
