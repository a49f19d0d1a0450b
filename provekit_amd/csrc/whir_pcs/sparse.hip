// sparse.hip -- the kernels of a linear statement whose weights are SPARSE: lists of (index, value) pairs instead of dense tables
// (pkw_open_sparse, pkw_sparse_sums, pkw_sparse_accumulate, pkw_sparse_evaluate; include/provekit_whir_sparse.h).  Each is the twin of
// a dense kernel and gives its bits on the densified table, in O(nnz) instead of O(2^n_vars).
//
// Validation.  No kernel below reads or writes through an index the validation pass has not seen: one lane per entry checks
// index < 2^n_vars and, inside a weight, index > the entry before it (read from global memory, so a pair across two workgroups is
// judged like any other), and the smallest offending entry number reaches the host through one 64-bit minimum.
//
// Sums.  A lane takes an entry: it loads index and value once, gathers that position from each of the `batch` polynomials (32
// bytes as two 16-byte loads; neighbouring entries of an increasing list hit neighbouring lines) and adds the products to one dot29
// per polynomial (linear_tile.hpp's tile, B x 1; B <= 2, so three or four polynomials take two slices of the grid and load an
// entry's index and value once per slice).  Workgroup x of weight y takes the entries x * 256 + lane of that weight, then
// strides by the grid; a workgroup beyond its weight's entries still writes its partial, a zero.  One workgroup reduction per
// (polynomial, weight), one partial per (polynomial, weight, workgroup) in rows of SPARSE_PASS, and evaluate.hip's finish kernel
// adds them.
//
// Accumulation.  table[index[k]] += scale * value[k].  There are no 256-bit atomics, so the race is excluded by construction: ONE
// launch per weight, in stream order.  Inside a launch the indexes are strictly increasing (validated), hence distinct: every
// position has at most one lane reading and writing it; across launches the stream orders them.
//
// Evaluation.  sum_k value[k] * eq(index[k], point) without n_vars products per entry: the index splits into chunks of 8 bits,
// a workgroup builds each chunk's 2^8-entry eq table in LDS in its prologue (every entry the product of two 16-entry halves, as
// mle_eval_kernel builds eq_lo), and an entry then costs one product per further chunk and one dot29 step with its value.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "block_sum.hpp"
#include "blocking.hpp"
#include "evaluate.hpp"
#include "pcs.hpp"
#include "sparse.hpp"

using namespace pk;

namespace pkw {

namespace {

constexpr unsigned THREADS = SPARSE_THREADS;

struct Spans {  // a launch's weights: where their entries start and how many they are
    unsigned long long begin[SPARSE_PASS], nnz[SPARSE_PASS];
};
struct Bounds {  // every weight's first entry, and the end: the validation pass covers all l at once
    unsigned long long at[PKW_MAX_WEIGHTS + 1];
};

// *slot = min(*slot, k) over the entries k that break the rule
__global__ __launch_bounds__(THREADS) void sparse_validate_kernel(const uint32_t* __restrict__ index, Bounds b, unsigned l, unsigned n_vars,
                                                                  unsigned long long* __restrict__ slot) {
    const unsigned long long total = b.at[l];
    for (unsigned long long k = (unsigned long long)blockIdx.x * THREADS + threadIdx.x; k < total; k += (unsigned long long)gridDim.x * THREADS) {
        const uint32_t at = index[k];
        bool first = false;
        for (unsigned i = 0; i < l; i++) first |= b.at[i] == k;  // uniform bounds, a handful of scalar compares
        if ((at >> n_vars) != 0 || (!first && index[k - 1] >= at)) atomicMin(slot, k);
    }
}

struct Polys {
    const fe* p[SPARSE_MAX_BATCH];
};

// partial[(b * SPARSE_PASS + blockIdx.y) * gridDim.x + blockIdx.x] = this workgroup's share of <w_y, f_b> for the B polynomials
// b = blockIdx.z * B + u < batch.  B is 1 or 2: four dot29 in one lane sit at the 256-VGPR ceiling (one wave per SIMD, the worst
// place for a gather), so three or four polynomials are two slices of two; a slot beyond batch repeats polynomial b0 and is not stored
template <int B>
__global__ __launch_bounds__(THREADS) void sparse_sums_kernel(Polys polys, unsigned batch, const uint32_t* __restrict__ index,
                                                              const fe* __restrict__ value, Spans s, fe* __restrict__ partial) {
    __shared__ fe red[B][4];
    const unsigned tid = threadIdx.x, wg = blockIdx.x, y = blockIdx.y, b0 = blockIdx.z * B;
    const fe* f[B];
#pragma unroll
    for (int u = 0; u < B; u++) f[u] = polys.p[b0 + u < batch ? b0 + u : b0];
    const uint32_t* idx = index + s.begin[y];
    const fe* val = value + s.begin[y];
    const size_t nnz = s.nnz[y];
    SparseTile<B> t;
    wsum_tile_init(t);
    for (size_t k = (size_t)wg * THREADS + tid; k < nnz; k += (size_t)gridDim.x * THREADS) {
        const size_t x = idx[k];
        fe fv[B];
        const fe v = fe_load(val + k);
#pragma unroll
        for (int u = 0; u < B; u++) fv[u] = fe_load(f[u] + x);
        sparse_tile_step(t, fv, v);
    }
#pragma unroll
    for (int u = 0; u < B; u++) {
        const fe sum = block_sum(wsum_tile_result(t, u, 0), red[u]);
        if (tid == 0 && b0 + u < batch) fe_store(partial + ((size_t)(b0 + u) * SPARSE_PASS + y) * gridDim.x + wg, sum);
    }
}

__global__ __launch_bounds__(THREADS) void sparse_accumulate_kernel(fe* __restrict__ table, const uint32_t* __restrict__ index, const fe* __restrict__ value,
                                                                    size_t nnz, fe scale) {
    const fe29 sc = unpack29<5>(scale);
    for (size_t k = (size_t)blockIdx.x * THREADS + threadIdx.x; k < nnz; k += (size_t)gridDim.x * THREADS) {
        fe* at = table + index[k];
        const fe prod = pack_canon29(mont261_29(unpack29<0>(fe_load(value + k)), sc));
        fe_store(at, fe_add(fe_load(at), prod));
    }
}

// prod_j (bit j of x ? r : 1 - r) with r = pt[var0 - j], `bits` variables; var0 <-> bit 0
__device__ __forceinline__ fe eq_bits(const fe* pt, int var0, unsigned bits, unsigned x) {
    fe acc = fe_one();
    for (unsigned j = 0; j < bits; j++) {
        const fe r = fe_load(pt + (var0 - (int)j));
        acc = fe_mulx(acc, (x >> j) & 1 ? r : fe_sub(fe_one(), r));
    }
    return acc;
}

// partial[blockIdx.y * gridDim.x + blockIdx.x] = this workgroup's share of weight blockIdx.y's extension at `point`
__global__ __launch_bounds__(THREADS) void sparse_evaluate_kernel(const uint32_t* __restrict__ index, const fe* __restrict__ value, Spans s,
                                                                  const fe* __restrict__ point, unsigned n, fe* __restrict__ partial) {
    __shared__ fe tab[SPARSE_MAX_CHUNKS][1u << SPARSE_CHUNK_BITS];
    __shared__ fe half[SPARSE_MAX_CHUNKS][2][16];
    __shared__ fe red[4];
    const unsigned tid = threadIdx.x, wg = blockIdx.x, y = blockIdx.y;
    const unsigned chunks = (n + SPARSE_CHUNK_BITS - 1) / SPARSE_CHUNK_BITS;
    if (tid < chunks * 32) {  // chunk c = bits [8 c, 8 c + bits): a low half of min(bits, 4) and a high half of the rest
        const unsigned c = tid >> 5, h = (tid >> 4) & 1, x = tid & 15;
        const unsigned bits = n - c * SPARSE_CHUNK_BITS < SPARSE_CHUNK_BITS ? n - c * SPARSE_CHUNK_BITS : SPARSE_CHUNK_BITS;
        const unsigned lo = bits < 4 ? bits : 4, mine = h ? bits - lo : lo;
        const int var0 = (int)n - 1 - (int)(c * SPARSE_CHUNK_BITS + (h ? lo : 0));
        half[c][h][x] = x < (1u << mine) ? eq_bits(point, var0, mine, x) : fe_zero();
    }
    __syncthreads();
    for (unsigned c = 0; c < chunks; c++) tab[c][tid] = fe_mulx(half[c][1][tid >> 4], half[c][0][tid & 15]);
    __syncthreads();

    const uint32_t* idx = index + s.begin[y];
    const fe* val = value + s.begin[y];
    const size_t nnz = s.nnz[y];
    dot29 d;
    dot29_init(d);
    for (size_t k = (size_t)wg * THREADS + tid; k < nnz; k += (size_t)gridDim.x * THREADS) {
        const uint32_t x = idx[k];
        fe e = chunks ? tab[0][x & 255] : fe_one();
        for (unsigned c = 1; c < chunks; c++) e = fe_mulx(e, tab[c][(x >> (c * SPARSE_CHUNK_BITS)) & 255]);
        dot29_add(d, unpack29<0>(e), unpack29<5>(fe_load(val + k)));
    }
    const fe sum = block_sum(dot29_result(d), red);
    if (tid == 0) fe_store(partial + (size_t)y * gridDim.x + wg, sum);
}

size_t max_nnz(const SparseWeights& w, unsigned i0, unsigned L) {
    size_t m = 0;
    for (unsigned i = 0; i < L; i++) m = std::max(m, w.nnz(i0 + i));
    return m;
}
Spans spans(const SparseWeights& w, unsigned i0, unsigned L) {
    Spans s{};
    for (unsigned i = 0; i < L; i++) s.begin[i] = w.begin(i0 + i), s.nnz[i] = w.nnz(i0 + i);
    return s;
}

}  // namespace

unsigned sparse_grid(unsigned n_vars, size_t nnz, unsigned steps) {
    const size_t per = (size_t)THREADS * steps, want = (nnz + per - 1) / per, cap = wsum_grid(n_vars);
    return (unsigned)(want < 1 ? 1 : want < cap ? want : cap);
}

size_t sparse_partial_fes(unsigned batch, unsigned n_vars) { return (size_t)batch * SPARSE_PASS * wsum_grid(n_vars); }

int sparse_validate(pk_ctx* ctx, hipStream_t stream, const SparseWeights& w, unsigned n_vars, uint64_t* d_slot, size_t* bad, uint32_t* at, uint32_t* prev) {
    *bad = ~(size_t)0;
    const size_t total = w.total();
    if (!total) return PK_OK;
    Bounds b{};
    for (unsigned i = 0; i <= w.l; i++) b.at[i] = w.offsets[i];
    if (hipMemsetAsync(d_slot, 0xff, 8, stream) != hipSuccess) return PK_ERR_HIP;
    sparse_validate_kernel<<<capped_grid(total), THREADS, 0, stream>>>(w.index, b, w.l, n_vars, (unsigned long long*)d_slot);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return PK_ERR_HIP;
    uint64_t k = 0;
    int rc = pk_memcpy_d2h(ctx, &k, d_slot, 8);
    if (rc || k == ~(uint64_t)0) return rc;
    if (k >= total) return PK_ERR_HIP;  // the kernel reports entries only
    *bad = (size_t)k;
    *prev = 0;
    rc = pk_memcpy_d2h(ctx, at, w.index + k, 4);
    bool first = false;
    for (unsigned i = 0; i < w.l; i++) first |= w.offsets[i] == k;
    if (!rc && !first) rc = pk_memcpy_d2h(ctx, prev, w.index + k - 1, 4);
    return rc;
}

int sparse_sums_launch(hipStream_t stream, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const SparseWeights& w, uint64_t* d_partial,
                       uint64_t* d_out, unsigned grid) {
    if (batch < 1 || batch > SPARSE_MAX_BATCH || grid > wsum_grid(n_vars)) return PK_ERR_BAD_ARG;  // the scratch is sized for wsum_grid
    Polys polys{};
    for (unsigned b = 0; b < batch; b++) polys.p[b] = (const fe*)d_evals[b];
    for (unsigned i0 = 0; i0 < w.l; i0 += SPARSE_PASS) {  // stream order keeps a pass's partials until the finish kernel has read them
        const unsigned L = w.l - i0 < SPARSE_PASS ? w.l - i0 : SPARSE_PASS;
        const unsigned g = grid ? grid : sparse_grid(n_vars, max_nnz(w, i0, L), 1);
        const Spans s = spans(w, i0, L);
        if (batch == 1)
            sparse_sums_kernel<1><<<dim3(g, L, 1), THREADS, 0, stream>>>(polys, batch, w.index, (const fe*)w.value, s, (fe*)d_partial);
        else
            sparse_sums_kernel<(int)SPARSE_TILE_B><<<dim3(g, L, (batch + SPARSE_TILE_B - 1) / SPARSE_TILE_B), THREADS, 0, stream>>>(polys, batch, w.index, (const fe*)w.value, s, (fe*)d_partial);
        finish_launch(stream, d_partial, g, batch, L, SPARSE_PASS, d_out + 4 * (size_t)i0, w.l);
        if (hipGetLastError() != hipSuccess) return PK_ERR_HIP;  // a failed pass ends the launch: nothing more is enqueued
    }
    return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP;
}

int sparse_accumulate_launch(hipStream_t stream, uint64_t* d_table, const SparseWeights& w, const uint64_t* scales) {
    for (unsigned i = 0; i < w.l; i++) {  // one launch per weight: see the head of this file
        const size_t nnz = w.nnz(i);
        if (!nnz) continue;
        sparse_accumulate_kernel<<<capped_grid(nnz), THREADS, 0, stream>>>((fe*)d_table, w.index + w.begin(i), (const fe*)w.value + w.begin(i), nnz,
                                                                           h_load(scales + 4 * (size_t)i));
    }
    return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP;
}

int sparse_evaluate_launch(hipStream_t stream, unsigned n_vars, const SparseWeights& w, const uint64_t* d_point, uint64_t* d_partial, uint64_t* d_out) {
    for (unsigned i0 = 0; i0 < w.l; i0 += SPARSE_PASS) {
        const unsigned L = w.l - i0 < SPARSE_PASS ? w.l - i0 : SPARSE_PASS;
        const unsigned g = sparse_grid(n_vars, max_nnz(w, i0, L), SPARSE_EVAL_STEPS);
        sparse_evaluate_kernel<<<dim3(g, L), THREADS, 0, stream>>>(w.index, (const fe*)w.value, spans(w, i0, L), (const fe*)d_point, n_vars, (fe*)d_partial);
        finish_launch(stream, d_partial, g, 1, L, SPARSE_PASS, d_out + 4 * (size_t)i0, w.l);
        if (hipGetLastError() != hipSuccess) return PK_ERR_HIP;  // a failed pass ends the launch: nothing more is enqueued
    }
    return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP;
}

// ---- pkw_sparse_sums, pkw_sparse_accumulate and pkw_sparse_evaluate ----------------------------------------------------------------

namespace {

// what the three share: the arguments' rule, and the validation pass followed by the entry's own launch, both on the null stream
// and finished on return
template <class Launch>
int sparse_blocking(pk_ctx* ctx, const SparseWeights& w, unsigned n_vars, uint64_t* d_slot, Launch launch) {
    return run_blocking(ctx, [&] {  // the operands are the context's work: finished before a kernel reads them
        size_t bad = 0;
        uint32_t at = 0, prev = 0;
        if (int rc = sparse_validate(ctx, nullptr, w, n_vars, d_slot, &bad, &at, &prev)) return rc;
        if (bad != ~(size_t)0) return refuse(sparse_index_reason(w, bad, at, prev, n_vars));
        return launch();
    });
}
int sparse_args(pk_ctx* ctx, unsigned n_vars, const uint64_t* offsets, const uint32_t* d_index, const uint64_t* d_value, unsigned l) {
    std::string why;
    if (!ctx || !offsets) return refuse("null pointer");
    if (n_vars > 30) return refuse("n_vars must be 0..30");
    if (l > PKW_MAX_WEIGHTS) return refuse("the number of weights must be 0..16");
    if (!sparse_offsets_ok(offsets, l, n_vars, why)) return refuse(why);
    if (offsets[l] && (!d_index || !d_value)) return refuse("null index or value list");
    return PK_OK;
}

}  // namespace
}  // namespace pkw

extern "C" {

int pkw_sparse_sums(pk_ctx* ctx, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* offsets, const uint32_t* d_index,
                    const uint64_t* d_value, unsigned l, uint64_t* out) {
    if (int rc = pkw::sparse_args(ctx, n_vars, offsets, d_index, d_value, l)) return rc;
    if (!d_evals || (l && !out) || batch < 1 || batch > pkw::SPARSE_MAX_BATCH) return pkw::refuse("the number of polynomials must be 1..4, none null");
    for (unsigned b = 0; b < batch; b++)
        if (!d_evals[b]) return pkw::refuse("null polynomial");
    if (!l) return PK_OK;
    const size_t part = pkw::sparse_partial_fes(batch, n_vars), res = (size_t)batch * l;
    pkw::Scratch d(ctx, part + res + 1);
    if (d.rc) return d.rc;
    uint64_t *d_part = d.take(part), *d_res = d.take(res), *d_slot = d.take(1);
    const pkw::SparseWeights w{offsets, d_index, d_value, l};
    const int rc = pkw::sparse_blocking(ctx, w, n_vars, d_slot, [&] { return pkw::sparse_sums_launch(nullptr, d_evals, batch, n_vars, w, d_part, d_res); });
    return rc ? rc : pk_memcpy_d2h(ctx, out, d_res, 32 * res);
}

int pkw_sparse_accumulate(pk_ctx* ctx, uint64_t* d_table, unsigned n_vars, const uint64_t* offsets, const uint32_t* d_index, const uint64_t* d_value, unsigned l,
                          const uint64_t* scales) {
    if (int rc = pkw::sparse_args(ctx, n_vars, offsets, d_index, d_value, l)) return rc;
    if (!d_table || (l && !scales)) return pkw::refuse("null pointer");
    for (unsigned i = 0; i < l; i++)
        if (!pkw::below_p(pk::h_load(scales + 4 * (size_t)i))) return pkw::refuse("scale " + std::to_string(i) + " is not below p");
    if (!l || !offsets[l]) return PK_OK;
    pkw::Scratch d(ctx, 1);
    if (d.rc) return d.rc;
    const pkw::SparseWeights w{offsets, d_index, d_value, l};
    return pkw::sparse_blocking(ctx, w, n_vars, d.take(1), [&] { return pkw::sparse_accumulate_launch(nullptr, d_table, w, scales); });
}

int pkw_sparse_evaluate(pk_ctx* ctx, unsigned n_vars, const uint64_t* offsets, const uint32_t* d_index, const uint64_t* d_value, unsigned l, const uint64_t* point,
                        uint64_t* out) {
    if (int rc = pkw::sparse_args(ctx, n_vars, offsets, d_index, d_value, l)) return rc;
    if ((n_vars && !point) || (l && !out)) return pkw::refuse("null pointer");
    if (!l) return PK_OK;
    const size_t part = pkw::sparse_partial_fes(1, n_vars), pts = n_vars ? n_vars : 1;
    pkw::Scratch d(ctx, part + pts + l + 1);
    if (d.rc) return d.rc;
    uint64_t *d_part = d.take(part), *d_pt = d.take(pts), *d_res = d.take(l), *d_slot = d.take(1);
    const pkw::SparseWeights w{offsets, d_index, d_value, l};
    if (n_vars)
        if (int rc = pk_memcpy_h2d(ctx, d_pt, point, 32 * (size_t)n_vars)) return rc;
    const int rc = pkw::sparse_blocking(ctx, w, n_vars, d_slot, [&] { return pkw::sparse_evaluate_launch(nullptr, n_vars, w, d_pt, d_part, d_res); });
    return rc ? rc : pk_memcpy_d2h(ctx, out, d_res, 32 * (size_t)l);
}

}  // extern "C"
