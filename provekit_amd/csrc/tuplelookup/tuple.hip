// tuple.hip -- the HIP kernels libprovekit_tuplelookup.so adds (gfx950): the compressed rows of up to four groups of up to four
// columns, and the multiplicities of a table of rows under those groups.
//
// tuple_leaf_kernel<W>: leaf[g 2^n + x] = alpha - sum_j beta^j col[g][j][x].  The launch's y dimension is the group: a workgroup picks
// its group's W column pointers with wave-uniform selects (no indexed read of the kernel's arguments) and stores at the group's
// offset of the stacked table; side T is the same kernel with one group.  A lane takes LEAF_ITEMS rows a workgroup-width apart: every
// load and store is coalesced across the lanes, and all W * LEAF_ITEMS loads are issued before the first product.  The row is
// compressed by Horner's rule in beta, from column W - 1 down: W - 1 Montgomery products, none at W = 1.  Products, sums and
// differences of values below p are exact values below p: the bits depend neither on the grid nor on the rows per lane.
//
// tuple_count_kernel<W, LDS>: one pass over idx[g], f[g][*] and the gathered t[*][idx].  A lane validates its row: idx[g][x] < 2^k
// BEFORE it is followed, then all W columns of the row against the row of t it names, on the stored words.  A failure lowers the
// 64-bit cell `bad` with atomicMin to the stacked index g 2^n + x, so the cell ends as the smallest failing one.  Valid rows are
// counted, all groups into the one counts array: tables of k <= COUNT_LDS_MAX_K in a workgroup-private LDS histogram that is flushed
// once per non-zero bin, larger ones with atomics on device memory.  As in lookup/lookup.hip, a wavefront whose valid lanes all name
// one bin keeps (bin, count) in wave-uniform registers across its iterations and adds when the bin changes and at its end: one atomic
// per wavefront under full skew.  A wavefront with mixed bins adds lane by lane.  Integer adds: the counts are exact in any order.
// mont_kernel then writes m as Montgomery elements.
//
// All stores are ordinary vector stores; the atomics are vector atomics on device memory or LDS.
#include <hip/hip_runtime.h>

#include "../fe29.hpp"
#include "kernels.hpp"

using namespace pk;

namespace pkt {

namespace {

struct TableColumns {
    const uint64_t* col[PKT_MAX_WIDTH];
};

// column j of the workgroup's group: a chain of wave-uniform selects over the kernel's arguments
template <int W>
__device__ __forceinline__ void group_columns(const Columns& cols, unsigned g, const fe* (&out)[W]) {
#pragma unroll
    for (int j = 0; j < W; j++) {
        const uint64_t* p = cols.col[0][j];
#pragma unroll
        for (int other = 1; other < PKT_MAX_GROUPS; other++)
            if (g == (unsigned)other) p = cols.col[other][j];
        out[j] = (const fe*)p;
    }
}

template <int W>
__global__ __launch_bounds__(THREADS) void tuple_leaf_kernel(Columns cols, size_t rows, fe alpha, fe beta, fe* __restrict__ leaf) {
    constexpr int I = (int)LEAF_ITEMS;
    const unsigned g = blockIdx.y;
    const fe* col[W];
    group_columns<W>(cols, g, col);
    fe* const out = leaf + (size_t)g * rows;
    const size_t tile = (size_t)THREADS * I, tiles = (rows + tile - 1) / tile;
    for (size_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const size_t x0 = tl * tile + threadIdx.x;
        fe v[I][W];
#pragma unroll
        for (int i = 0; i < I; i++) {
            const size_t x = x0 + (size_t)i * THREADS;
#pragma unroll
            for (int j = 0; j < W; j++) v[i][j] = x < rows ? fe_load(col[j] + x) : fe_zero();
        }
#pragma unroll
        for (int i = 0; i < I; i++) {
            const size_t x = x0 + (size_t)i * THREADS;
            fe acc = v[i][W - 1];
#pragma unroll
            for (int j = W - 2; j >= 0; j--) acc = fe_add(fe_mulx(acc, beta), v[i][j]);
            if (x < rows) fe_store(out + x, fe_sub(alpha, acc));
        }
    }
}

template <int W, bool LDS>
__global__ __launch_bounds__(THREADS) void tuple_count_kernel(Columns f, TableColumns t, unsigned n, unsigned k, u32* __restrict__ counts,
                                                              unsigned long long* __restrict__ bad) {
    __shared__ u32 bins[LDS ? (1u << COUNT_LDS_MAX_K) : 1];
    const u32 size = 1u << k;
    if (LDS) {
        for (u32 b = threadIdx.x; b < size; b += THREADS) bins[b] = 0;
        __syncthreads();
    }
    const unsigned g = blockIdx.y;
    const fe* col[W];
    group_columns<W>(f, g, col);
    const u32* idx = f.idx[0];
#pragma unroll
    for (int other = 1; other < PKT_MAX_GROUPS; other++)
        if (g == (unsigned)other) idx = f.idx[other];
    const size_t total = (size_t)1 << n, stride = (size_t)gridDim.x * THREADS, stacked = (size_t)g << n;
    const unsigned lane = threadIdx.x & 63;
    u32 pending_bin = 0, pending = 0;  // wave-uniform: rows of one-bin iterations not yet added
    auto flush = [&]() {               // under wave-uniform control
        if (pending && lane == 0) {
            if (LDS)
                atomicAdd(&bins[pending_bin], pending);
            else
                atomicAdd(counts + pending_bin, pending);
        }
        pending = 0;
    };
    for (size_t base = (size_t)blockIdx.x * THREADS; base < total; base += stride) {  // workgroup-uniform trip count
        const size_t x = base + threadIdx.x;
        bool ok = false;
        u32 i = 0;
        if (x < total) {
            i = idx[x];
            if (i < size) {  // followed only now
                ok = true;
#pragma unroll
                for (int j = 0; j < W; j++) ok = ok & fe_eq(fe_load(col[j] + x), fe_load((const fe*)t.col[j] + i));
            }
            if (!ok) atomicMin(bad, (unsigned long long)(stacked + x));
        }
        const unsigned long long voters = __ballot(ok);
        if (voters == 0) continue;  // wave-uniform
        const unsigned leader = (unsigned)__ffsll((long long)voters) - 1;
        const u32 first = __shfl(i, leader, 64);
        const bool one_bin = __ballot(ok && i == first) == voters;  // wave-uniform
        if (one_bin) {
            if (pending && pending_bin != first) flush();
            pending_bin = first;
            pending += (u32)__popcll(voters);
        } else if (ok) {
            if (LDS)
                atomicAdd(&bins[i], 1u);
            else
                atomicAdd(counts + i, 1u);
        }
    }
    flush();
    if (LDS) {
        __syncthreads();
        for (u32 b = threadIdx.x; b < size; b += THREADS) {
            const u32 c = bins[b];
            if (c) atomicAdd(counts + b, c);
        }
    }
}

__global__ __launch_bounds__(THREADS) void mont_kernel(const u32* __restrict__ counts, size_t size, fe* __restrict__ m_out) {
    for (size_t y = (size_t)blockIdx.x * THREADS + threadIdx.x; y < size; y += (size_t)gridDim.x * THREADS) {
        fe c = fe_zero();
        c.v[0] = counts[y];
        fe_store(m_out + y, fe_mulx(c, fe_r2()));
    }
}

int launched() { return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP; }
bool shape_ok(unsigned n, unsigned w, unsigned c, unsigned grid) {
    return n >= 1 && n <= PKT_MAX_VARS && w >= 1 && w <= PKT_MAX_WIDTH && groups_ok(c) && grid <= PKT_MAX_GRID;
}

template <int W>
void count_step(hipStream_t stream, dim3 grid, bool lds, const Columns& f, const TableColumns& t, unsigned n, unsigned k, u32* counts, unsigned long long* bad) {
    if (lds)
        tuple_count_kernel<W, true><<<grid, THREADS, 0, stream>>>(f, t, n, k, counts, bad);
    else
        tuple_count_kernel<W, false><<<grid, THREADS, 0, stream>>>(f, t, n, k, counts, bad);
}

}  // namespace

int leaf_launch(hipStream_t stream, unsigned n, unsigned w, unsigned c, const Columns& cols, const uint64_t alpha[4], const uint64_t beta[4], uint64_t* d_leaf,
                unsigned grid_or_0) {
    if (!shape_ok(n, w, c, grid_or_0) || !alpha || !beta || !d_leaf) return PK_ERR_BAD_ARG;
    for (unsigned g = 0; g < c; g++)
        for (unsigned j = 0; j < w; j++)
            if (!cols.col[g][j]) return PK_ERR_BAD_ARG;
    const size_t rows = (size_t)1 << n;
    const dim3 grid(grid_or_0 ? grid_or_0 : rows_grid(rows, LEAF_ITEMS), c);
    fe a, b;
    memcpy(a.v, alpha, 32), memcpy(b.v, beta, 32);
    if (w == 1)
        tuple_leaf_kernel<1><<<grid, THREADS, 0, stream>>>(cols, rows, a, b, (fe*)d_leaf);
    else if (w == 2)
        tuple_leaf_kernel<2><<<grid, THREADS, 0, stream>>>(cols, rows, a, b, (fe*)d_leaf);
    else if (w == 3)
        tuple_leaf_kernel<3><<<grid, THREADS, 0, stream>>>(cols, rows, a, b, (fe*)d_leaf);
    else
        tuple_leaf_kernel<4><<<grid, THREADS, 0, stream>>>(cols, rows, a, b, (fe*)d_leaf);
    return launched();
}

int count_launch(hipStream_t stream, unsigned n, unsigned k, unsigned w, unsigned c, const Columns& f, const uint64_t* const d_t[PKT_MAX_WIDTH],
                 uint32_t* d_counts, unsigned long long* d_bad, uint64_t* d_m_out, unsigned grid_or_0) {
    if (!shape_ok(n, w, c, grid_or_0) || k < 1 || k > PKT_MAX_VARS || !d_t || !d_counts || !d_bad || !d_m_out) return PK_ERR_BAD_ARG;
    TableColumns t{};
    for (unsigned j = 0; j < w; j++) {
        if (!d_t[j]) return PK_ERR_BAD_ARG;
        t.col[j] = d_t[j];
    }
    for (unsigned g = 0; g < c; g++) {
        if (!f.idx[g]) return PK_ERR_BAD_ARG;
        for (unsigned j = 0; j < w; j++)
            if (!f.col[g][j]) return PK_ERR_BAD_ARG;
    }
    const size_t total = (size_t)1 << n, size = (size_t)1 << k;
    if (hipMemsetAsync(d_counts, 0, 4 * size, stream) != hipSuccess || hipMemsetAsync(d_bad, 0xff, 8, stream) != hipSuccess) return PK_ERR_HIP;
    const dim3 grid(grid_or_0 ? grid_or_0 : rows_grid(total, COUNT_ITEMS), c);
    const bool lds = k <= COUNT_LDS_MAX_K;
    if (w == 1)
        count_step<1>(stream, grid, lds, f, t, n, k, d_counts, d_bad);
    else if (w == 2)
        count_step<2>(stream, grid, lds, f, t, n, k, d_counts, d_bad);
    else if (w == 3)
        count_step<3>(stream, grid, lds, f, t, n, k, d_counts, d_bad);
    else
        count_step<4>(stream, grid, lds, f, t, n, k, d_counts, d_bad);
    mont_kernel<<<grid_or_0 ? grid_or_0 : rows_grid(size, COUNT_ITEMS), THREADS, 0, stream>>>(d_counts, size, (fe*)d_m_out);
    return launched();
}

}  // namespace pkt
