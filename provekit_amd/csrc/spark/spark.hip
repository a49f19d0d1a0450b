// spark.hip -- the HIP kernels libprovekit_spark.so adds (gfx950): the per-query gather from the two eq tables, and the preprocessing of
// a sparse matrix's entry list into its committed columns.
//
// spark_gather_kernel (the per-query hot pass): e_row[k] = eq_row[row_idx[k]], e_col[k] = eq_col[col_idx[k]].  A lane takes
//   GATHER_ITEMS entries a workgroup-width apart: the u32 indices are loaded coalesced and validated BEFORE they are followed
//   (row_idx[k] < 2^s, col_idx[k] < 2^t; a failure lowers the 64-bit cell `bad` with atomicMin to k, so the cell ends as the smallest
//   failing entry, and the entry goes on as index 0), then all 2 * GATHER_ITEMS 32-byte gathers are issued before the first store, and
//   the stores are coalesced.  Its own bytes per entry: 8 of indices, 64 gathered, 64 stored.
// spark_count_kernel<LDS>: the histogram of one index array, indices only (no row is compared: the lookup's proof does that).  Every
//   index is validated the same way and a bad one is not counted.  Up to 2^COUNT_LDS_MAX bins in a workgroup-private LDS histogram
//   flushed once per non-zero bin, larger ones with atomics on device memory.  As in tuplelookup/tuple.hip a wavefront whose valid lanes
//   all name one bin keeps (bin, count) in wave-uniform registers and adds when the bin changes and at its end: one atomic per
//   wavefront under full skew -- an R1CS's column 0, the constant-one witness, and the padding's (0, 0).  Integer adds: the counts are
//   exact in any order.  spark_mont_kernel writes m as elements.
// spark_columns_kernel: an index as a Montgomery element, one product; it follows no index.
// iota_kernel: the index column 0 .. 2^v - 1, once per prover.
//
// All loads and stores are ordinary vector accesses; the atomics are vector atomics on device memory or LDS.
#include <hip/hip_runtime.h>

#include "../fe29.hpp"
#include "kernels.hpp"

using namespace pk;

namespace pkx {

namespace {

typedef unsigned long long u64;

// a small integer as a Montgomery element: one product
__device__ __forceinline__ fe small_mont(u32 c) {
    fe x = fe_zero();
    x.v[0] = c;
    return fe_mulx(x, fe_r2());
}

__global__ __launch_bounds__(THREADS) void iota_kernel(size_t rows, fe* __restrict__ out) {
    for (size_t x = (size_t)blockIdx.x * THREADS + threadIdx.x; x < rows; x += (size_t)gridDim.x * THREADS) fe_store(out + x, small_mont((u32)x));
}

__global__ __launch_bounds__(THREADS) void spark_gather_kernel(const u32* __restrict__ row_idx, const u32* __restrict__ col_idx, const fe* __restrict__ eq_row,
                                                               const fe* __restrict__ eq_col, size_t rows, unsigned s, unsigned t, fe* __restrict__ e_row,
                                                               fe* __restrict__ e_col, u64* __restrict__ bad) {
    constexpr int I = (int)GATHER_ITEMS;
    const size_t tile = (size_t)THREADS * I, tiles = (rows + tile - 1) / tile;
    for (size_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const size_t x0 = tl * tile + threadIdx.x;
        u32 r[I], c[I];
#pragma unroll
        for (int i = 0; i < I; i++) {
            const size_t x = x0 + (size_t)i * THREADS;
            r[i] = x < rows ? row_idx[x] : 0;
            c[i] = x < rows ? col_idx[x] : 0;
        }
#pragma unroll
        for (int i = 0; i < I; i++) {  // s, t <= 28: an index with a bit at or above them is outside its table.  Reported, and followed as 0
            if ((r[i] >> s) | (c[i] >> t)) {
                atomicMin(bad, (u64)(x0 + (size_t)i * THREADS));
                r[i] = c[i] = 0;
            }
        }
        fe vr[I], vc[I];
#pragma unroll
        for (int i = 0; i < I; i++) {
            vr[i] = fe_load(eq_row + r[i]);
            vc[i] = fe_load(eq_col + c[i]);
        }
#pragma unroll
        for (int i = 0; i < I; i++) {
            const size_t x = x0 + (size_t)i * THREADS;
            if (x < rows) {
                fe_store(e_row + x, vr[i]);
                fe_store(e_col + x, vc[i]);
            }
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(THREADS) void spark_count_kernel(const u32* __restrict__ idx, unsigned n, unsigned bits, u32* __restrict__ counts, u64* __restrict__ bad) {
    __shared__ u32 bins[LDS ? (1u << COUNT_LDS_MAX) : 1];
    const u32 size = 1u << bits;
    if (LDS) {
        for (u32 b = threadIdx.x; b < size; b += THREADS) bins[b] = 0;
        __syncthreads();
    }
    const size_t total = (size_t)1 << n, stride = (size_t)gridDim.x * THREADS;
    const unsigned lane = threadIdx.x & 63;
    u32 pending_bin = 0, pending = 0;  // wave-uniform: entries of one-bin iterations not yet added
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
        u32 v = 0;
        if (x < total) {
            v = idx[x];
            ok = v < size;  // a bin is never taken on trust
            if (!ok) atomicMin(bad, (u64)x);
        }
        const u64 voters = __ballot(ok);
        if (voters == 0) continue;  // wave-uniform
        const unsigned leader = (unsigned)__ffsll((long long)voters) - 1;
        const u32 first = __shfl(v, leader, 64);
        const bool one_bin = __ballot(ok && v == first) == voters;  // wave-uniform
        if (one_bin) {
            if (pending && pending_bin != first) flush();
            pending_bin = first;
            pending += (u32)__popcll(voters);
        } else if (ok) {
            if (LDS)
                atomicAdd(&bins[v], 1u);
            else
                atomicAdd(counts + v, 1u);
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

__global__ __launch_bounds__(THREADS) void spark_mont_kernel(const u32* __restrict__ counts, size_t size, fe* __restrict__ m_out) {
    for (size_t y = (size_t)blockIdx.x * THREADS + threadIdx.x; y < size; y += (size_t)gridDim.x * THREADS) fe_store(m_out + y, small_mont(counts[y]));
}

__global__ __launch_bounds__(THREADS) void spark_columns_kernel(const u32* __restrict__ row_idx, const u32* __restrict__ col_idx, size_t rows, fe* __restrict__ row_out,
                                                                fe* __restrict__ col_out) {
    for (size_t x = (size_t)blockIdx.x * THREADS + threadIdx.x; x < rows; x += (size_t)gridDim.x * THREADS) {
        const u32 r = row_idx[x], c = col_idx[x];
        fe_store(row_out + x, small_mont(r));
        fe_store(col_out + x, small_mont(c));
    }
}

int launched() { return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP; }
bool vars_ok(unsigned v) { return v >= 1 && v <= PKX_MAX_VARS; }
bool shape_ok(unsigned n, unsigned s, unsigned t, unsigned grid) { return vars_ok(n) && vars_ok(s) && vars_ok(t) && grid <= PKX_MAX_GRID; }
unsigned grid_for(unsigned grid_or_0, size_t rows, unsigned per_lane) { return grid_or_0 ? grid_or_0 : rows_grid(rows, per_lane); }

void count_step(hipStream_t stream, unsigned grid, const u32* idx, unsigned n, unsigned bits, u32* counts, u64* bad) {
    if (bits <= COUNT_LDS_MAX)
        spark_count_kernel<true><<<grid, THREADS, 0, stream>>>(idx, n, bits, counts, bad);
    else
        spark_count_kernel<false><<<grid, THREADS, 0, stream>>>(idx, n, bits, counts, bad);
}

}  // namespace

int iota_launch(hipStream_t stream, unsigned v, uint64_t* d_out, unsigned grid_or_0) {
    if (!vars_ok(v) || grid_or_0 > PKX_MAX_GRID || !d_out) return PK_ERR_BAD_ARG;
    const size_t rows = (size_t)1 << v;
    iota_kernel<<<grid_for(grid_or_0, rows, MATRIX_ITEMS), THREADS, 0, stream>>>(rows, (fe*)d_out);
    return launched();
}

int count_launch(hipStream_t stream, unsigned n, unsigned s, unsigned t, const uint32_t* d_row_idx, const uint32_t* d_col_idx, uint32_t* d_counts_row,
                 uint32_t* d_counts_col, unsigned long long* d_bad, unsigned grid_or_0) {
    if (!shape_ok(n, s, t, grid_or_0) || !d_row_idx || !d_col_idx || !d_counts_row || !d_counts_col || !d_bad) return PK_ERR_BAD_ARG;
    if (hipMemsetAsync(d_counts_row, 0, (size_t)4 << s, stream) != hipSuccess || hipMemsetAsync(d_counts_col, 0, (size_t)4 << t, stream) != hipSuccess ||
        hipMemsetAsync(d_bad, 0xff, 8, stream) != hipSuccess)
        return PK_ERR_HIP;
    const unsigned grid = grid_for(grid_or_0, (size_t)1 << n, MATRIX_ITEMS);
    count_step(stream, grid, d_row_idx, n, s, d_counts_row, d_bad);
    count_step(stream, grid, d_col_idx, n, t, d_counts_col, d_bad);
    return launched();
}

int columns_launch(hipStream_t stream, unsigned n, unsigned s, unsigned t, const uint32_t* d_row_idx, const uint32_t* d_col_idx, const uint32_t* d_counts_row,
                   const uint32_t* d_counts_col, uint64_t* d_row_out, uint64_t* d_col_out, uint64_t* d_m_row_out, uint64_t* d_m_col_out, unsigned grid_or_0) {
    if (!shape_ok(n, s, t, grid_or_0) || !d_row_idx || !d_col_idx || !d_counts_row || !d_counts_col || !d_row_out || !d_col_out || !d_m_row_out || !d_m_col_out)
        return PK_ERR_BAD_ARG;
    const size_t rows = (size_t)1 << n;
    spark_columns_kernel<<<grid_for(grid_or_0, rows, MATRIX_ITEMS), THREADS, 0, stream>>>(d_row_idx, d_col_idx, rows, (fe*)d_row_out, (fe*)d_col_out);
    spark_mont_kernel<<<grid_for(grid_or_0, (size_t)1 << s, MATRIX_ITEMS), THREADS, 0, stream>>>(d_counts_row, (size_t)1 << s, (fe*)d_m_row_out);
    spark_mont_kernel<<<grid_for(grid_or_0, (size_t)1 << t, MATRIX_ITEMS), THREADS, 0, stream>>>(d_counts_col, (size_t)1 << t, (fe*)d_m_col_out);
    return launched();
}

int gather_launch(hipStream_t stream, unsigned n, unsigned s, unsigned t, const uint32_t* d_row_idx, const uint32_t* d_col_idx, const uint64_t* d_eq_row,
                  const uint64_t* d_eq_col, uint64_t* d_e_row_out, uint64_t* d_e_col_out, unsigned long long* d_bad, unsigned grid_or_0) {
    if (!shape_ok(n, s, t, grid_or_0) || !d_row_idx || !d_col_idx || !d_eq_row || !d_eq_col || !d_e_row_out || !d_e_col_out || !d_bad) return PK_ERR_BAD_ARG;
    if (hipMemsetAsync(d_bad, 0xff, 8, stream) != hipSuccess) return PK_ERR_HIP;
    const size_t rows = (size_t)1 << n;
    spark_gather_kernel<<<grid_for(grid_or_0, rows, GATHER_ITEMS), THREADS, 0, stream>>>(d_row_idx, d_col_idx, (const fe*)d_eq_row, (const fe*)d_eq_col, rows, s, t,
                                                                                         (fe*)d_e_row_out, (fe*)d_e_col_out, d_bad);
    return launched();
}

}  // namespace pkx
