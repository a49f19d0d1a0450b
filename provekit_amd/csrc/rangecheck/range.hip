// range.hip -- the HIP kernels libprovekit_rangecheck.so adds (gfx950): the fused decomposition of a column into its limb columns and
// their multiplicities, the scaled top limb of a proof, and the index table.
//
// range_decompose_kernel<LDS> (the hot pass): per entry one coalesced 32-byte load, out of Montgomery form by one product, ALL words
//   of the canonical value checked against 2^bits (words 2 .. 7 zero, and the low 64 bits below 2^bits: a value with only a high word
//   set fails; a failure lowers the 64-bit cell `bad` with atomicMin to x, so the cell ends as the smallest failing entry), the L limbs
//   taken with shifts of the low 64 bits, each back to Montgomery form by one product with R^2 and stored coalesced to its column, and
//   the bins of all c groups of the plan (statement.hpp) counted: the limbs, the top limb shifted by k - r, the spare group's repeat of
//   limb 0.  No gather and no index list: the table is the identity, a limb is its own bin.  A failing entry is not counted.  A lane
//   takes DECOMPOSE_ITEMS entries a workgroup-width apart, their loads issued before the first product.
//   Bins follow tuplelookup/tuple.hip's rule: up to 2^COUNT_LDS_MAX_K of them in a workgroup-private LDS histogram flushed once per
//   non-zero bin, more with vector atomics on device memory.  The wavefront aggregation is kept PER GROUP: a pair of wave-uniform
//   (bin, pending) registers for each of the c groups, added when that group's bin changes and at the end.  64-bit columns that hold
//   small numbers put every high limb in bin 0: one atomic per wavefront and group instead of 64.  A wavefront with mixed bins in a
//   group adds lane by lane in that group.  Integer adds: the counts are exact in any order, no bit depends on the grid.
// mont_kernel writes m as Montgomery elements (tuple.hip's rule, written out again: that file's kernels stay as they are).
// range_scale_kernel: scaled[x] = 2^(k-r) limb[x], one product per element.
// index_kernel: the table 0 .. 2^k - 1, once per prover.
//
// All loads and stores are ordinary vector accesses; the atomics are vector atomics on device memory or LDS.
#include <hip/hip_runtime.h>

#include "../fe29.hpp"
#include "kernels.hpp"

using namespace pk;

namespace pkr {

namespace {

typedef unsigned long long u64a;  // atomicMin's 64-bit type

struct LimbColumns {
    uint64_t* col[PKR_MAX_GROUPS];
};

// a small integer as a Montgomery element: one product
__device__ __forceinline__ fe small_mont(u32 c) {
    fe x = fe_zero();
    x.v[0] = c;
    return fe_mulx(x, fe_r2());
}

__global__ __launch_bounds__(THREADS) void index_kernel(size_t rows, fe* __restrict__ out) {
    for (size_t y = (size_t)blockIdx.x * THREADS + threadIdx.x; y < rows; y += (size_t)gridDim.x * THREADS) fe_store(out + y, small_mont((u32)y));
}

__global__ __launch_bounds__(THREADS) void range_scale_kernel(const fe* __restrict__ limb, size_t rows, fe factor, fe* __restrict__ out) {
    for (size_t x = (size_t)blockIdx.x * THREADS + threadIdx.x; x < rows; x += (size_t)gridDim.x * THREADS) fe_store(out + x, fe_mulx(fe_load(limb + x), factor));
}

__global__ __launch_bounds__(THREADS) void mont_kernel(const u32* __restrict__ counts, size_t size, fe* __restrict__ m_out) {
    for (size_t y = (size_t)blockIdx.x * THREADS + threadIdx.x; y < size; y += (size_t)gridDim.x * THREADS) fe_store(m_out + y, small_mont(counts[y]));
}

template <bool LDS>
__global__ __launch_bounds__(THREADS) void range_decompose_kernel(const fe* __restrict__ f, size_t total, unsigned bits, unsigned k, LimbColumns out,
                                                                  u32* __restrict__ counts, u64a* __restrict__ bad) {
    constexpr int I = (int)DECOMPOSE_ITEMS, GROUPS = PKR_MAX_GROUPS;
    __shared__ u32 bins[LDS ? (1u << COUNT_LDS_MAX_K) : 1];
    const Plan P = plan_of(bits, k);  // wave-uniform
    const u32 size = 1u << k, mask = size - 1;
    if (LDS) {
        for (u32 b = threadIdx.x; b < size; b += THREADS) bins[b] = 0;
        __syncthreads();
    }
    const unsigned lane = threadIdx.x & 63;
    u32 pending_bin[GROUPS] = {0, 0, 0, 0}, pending[GROUPS] = {0, 0, 0, 0};  // wave-uniform, per group: entries of one-bin steps not yet added
    auto flush = [&](int g) {                                                // under wave-uniform control
        if (pending[g] && lane == 0) {
            if (LDS)
                atomicAdd(&bins[pending_bin[g]], pending[g]);
            else
                atomicAdd(counts + pending_bin[g], pending[g]);
        }
        pending[g] = 0;
    };
    const size_t tile = (size_t)THREADS * I, tiles = (total + tile - 1) / tile;
    for (size_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {  // workgroup-uniform trip count
        const size_t x0 = tl * tile + threadIdx.x;
        fe v[I];
#pragma unroll
        for (int i = 0; i < I; i++) {
            const size_t x = x0 + (size_t)i * THREADS;
            v[i] = x < total ? fe_load(f + x) : fe_zero();
        }
#pragma unroll
        for (int i = 0; i < I; i++) {
            const size_t x = x0 + (size_t)i * THREADS;
            const bool inside = x < total;
            const fe c = fe_from_montx(v[i]);
            const uint64_t lo = (uint64_t)c.v[0] | (uint64_t)c.v[1] << 32;
            const u32 high = c.v[2] | c.v[3] | c.v[4] | c.v[5] | c.v[6] | c.v[7];
            const bool fits = high == 0 && (bits == 64 || (lo >> bits) == 0);
            const bool ok = inside && fits;
            if (inside && !fits) atomicMin(bad, (u64a)x);
#pragma unroll
            for (int j = 0; j < GROUPS; j++)  // the limbs, each back to Montgomery form; of a failing entry the low 64 bits' (not meaningful)
                if ((unsigned)j < P.L && inside) fe_store((fe*)out.col[j] + x, small_mont((u32)(lo >> (k * j)) & mask));
            const u64a voters = __ballot(ok);
            if (voters == 0) continue;  // wave-uniform
            const unsigned leader = (unsigned)__ffsll((long long)voters) - 1;
#pragma unroll
            for (int g = 0; g < GROUPS; g++) {
                if ((unsigned)g >= P.c) continue;  // wave-uniform
                // group g's bin by the plan: a limb below 2^k; the top limb of an entry that fits is below 2^r, so its shift is below 2^k
                const u32 b = ((u32)(lo >> (k * P.limb_of[g])) & mask) << P.shift_of[g];
                const u32 first = __shfl(b, leader, 64);
                const bool one_bin = __ballot(ok && b == first) == voters;  // wave-uniform
                if (one_bin) {
                    if (pending[g] && pending_bin[g] != first) flush(g);
                    pending_bin[g] = first;
                    pending[g] += (u32)__popcll(voters);
                } else if (ok) {
                    if (LDS)
                        atomicAdd(&bins[b], 1u);
                    else
                        atomicAdd(counts + b, 1u);
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < GROUPS; g++) flush(g);
    if (LDS) {
        __syncthreads();
        for (u32 b = threadIdx.x; b < size; b += THREADS) {
            const u32 c = bins[b];
            if (c) atomicAdd(counts + b, c);
        }
    }
}

int launched() { return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP; }
bool vars_ok(unsigned v) { return v >= 1 && v <= PKR_MAX_VARS; }
unsigned grid_for(unsigned grid_or_0, size_t rows, unsigned per_lane) { return grid_or_0 ? grid_or_0 : rows_grid(rows, per_lane); }

}  // namespace

int index_launch(hipStream_t stream, unsigned k, uint64_t* d_out, unsigned grid_or_0) {
    if (!vars_ok(k) || grid_or_0 > PKR_MAX_GRID || !d_out) return PK_ERR_BAD_ARG;
    const size_t rows = (size_t)1 << k;
    index_kernel<<<grid_for(grid_or_0, rows, PLAIN_ITEMS), THREADS, 0, stream>>>(rows, (fe*)d_out);
    return launched();
}

int decompose_launch(hipStream_t stream, unsigned n, unsigned bits, unsigned k, const uint64_t* d_f, uint64_t* const d_limbs[PKR_MAX_GROUPS], uint32_t* d_counts,
                     unsigned long long* d_bad, uint64_t* d_m_out, unsigned grid_or_0) {
    if (!vars_ok(n) || bits < 1 || bits > PKR_MAX_BITS || k < 1 || k > PKR_MAX_LIMB_BITS || grid_or_0 > PKR_MAX_GRID) return PK_ERR_BAD_ARG;
    if (!d_f || !d_limbs || !d_counts || !d_bad || !d_m_out) return PK_ERR_BAD_ARG;
    const Plan P = plan_of(bits, k);
    if (!P.c) return PK_ERR_BAD_ARG;
    LimbColumns out{};
    for (unsigned i = 0; i < P.L; i++)
        if (!(out.col[i] = d_limbs[i])) return PK_ERR_BAD_ARG;
    const size_t total = (size_t)1 << n, size = (size_t)1 << k;
    if (hipMemsetAsync(d_counts, 0, 4 * size, stream) != hipSuccess || hipMemsetAsync(d_bad, 0xff, 8, stream) != hipSuccess) return PK_ERR_HIP;
    const unsigned grid = grid_for(grid_or_0, total, DECOMPOSE_ITEMS);
    if (k <= COUNT_LDS_MAX_K)
        range_decompose_kernel<true><<<grid, THREADS, 0, stream>>>((const fe*)d_f, total, bits, k, out, d_counts, d_bad);
    else
        range_decompose_kernel<false><<<grid, THREADS, 0, stream>>>((const fe*)d_f, total, bits, k, out, d_counts, d_bad);
    mont_kernel<<<grid_for(grid_or_0, size, PLAIN_ITEMS), THREADS, 0, stream>>>(d_counts, size, (fe*)d_m_out);
    return launched();
}

int scale_launch(hipStream_t stream, unsigned n, unsigned shift, const uint64_t* d_limb, uint64_t* d_out, unsigned grid_or_0) {
    if (!vars_ok(n) || shift >= PKR_MAX_LIMB_BITS || grid_or_0 > PKR_MAX_GRID || !d_limb || !d_out) return PK_ERR_BAD_ARG;
    const size_t rows = (size_t)1 << n;
    range_scale_kernel<<<grid_for(grid_or_0, rows, PLAIN_ITEMS), THREADS, 0, stream>>>((const fe*)d_limb, rows, pow2(shift), (fe*)d_out);
    return launched();
}

}  // namespace pkr
