// lookup.hip -- the HIP kernels libprovekit_lookup.so adds (gfx950): the multiplicities of a table under a column of lookups, the
// table side's helper columns with their sum, and the column side's gather.
//
// count_kernel: one pass over idx, f and the gathered t[idx].  A lane validates its lookup (idx[x] < 2^k, f[x] == t[idx[x]] on the
// stored words); a failure lowers the 64-bit cell `bad` with atomicMin, so the cell ends as the smallest failing x.  Valid lookups
// are counted: tables of k <= COUNT_LDS_MAX_K in a workgroup-private LDS histogram that is flushed once per non-zero bin, larger ones
// with atomics on device memory.  Full skew (every lookup one bin) would serialise either kind of atomic, so a wavefront whose valid
// lanes all name one bin does not add at once: it keeps (bin, count) in wave-uniform registers across its iterations and adds when the
// bin changes and at its end -- one atomic per wavefront under full skew (EXPERIMENTS round 24 has the phase under both
// distributions).  A wavefront with mixed bins adds lane by lane.  The counts are exact whatever the order: integer adds.
// mont_kernel then writes m as Montgomery elements.
//
// table_kernel: one pass over y.  A lane takes TABLE_BATCH = E elements a workgroup-width apart (loads and stores coalesced), forms
// d = alpha - t, inverts the E of them with Montgomery's trick -- E - 1 prefix products, ONE feinv.hpp inverse, 2 (E - 1) products on
// the way back -- and writes d_t, g = 1/d and h_t = count * g (0 for a count of 0).  A zero denominator raises flags[0] and stands in
// the batch as 1, so the lane's other E - 1 inverses stay what they are; the host fails the call on the flag.  s = sum h_t goes
// through reduce.hpp's block_reduce_fe to one partial per workgroup and finish_kernel adds the partials: field addition is exact, so
// s does not depend on the grid.
//
// gather_kernel: one pass over x: h_f[x] = g[idx[x]], d_f[x] = d_t[idx[x]].  ITEMS_PER_LANE lookups per lane, all indices loaded
// before the first dependent read, so a lane has 2 * ITEMS_PER_LANE random 32-byte reads in flight; stores are coalesced.  The
// sources are read through L2.  gather_staged_kernel is the same pass for k <= GATHER_LDS_MAX_K: every workgroup first copies both
// source tables (2 * 2^k * 32 bytes) into LDS and gathers from there; few workgroups (two per CU, one at the 128 KiB of k = 11), each
// striding over many tiles.  Measured against gather_kernel on the same box, alternating, it won at every k it takes (EXPERIMENTS
// round 24), so it ships.  An index >= 2^k is not followed and raises flags[1] (idx changed after pkl_multiplicities validated it).
//
// All stores are ordinary vector stores; the atomics are vector atomics on device memory or LDS.
#include <hip/hip_runtime.h>

#include "../reduce.hpp"
#include "../feinv.hpp"
#include "kernels.hpp"

using namespace pk;

namespace pkl {

namespace {

__device__ __forceinline__ fe mont_from_u32(u32 c) {
    fe x = fe_zero();
    x.v[0] = c;
    return fe_mulx(x, fe_r2());
}

template <bool LDS>
__global__ __launch_bounds__(THREADS) void count_kernel(const fe* __restrict__ f, const fe* __restrict__ t, const u32* __restrict__ idx, unsigned n, unsigned k,
                                                        u32* __restrict__ counts, unsigned long long* __restrict__ bad) {
    __shared__ u32 bins[LDS ? (1u << COUNT_LDS_MAX_K) : 1];
    const u32 size = 1u << k;
    if (LDS) {
        for (u32 b = threadIdx.x; b < size; b += THREADS) bins[b] = 0;
        __syncthreads();
    }
    const size_t total = (size_t)1 << n, stride = (size_t)gridDim.x * THREADS;
    const unsigned lane = threadIdx.x & 63;
    u32 pending_bin = 0, pending = 0;  // wave-uniform: lookups of one-bin iterations not yet added
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
            if (i < size) ok = fe_eq(fe_load(f + x), fe_load(t + i));
            if (!ok) atomicMin(bad, (unsigned long long)x);
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
    for (size_t y = (size_t)blockIdx.x * THREADS + threadIdx.x; y < size; y += (size_t)gridDim.x * THREADS) fe_store(m_out + y, mont_from_u32(counts[y]));
}

__global__ __launch_bounds__(THREADS) void table_kernel(const fe* __restrict__ t, const u32* __restrict__ counts, fe alpha, size_t size, fe* __restrict__ dt,
                                                        fe* __restrict__ g, fe* __restrict__ ht, fe* __restrict__ partial, u32* __restrict__ flags) {
    constexpr int E = (int)TABLE_BATCH;
    const size_t tile = (size_t)THREADS * E, tiles = (size + tile - 1) / tile;
    fe acc[1] = {fe_zero()};
    bool hit = false;
    for (size_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const size_t y0 = tl * tile + threadIdx.x;
        fe d[E], pre[E];  // pre[e] = d[0] .. d[e]
#pragma unroll
        for (int e = 0; e < E; e++) {
            const size_t y = y0 + (size_t)e * THREADS;
            d[e] = fe_one();
            if (y < size) {
                const fe diff = fe_sub(alpha, fe_load(t + y));
                fe_store(dt + y, diff);
                if (fe_eq(diff, fe_zero()))
                    hit = true;  // stands in the batch as 1
                else
                    d[e] = diff;
            }
            pre[e] = e ? fe_mulx(pre[e - 1], d[e]) : d[e];
        }
        fe inv = fe_inverse_mont(pre[E - 1]);  // 1 / (d[0] .. d[E-1])
#pragma unroll
        for (int e = E - 1; e >= 0; e--) {
            const fe ge = e ? fe_mulx(inv, pre[e - 1]) : inv;
            if (e) inv = fe_mulx(inv, d[e]);
            const size_t y = y0 + (size_t)e * THREADS;
            if (y < size) {
                fe_store(g + y, ge);
                const u32 c = counts[y];
                const fe h = c ? fe_mulx(ge, mont_from_u32(c)) : fe_zero();
                fe_store(ht + y, h);
                acc[0] = fe_add(acc[0], h);
            }
        }
    }
    if (hit) atomicOr(flags, 1u);
    const fe mine = block_reduce_fe<1>(acc);
    if (threadIdx.x == 0) fe_store(partial + blockIdx.x, mine);
}

// out[0] = the sum of partial[0 .. n_wg); one workgroup
__global__ __launch_bounds__(THREADS) void finish_kernel(const fe* __restrict__ partial, unsigned n_wg, fe* __restrict__ out) {
    fe acc = fe_zero();
    for (unsigned j = threadIdx.x; j < n_wg; j += THREADS) acc = fe_add(acc, fe_load(partial + j));
    acc = block_sum(acc);
    if (threadIdx.x == 0) fe_store(out, acc);
}

__global__ __launch_bounds__(THREADS) void gather_kernel(const u32* __restrict__ idx, const fe* __restrict__ g, const fe* __restrict__ dt, size_t total, u32 size,
                                                         fe* __restrict__ hf, fe* __restrict__ df, u32* __restrict__ flags) {
    constexpr int I = (int)ITEMS_PER_LANE;
    const size_t tile = (size_t)THREADS * I, tiles = (total + tile - 1) / tile;
    bool stray = false;
    for (size_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const size_t x0 = tl * tile + threadIdx.x;
        u32 at[I];
        bool live[I];
#pragma unroll
        for (int j = 0; j < I; j++) {
            const size_t x = x0 + (size_t)j * THREADS;
            live[j] = x < total;
            at[j] = live[j] ? idx[x] : 0;
            if (at[j] >= size) stray = true, live[j] = false;
        }
        fe a[I], b[I];
#pragma unroll
        for (int j = 0; j < I; j++)
            if (live[j]) a[j] = fe_load(g + at[j]), b[j] = fe_load(dt + at[j]);
#pragma unroll
        for (int j = 0; j < I; j++)
            if (live[j]) {
                const size_t x = x0 + (size_t)j * THREADS;
                fe_store(hf + x, a[j]);
                fe_store(df + x, b[j]);
            }
    }
    if (stray) atomicOr(flags + 1, 1u);
}

// stage[0 .. 2 size): g as 16-byte halves; stage[2 size .. 4 size): d_t
__global__ __launch_bounds__(THREADS) void gather_staged_kernel(const u32* __restrict__ idx, const uint4* __restrict__ g, const uint4* __restrict__ dt, size_t total,
                                                                u32 size, uint4* __restrict__ hf, uint4* __restrict__ df, u32* __restrict__ flags) {
    extern __shared__ uint4 stage[];
    constexpr int I = (int)ITEMS_PER_LANE;
    for (u32 i = threadIdx.x; i < 2 * size; i += THREADS) {
        stage[i] = g[i];
        stage[2 * size + i] = dt[i];
    }
    __syncthreads();
    const size_t tile = (size_t)THREADS * I, tiles = (total + tile - 1) / tile;
    bool stray = false;
    for (size_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const size_t x0 = tl * tile + threadIdx.x;
#pragma unroll
        for (int j = 0; j < I; j++) {
            const size_t x = x0 + (size_t)j * THREADS;
            if (x >= total) continue;
            const u32 at = idx[x];
            if (at >= size) {
                stray = true;
                continue;
            }
            hf[2 * x] = stage[2 * at];
            hf[2 * x + 1] = stage[2 * at + 1];
            df[2 * x] = stage[2 * size + 2 * at];
            df[2 * x + 1] = stage[2 * size + 2 * at + 1];
        }
    }
    if (stray) atomicOr(flags + 1, 1u);
}

bool grid_ok(unsigned grid) { return grid <= PKL_MAX_GRID; }
int launched() { return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP; }

}  // namespace

int count_launch(hipStream_t stream, unsigned n, unsigned k, const uint64_t* d_f, const uint64_t* d_t, const uint32_t* d_idx, uint32_t* d_counts,
                 unsigned long long* d_bad, uint64_t* d_m_out, unsigned grid_or_0) {
    if (n < 1 || n > PKL_MAX_VARS || k < 1 || k > PKL_MAX_VARS || !grid_ok(grid_or_0)) return PK_ERR_BAD_ARG;
    const size_t total = (size_t)1 << n, size = (size_t)1 << k;
    if (hipMemsetAsync(d_counts, 0, 4 * size, stream) != hipSuccess || hipMemsetAsync(d_bad, 0xff, 8, stream) != hipSuccess) return PK_ERR_HIP;
    const unsigned grid = grid_or_0 ? grid_or_0 : lookups_grid(total);
    if (k <= COUNT_LDS_MAX_K)
        count_kernel<true><<<grid, THREADS, 0, stream>>>((const fe*)d_f, (const fe*)d_t, d_idx, n, k, d_counts, d_bad);
    else
        count_kernel<false><<<grid, THREADS, 0, stream>>>((const fe*)d_f, (const fe*)d_t, d_idx, n, k, d_counts, d_bad);
    mont_kernel<<<grid_or_0 ? grid_or_0 : lookups_grid(size), THREADS, 0, stream>>>(d_counts, size, (fe*)d_m_out);
    return launched();
}

int table_launch(hipStream_t stream, unsigned k, const uint64_t* d_t, const uint32_t* d_counts, const uint64_t* alpha, uint64_t* d_dt, uint64_t* d_g,
                 uint64_t* d_ht, uint64_t* d_partials, uint64_t* d_sum, uint32_t* d_flags, unsigned grid_or_0) {
    if (k < 1 || k > PKL_MAX_VARS || !grid_ok(grid_or_0)) return PK_ERR_BAD_ARG;
    const size_t size = (size_t)1 << k;
    if (hipMemsetAsync(d_flags, 0, 4, stream) != hipSuccess) return PK_ERR_HIP;
    const unsigned grid = grid_or_0 ? grid_or_0 : table_grid(size);
    fe a;
    memcpy(a.v, alpha, 32);
    table_kernel<<<grid, THREADS, 0, stream>>>((const fe*)d_t, d_counts, a, size, (fe*)d_dt, (fe*)d_g, (fe*)d_ht, (fe*)d_partials, d_flags);
    finish_kernel<<<1, THREADS, 0, stream>>>((const fe*)d_partials, grid, (fe*)d_sum);
    return launched();
}

int gather_prepare(GatherPlan& plan) {
    int device = 0, cus = 0;
    if (hipGetDevice(&device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1)
        return PK_ERR_HIP;
    // up to 128 KiB: above the 64 KiB a kernel gets without asking
    if (hipFuncSetAttribute((const void*)gather_staged_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)64 << GATHER_LDS_MAX_K)) != hipSuccess)
        return PK_ERR_HIP;
    plan.cus = cus;
    return PK_OK;
}

int gather_launch(hipStream_t stream, const GatherPlan& plan, unsigned n, unsigned k, const uint32_t* d_idx, const uint64_t* d_g, const uint64_t* d_dt,
                  uint64_t* d_hf, uint64_t* d_df, uint32_t* d_flags, unsigned grid_or_0, int staging) {
    if (n < 1 || n > PKL_MAX_VARS || k < 1 || k > PKL_MAX_VARS || !grid_ok(grid_or_0)) return PK_ERR_BAD_ARG;
    if (staging > 0 && k > GATHER_LDS_MAX_K) return PK_ERR_BAD_ARG;
    const size_t total = (size_t)1 << n;
    const bool staged = staging < 0 ? k <= GATHER_LDS_MAX_K : staging > 0;
    if (staged && plan.cus < 1) return PK_ERR_BAD_ARG;
    if (hipMemsetAsync(d_flags + 1, 0, 4, stream) != hipSuccess) return PK_ERR_HIP;
    if (staged) {
        const size_t lds = (size_t)64 << k;
        // two workgroups per CU while two stages fit its LDS, one at k = 11; never more workgroups than tiles
        const size_t per_cu = 2 * lds <= (size_t)160 * 1024 ? 2 : 1, tiles = (total + (size_t)THREADS * ITEMS_PER_LANE - 1) / ((size_t)THREADS * ITEMS_PER_LANE);
        size_t rule = per_cu * (size_t)plan.cus;
        rule = rule > tiles ? tiles : rule;
        rule = rule > PKL_MAX_GRID ? PKL_MAX_GRID : rule;
        const unsigned grid = grid_or_0 ? grid_or_0 : (unsigned)rule;
        gather_staged_kernel<<<grid, THREADS, lds, stream>>>(d_idx, (const uint4*)d_g, (const uint4*)d_dt, total, 1u << k, (uint4*)d_hf, (uint4*)d_df, d_flags);
        return launched();
    }
    const unsigned grid = grid_or_0 ? grid_or_0 : lookups_grid(total);
    gather_kernel<<<grid, THREADS, 0, stream>>>(d_idx, (const fe*)d_g, (const fe*)d_dt, total, 1u << k, (fe*)d_hf, (fe*)d_df, d_flags);
    return launched();
}

}  // namespace pkl
