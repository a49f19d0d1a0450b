// mem.hip -- the HIP kernels libprovekit_memcheck.so adds (gfx950): the trace builder of a read-write memory and the two stacked
// leaf tables of its memory-checking argument.
//
// THE TRACE BUILDER (the method of witness.hip's Spice blocks, written for tables rather than witness indices):
//   mem_key_kernel      validates every address BEFORE anything follows it (addr[i] < 2^k; a failure lowers the 64-bit cell `bad` with
//                       atomicMin to i, so the cell ends as the smallest failing index, and the operation goes on as address 0), writes
//                       a[i] and the key (addr << n | i): the n + k significant bits contiguous, so the one radix sort walks no dead
//                       bits.  The same launch sets fin = init and ft = 0 for every cell.
//   (rocPRIM radix sort of the keys over bits 0 .. n + k: equal addresses become one run, in operation order)
//   mem_resolve_kernel  a lane takes one sorted key and looks at its two neighbours: the left one with the same address is the write this
//                       operation reads (rv = its wv, rt = its time), otherwise init and 0; the last operation of a run writes fin and
//                       ft.  It also stores the integer i - rt_i (u32, at index i) for the count.
//   mem_count_kernel<LDS>  the histogram of those integers, 2^n bins: up to 2^COUNT_LDS_MAX_N bins in a workgroup-private LDS histogram
//                       flushed once per non-zero bin, larger ones with atomics on device memory.  As in tuplelookup/tuple.hip a
//                       wavefront whose lanes all name one bin keeps (bin, count) in wave-uniform registers and adds when the bin
//                       changes and at its end: one address under full skew (every operation on one cell gives i - rt_i = 0 throughout).  Integer adds: the counts are exact in any order.  mem_mont_kernel writes m as elements.
//
// THE LEAVES: mem_ops_leaf_kernel writes both halves of side OPS's denominators in one pass over a, wv, rv, rt (and f_i = i - rt_i,
// from the rt it holds anyway); mem_cells_leaf_kernel does the same for side MEM.  The time i + 1 and the cell index j come from the
// lane's index.  As tuple_leaf_kernel: one row per lane, LEAF_ITEMS rows a workgroup-width apart, every load issued before the first
// product, Horner in beta.  Products, sums and differences of values below p are exact values below p: the bits depend neither on the
// grid nor on the rows per lane.
//
// All loads and stores are ordinary vector accesses; the atomics are vector atomics on device memory or LDS.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "../fe29.hpp"
#include "kernels.hpp"

using namespace pk;

namespace pkm {

namespace {

typedef unsigned long long u64;

// a small integer as a Montgomery element: one product
__device__ __forceinline__ fe small_mont(u32 c) {
    fe x = fe_zero();
    x.v[0] = c;
    return fe_mulx(x, fe_r2());
}

__global__ __launch_bounds__(THREADS) void sign_kernel(size_t half, fe* __restrict__ out) {
    const fe plus = fe_one(), minus = fe_neg(fe_one());
    for (size_t x = (size_t)blockIdx.x * THREADS + threadIdx.x; x < 2 * half; x += (size_t)gridDim.x * THREADS) fe_store(out + x, x < half ? plus : minus);
}

__global__ __launch_bounds__(THREADS) void iota_kernel(size_t rows, fe* __restrict__ out) {
    for (size_t x = (size_t)blockIdx.x * THREADS + threadIdx.x; x < rows; x += (size_t)gridDim.x * THREADS) fe_store(out + x, small_mont((u32)x));
}

__global__ __launch_bounds__(THREADS) void mem_key_kernel(const u32* __restrict__ addr, unsigned n, unsigned k, const fe* __restrict__ init, fe* __restrict__ a_out,
                                                          u64* __restrict__ keys, fe* __restrict__ fin, fe* __restrict__ ft, u64* __restrict__ bad) {
    const size_t rows = (size_t)1 << n, cells = (size_t)1 << k, stride = (size_t)gridDim.x * THREADS, first = (size_t)blockIdx.x * THREADS + threadIdx.x;
    for (size_t i = first; i < rows; i += stride) {
        u32 ad = addr[i];
        if (ad >> k) {  // k <= 27: outside the memory.  Reported, and followed as cell 0
            atomicMin(bad, (u64)i);
            ad = 0;
        }
        fe_store(a_out + i, small_mont(ad));
        keys[i] = ((u64)ad << n) | (u64)i;
    }
    for (size_t j = first; j < cells; j += stride) {  // cells no operation touches keep their initial value, time 0
        fe_store(fin + j, fe_load(init + j));
        fe_store(ft + j, fe_zero());
    }
}

// sorted by (address, operation): the left neighbour with the same address is the previous operation on that address.  Every address
// in a key is below 2^k and every operation index below 2^n (mem_key_kernel made them so): each store is inside its table.
__global__ __launch_bounds__(THREADS) void mem_resolve_kernel(const u64* __restrict__ sorted, unsigned n, const fe* __restrict__ wv, const fe* __restrict__ init,
                                                              fe* __restrict__ rv, fe* __restrict__ rt, fe* __restrict__ fin, fe* __restrict__ ft,
                                                              u32* __restrict__ f_int) {
    const size_t rows = (size_t)1 << n;
    const u64 mask = rows - 1;
    for (size_t s = (size_t)blockIdx.x * THREADS + threadIdx.x; s < rows; s += (size_t)gridDim.x * THREADS) {
        const u64 key = sorted[s], left = s > 0 ? sorted[s - 1] : 0, right = s + 1 < rows ? sorted[s + 1] : 0;
        const u64 a = key >> n;
        const u32 i = (u32)(key & mask), prev = (u32)(left & mask);
        const bool has_prev = s > 0 && (left >> n) == a;
        const bool last = s + 1 == rows || (right >> n) != a;
        const u32 time = has_prev ? prev + 1 : 0;  // prev < i: the sort orders a run by operation
        fe_store(rv + i, has_prev ? fe_load(wv + prev) : fe_load(init + a));
        fe_store(rt + i, small_mont(time));
        f_int[i] = i - time;
        if (last) {
            fe_store(fin + a, fe_load(wv + i));
            fe_store(ft + a, small_mont(i + 1));
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(THREADS) void mem_count_kernel(const u32* __restrict__ f_int, unsigned n, u32* __restrict__ counts) {
    __shared__ u32 bins[LDS ? (1u << COUNT_LDS_MAX_N) : 1];
    const u32 size = 1u << n;
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
            v = f_int[x];
            ok = v < size;  // always, by mem_resolve_kernel's construction; a bin is never taken on trust
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

__global__ __launch_bounds__(THREADS) void mem_mont_kernel(const u32* __restrict__ counts, size_t size, fe* __restrict__ m_out) {
    for (size_t y = (size_t)blockIdx.x * THREADS + threadIdx.x; y < size; y += (size_t)gridDim.x * THREADS) fe_store(m_out + y, small_mont(counts[y]));
}

__global__ __launch_bounds__(THREADS) void mem_ops_leaf_kernel(const fe* __restrict__ a, const fe* __restrict__ wv, const fe* __restrict__ rv, const fe* __restrict__ rt,
                                                               size_t rows, fe gamma, fe beta, fe* __restrict__ q, fe* __restrict__ f_or_null) {
    constexpr int I = (int)LEAF_ITEMS;
    const size_t tile = (size_t)THREADS * I, tiles = (rows + tile - 1) / tile;
    for (size_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const size_t x0 = tl * tile + threadIdx.x;
        fe v[I][4];
#pragma unroll
        for (int i = 0; i < I; i++) {
            const size_t x = x0 + (size_t)i * THREADS;
            const bool in = x < rows;
            v[i][0] = in ? fe_load(a + x) : fe_zero();
            v[i][1] = in ? fe_load(wv + x) : fe_zero();
            v[i][2] = in ? fe_load(rv + x) : fe_zero();
            v[i][3] = in ? fe_load(rt + x) : fe_zero();
        }
#pragma unroll
        for (int i = 0; i < I; i++) {
            const size_t x = x0 + (size_t)i * THREADS;
            if (x >= rows) continue;
            const fe time = small_mont((u32)x + 1);  // the write's global time i + 1
            const fe write = fe_add(fe_mulx(fe_add(fe_mulx(time, beta), v[i][1]), beta), v[i][0]);
            const fe read = fe_add(fe_mulx(fe_add(fe_mulx(v[i][3], beta), v[i][2]), beta), v[i][0]);
            fe_store(q + x, fe_sub(gamma, write));
            fe_store(q + rows + x, fe_sub(gamma, read));
            if (f_or_null) fe_store(f_or_null + x, fe_sub(fe_sub(time, fe_one()), v[i][3]));  // i - rt_i
        }
    }
}

__global__ __launch_bounds__(THREADS) void mem_cells_leaf_kernel(const fe* __restrict__ init, const fe* __restrict__ fin, const fe* __restrict__ ft, size_t cells,
                                                                 fe gamma, fe beta, fe* __restrict__ q) {
    constexpr int I = (int)LEAF_ITEMS;
    const size_t tile = (size_t)THREADS * I, tiles = (cells + tile - 1) / tile;
    for (size_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const size_t x0 = tl * tile + threadIdx.x;
        fe v[I][3];
#pragma unroll
        for (int i = 0; i < I; i++) {
            const size_t x = x0 + (size_t)i * THREADS;
            const bool in = x < cells;
            v[i][0] = in ? fe_load(init + x) : fe_zero();
            v[i][1] = in ? fe_load(fin + x) : fe_zero();
            v[i][2] = in ? fe_load(ft + x) : fe_zero();
        }
#pragma unroll
        for (int i = 0; i < I; i++) {
            const size_t x = x0 + (size_t)i * THREADS;
            if (x >= cells) continue;
            const fe cell = small_mont((u32)x);
            fe_store(q + x, fe_sub(gamma, fe_add(fe_mulx(v[i][0], beta), cell)));
            fe_store(q + cells + x, fe_sub(gamma, fe_add(fe_mulx(fe_add(fe_mulx(v[i][2], beta), v[i][1]), beta), cell)));
        }
    }
}

int launched() { return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP; }
bool vars_ok(unsigned v, unsigned grid) { return v >= 1 && v <= PKM_MAX_VARS && grid <= PKM_MAX_GRID; }
unsigned grid_for(unsigned grid_or_0, size_t rows, unsigned per_lane) { return grid_or_0 ? grid_or_0 : rows_grid(rows, per_lane); }
void record(hipEvent_t* ev, int which, hipStream_t stream) {
    if (ev) (void)hipEventRecord(ev[which], stream);
}

}  // namespace

size_t sort_tmp_bytes(unsigned n, unsigned k) {
    size_t bytes = 0;
    if (hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, (const u64*)nullptr, (u64*)nullptr, (int)(1u << n), 0, (int)(n + k), nullptr) != hipSuccess) return 0;
    return bytes ? bytes : 1;
}

int sign_launch(hipStream_t stream, unsigned v, uint64_t* d_sign, unsigned grid_or_0) {
    if (!vars_ok(v, grid_or_0) || !d_sign) return PK_ERR_BAD_ARG;
    const size_t half = (size_t)1 << v;
    sign_kernel<<<grid_for(grid_or_0, 2 * half, TRACE_ITEMS), THREADS, 0, stream>>>(half, (fe*)d_sign);
    return launched();
}

int iota_launch(hipStream_t stream, unsigned n, uint64_t* d_t, unsigned grid_or_0) {
    if (!vars_ok(n, grid_or_0) || !d_t) return PK_ERR_BAD_ARG;
    const size_t rows = (size_t)1 << n;
    iota_kernel<<<grid_for(grid_or_0, rows, TRACE_ITEMS), THREADS, 0, stream>>>(rows, (fe*)d_t);
    return launched();
}

int trace_launch(hipStream_t stream, unsigned n, unsigned k, const TraceTables& t, const TraceScratch& s, unsigned grid_or_0, hipEvent_t* ev) {
    if (!vars_ok(n, grid_or_0) || !vars_ok(k, 0)) return PK_ERR_BAD_ARG;
    if (!t.addr || !t.wv || !t.init || !t.a || !t.rv || !t.rt || !t.m || !t.fin || !t.ft) return PK_ERR_BAD_ARG;
    if (!s.keys || !s.sorted || !s.counts || !s.sort_tmp || !s.bad) return PK_ERR_BAD_ARG;
    const size_t rows = (size_t)1 << n, cells = (size_t)1 << k;
    const unsigned grid = grid_for(grid_or_0, rows, TRACE_ITEMS);
    if (hipMemsetAsync(s.counts, 0, 4 * rows, stream) != hipSuccess || hipMemsetAsync(s.bad, 0xff, 8, stream) != hipSuccess) return PK_ERR_HIP;
    record(ev, 0, stream);
    mem_key_kernel<<<grid_for(grid_or_0, rows > cells ? rows : cells, TRACE_ITEMS), THREADS, 0, stream>>>(t.addr, n, k, (const fe*)t.init, (fe*)t.a, s.keys, (fe*)t.fin,
                                                                                                          (fe*)t.ft, s.bad);
    record(ev, 1, stream);
    size_t tmp = s.sort_tmp_bytes;
    if (hipcub::DeviceRadixSort::SortKeys(s.sort_tmp, tmp, (const u64*)s.keys, s.sorted, (int)rows, 0, (int)(n + k), stream) != hipSuccess) return PK_ERR_HIP;
    record(ev, 2, stream);
    u32* f_int = (u32*)s.keys;  // the sort's input is free now
    mem_resolve_kernel<<<grid, THREADS, 0, stream>>>(s.sorted, n, (const fe*)t.wv, (const fe*)t.init, (fe*)t.rv, (fe*)t.rt, (fe*)t.fin, (fe*)t.ft, f_int);
    record(ev, 3, stream);
    if (n <= COUNT_LDS_MAX_N)
        mem_count_kernel<true><<<grid, THREADS, 0, stream>>>(f_int, n, s.counts);
    else
        mem_count_kernel<false><<<grid, THREADS, 0, stream>>>(f_int, n, s.counts);
    mem_mont_kernel<<<grid, THREADS, 0, stream>>>(s.counts, rows, (fe*)t.m);
    record(ev, 4, stream);
    return launched();
}

int ops_leaf_launch(hipStream_t stream, unsigned n, const LeafColumns& c, const uint64_t gamma[4], const uint64_t beta[4], uint64_t* d_q, uint64_t* d_f_or_null,
                    unsigned grid_or_0) {
    if (!vars_ok(n, grid_or_0) || !c.a || !c.wv || !c.rv || !c.rt || !gamma || !beta || !d_q) return PK_ERR_BAD_ARG;
    const size_t rows = (size_t)1 << n;
    fe g, b;
    memcpy(g.v, gamma, 32), memcpy(b.v, beta, 32);
    mem_ops_leaf_kernel<<<grid_for(grid_or_0, rows, LEAF_ITEMS), THREADS, 0, stream>>>((const fe*)c.a, (const fe*)c.wv, (const fe*)c.rv, (const fe*)c.rt, rows, g, b,
                                                                                       (fe*)d_q, (fe*)d_f_or_null);
    return launched();
}

int cells_leaf_launch(hipStream_t stream, unsigned k, const LeafColumns& c, const uint64_t gamma[4], const uint64_t beta[4], uint64_t* d_q, unsigned grid_or_0) {
    if (!vars_ok(k, grid_or_0) || !c.init || !c.fin || !c.ft || !gamma || !beta || !d_q) return PK_ERR_BAD_ARG;
    const size_t cells = (size_t)1 << k;
    fe g, b;
    memcpy(g.v, gamma, 32), memcpy(b.v, beta, 32);
    mem_cells_leaf_kernel<<<grid_for(grid_or_0, cells, LEAF_ITEMS), THREADS, 0, stream>>>((const fe*)c.init, (const fe*)c.fin, (const fe*)c.ft, cells, g, b, (fe*)d_q);
    return launched();
}

}  // namespace pkm
