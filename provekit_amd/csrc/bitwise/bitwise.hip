// bitwise.hip -- the HIP kernels libprovekit_bitwise.so adds (gfx950): the fused pass that forms c = a op b, splits a, b and c into their
// digit columns and counts the digit rows' multiplicities, and the operation's table.
//
// bitwise_decompose_kernel<LDS, L> (the hot pass; one instance per digit count and histogram kind): per entry two coalesced 32-byte loads (three when c is given), issued before the first
//   product; both operands out of Montgomery form by one product each; ALL words of each canonical value checked against 2^bits
//   (words 2 .. 7 zero, and the low 64 bits below 2^bits: a value with only a high word set fails); a op b formed on the low 64 bits; a
//   given c taken out of Montgomery form and compared, all words.  A failure lowers the 64-bit cell `bad` with atomicMin to
//   (x << 2) | case, so the cell ends as the smallest failing entry with its case (kernels.hpp).  c (when not given) and the 3 L digits
//   go back to Montgomery form by one product with R^2 each and are stored coalesced, and the bin (a_i << d) | b_i of every one of the
//   c groups of the plan (statement.hpp) is counted: the digits, and the spare group's repeat of digit 0.  No gather and no index list:
//   a row's place in the table is made of its own digits.  A failing entry is not counted.
//   Bins follow tuplelookup/tuple.hip's rule: up to 2^12 of them (d <= COUNT_LDS_MAX_D) in a workgroup-private LDS histogram flushed
//   once per non-zero bin, more with vector atomics on device memory.  The wavefront aggregation is kept PER GROUP: a pair of
//   wave-uniform (bin, pending) registers for each of the c groups, added when that group's bin changes and at the end.  Columns of
//   small words put every high digit row in bin 0: one atomic per wavefront and group instead of 64.  A wavefront with mixed bins in a
//   group adds lane by lane in that group.  Integer adds: the counts are exact in any order, no bit depends on the grid.
// mont_kernel writes m as Montgomery elements (tuple.hip's rule, written out again: that file's kernels stay as they are).
// bitwise_table_kernel: the table's three columns, once per prover.
//
// All loads and stores are ordinary vector accesses; the atomics are vector atomics on device memory or LDS.
#include <hip/hip_runtime.h>

#include "../fe29.hpp"
#include "kernels.hpp"

using namespace pk;

namespace pkb {

namespace {

typedef unsigned long long u64a;  // atomicMin's 64-bit type

struct DigitColumns {
    uint64_t* col[3][PKB_MAX_DIGITS];  // [j][i]: digit i of a, b, c
};
struct TableColumns {
    uint64_t* col[3];
};

// an integer below 2^64 as a Montgomery element: one product
__device__ __forceinline__ fe word_mont(uint64_t c) {
    fe x = fe_zero();
    x.v[0] = (u32)c, x.v[1] = (u32)(c >> 32);
    return fe_mulx(x, fe_r2());
}

__global__ __launch_bounds__(THREADS) void bitwise_table_kernel(size_t rows, unsigned op, unsigned d, TableColumns out) {
    const u32 mask = (1u << d) - 1;
    for (size_t y = (size_t)blockIdx.x * THREADS + threadIdx.x; y < rows; y += (size_t)gridDim.x * THREADS) {
        const u32 u = (u32)(y >> d), v = (u32)y & mask;
        fe_store((fe*)out.col[0] + y, word_mont(u));
        fe_store((fe*)out.col[1] + y, word_mont(v));
        fe_store((fe*)out.col[2] + y, word_mont(apply(op, u, v)));
    }
}

__global__ __launch_bounds__(THREADS) void mont_kernel(const u32* __restrict__ counts, size_t size, fe* __restrict__ m_out) {
    for (size_t y = (size_t)blockIdx.x * THREADS + threadIdx.x; y < size; y += (size_t)gridDim.x * THREADS) fe_store(m_out + y, word_mont(counts[y]));
}

// the low 64 bits of a canonical value, and whether the value is an integer below 2^bits (bits <= 48)
__device__ __forceinline__ bool word_of(const fe& c, unsigned bits, uint64_t& lo) {
    lo = (uint64_t)c.v[0] | (uint64_t)c.v[1] << 32;
    const u32 high = c.v[2] | c.v[3] | c.v[4] | c.v[5] | c.v[6] | c.v[7];
    return high == 0 && (lo >> bits) == 0;
}

// L is a template parameter: with the digit count known the unused column pointers and their guards fall away, which keeps the kernel's
// scalar registers (12 column pointers at L = 4, the groups' (bin, pending) pairs) inside the file without a spill
template <bool LDS, unsigned L>
__global__ __launch_bounds__(THREADS) void bitwise_decompose_kernel(const fe* __restrict__ a, const fe* __restrict__ b, fe* __restrict__ c, bool c_given, size_t total,
                                                                    unsigned op, unsigned d, DigitColumns out, u32* __restrict__ counts, u64a* __restrict__ bad) {
    constexpr int I = (int)DECOMPOSE_ITEMS, GROUPS = PKB_MAX_DIGITS;
    __shared__ u32 bins[LDS ? (1u << (2 * COUNT_LDS_MAX_D)) : 1];
    const Plan P = plan_of(L);  // wave-uniform
    const unsigned bits = L * d;
    const u32 size = 1u << (2 * d), mask = (1u << d) - 1;
    if (LDS) {
        for (u32 y = threadIdx.x; y < size; y += THREADS) bins[y] = 0;
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
        fe va[I], vb[I], vc[I];
#pragma unroll
        for (int i = 0; i < I; i++) {
            const size_t x = x0 + (size_t)i * THREADS;
            va[i] = x < total ? fe_load(a + x) : fe_zero();
            vb[i] = x < total ? fe_load(b + x) : fe_zero();
            vc[i] = x < total && c_given ? fe_load(c + x) : fe_zero();
        }
#pragma unroll
        for (int i = 0; i < I; i++) {
            const size_t x = x0 + (size_t)i * THREADS;
            const bool inside = x < total;
            uint64_t wa, wb, wc;
            const bool a_fits = word_of(fe_from_montx(va[i]), bits, wa);
            const bool b_fits = word_of(fe_from_montx(vb[i]), bits, wb);
            const uint64_t w = apply(op, wa, wb);
            bool c_right = true;
            if (c_given) c_right = word_of(fe_from_montx(vc[i]), bits, wc) && wc == w;  // wave-uniform branch
            const bool fits = a_fits && b_fits && c_right;
            const bool ok = inside && fits;
            if (inside && !fits) atomicMin(bad, (u64a)x << 2 | (!a_fits ? BAD_A : !b_fits ? BAD_B : BAD_C));
            if (inside) {
                if (!c_given) fe_store(c + x, word_mont(w));
#pragma unroll
                for (int j = 0; j < GROUPS; j++)  // the digits, each back to Montgomery form; of a failing entry the low 64 bits' (not meaningful)
                    if ((unsigned)j < L) {
                        fe_store((fe*)out.col[0][j] + x, word_mont((u32)(wa >> (d * j)) & mask));
                        fe_store((fe*)out.col[1][j] + x, word_mont((u32)(wb >> (d * j)) & mask));
                        fe_store((fe*)out.col[2][j] + x, word_mont((u32)(w >> (d * j)) & mask));
                    }
            }
            const u64a voters = __ballot(ok);
            if (voters == 0) continue;  // wave-uniform
            const unsigned leader = (unsigned)__ffsll((long long)voters) - 1;
#pragma unroll
            for (int g = 0; g < GROUPS; g++) {
                if ((unsigned)g >= P.c) continue;  // wave-uniform
                // group g's bin by the plan: the row (a_i, b_i, a_i op b_i) stands at (a_i << d) | b_i, below 2^(2d) by the masks
                const unsigned sh = d * P.digit_of[g];
                const u32 y = ((u32)(wa >> sh) & mask) << d | ((u32)(wb >> sh) & mask);
                const u32 first = __shfl(y, leader, 64);
                const bool one_bin = __ballot(ok && y == first) == voters;  // wave-uniform
                if (one_bin) {
                    if (pending[g] && pending_bin[g] != first) flush(g);
                    pending_bin[g] = first;
                    pending[g] += (u32)__popcll(voters);
                } else if (ok) {
                    if (LDS)
                        atomicAdd(&bins[y], 1u);
                    else
                        atomicAdd(counts + y, 1u);
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < GROUPS; g++) flush(g);
    if (LDS) {
        __syncthreads();
        for (u32 y = threadIdx.x; y < size; y += THREADS) {
            const u32 n = bins[y];
            if (n) atomicAdd(counts + y, n);
        }
    }
}

int launched() { return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP; }
bool shape_ok(unsigned op, unsigned d, unsigned L) { return op < PKB_OP_COUNT && d >= 1 && d <= PKB_MAX_DIGIT_BITS && L >= 1 && L <= PKB_MAX_DIGITS; }
unsigned grid_for(unsigned grid_or_0, size_t rows, unsigned per_lane) { return grid_or_0 ? grid_or_0 : rows_grid(rows, per_lane); }

}  // namespace

int table_launch(hipStream_t stream, unsigned op, unsigned d, uint64_t* const d_cols[3], unsigned grid_or_0) {
    if (!shape_ok(op, d, 1) || grid_or_0 > PKB_MAX_GRID || !d_cols) return PK_ERR_BAD_ARG;
    TableColumns out{};
    for (int j = 0; j < 3; j++)
        if (!(out.col[j] = d_cols[j])) return PK_ERR_BAD_ARG;
    const size_t rows = (size_t)1 << (2 * d);
    bitwise_table_kernel<<<grid_for(grid_or_0, rows, PLAIN_ITEMS), THREADS, 0, stream>>>(rows, op, d, out);
    return launched();
}

int decompose_launch(hipStream_t stream, unsigned n, unsigned op, unsigned d, unsigned L, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, bool c_given,
                     uint64_t* const* d_digits, uint32_t* d_counts, unsigned long long* d_bad, uint64_t* d_m_out, unsigned grid_or_0) {
    if (n < 1 || n > PKB_MAX_VARS || !shape_ok(op, d, L) || grid_or_0 > PKB_MAX_GRID) return PK_ERR_BAD_ARG;
    if (!d_a || !d_b || !d_c || !d_digits || !d_counts || !d_bad || !d_m_out) return PK_ERR_BAD_ARG;
    DigitColumns out{};
    for (unsigned j = 0; j < 3; j++)
        for (unsigned i = 0; i < L; i++)
            if (!(out.col[j][i] = d_digits[j * L + i])) return PK_ERR_BAD_ARG;
    const size_t total = (size_t)1 << n, size = (size_t)1 << (2 * d);
    if (hipMemsetAsync(d_counts, 0, 4 * size, stream) != hipSuccess || hipMemsetAsync(d_bad, 0xff, 8, stream) != hipSuccess) return PK_ERR_HIP;
    const unsigned grid = grid_for(grid_or_0, total, DECOMPOSE_ITEMS);
    const bool lds = d <= COUNT_LDS_MAX_D;
#define PKB_DECOMPOSE(DIGITS)                                                                                                                                      \
    case DIGITS:                                                                                                                                                   \
        if (lds)                                                                                                                                                   \
            bitwise_decompose_kernel<true, DIGITS><<<grid, THREADS, 0, stream>>>((const fe*)d_a, (const fe*)d_b, (fe*)d_c, c_given, total, op, d, out, d_counts, d_bad); \
        else                                                                                                                                                       \
            bitwise_decompose_kernel<false, DIGITS><<<grid, THREADS, 0, stream>>>((const fe*)d_a, (const fe*)d_b, (fe*)d_c, c_given, total, op, d, out, d_counts, d_bad); \
        break;
    switch (L) {
        PKB_DECOMPOSE(1)
        PKB_DECOMPOSE(2)
        PKB_DECOMPOSE(3)
        PKB_DECOMPOSE(4)
    }
#undef PKB_DECOMPOSE
    mont_kernel<<<grid_for(grid_or_0, size, PLAIN_ITEMS), THREADS, 0, stream>>>(d_counts, size, (fe*)d_m_out);
    return launched();
}

}  // namespace pkb
