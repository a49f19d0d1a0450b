// layout.hpp -- the prover's device arena and the constants the kernels' launch rules and the host accessors share.  Host only.
#pragma once
#include "statement.hpp"

namespace pkr {

constexpr unsigned THREADS = 256;
// Limbs of up to 12 bits are counted in a workgroup-private LDS histogram: 4096 u32 bins = 16 KiB of the CU's 160 KiB, the tuple-lookup
// library's threshold (tuplelookup/layout.hpp) for its reasons.  Wider limbs count with device-memory atomics.
constexpr unsigned COUNT_LDS_MAX_K = 12;
// Entries per lane of range_decompose_kernel: a lane's entries are a workgroup-width apart, their loads issued before the first
// product.  An entry is one 32-byte load, 1 + L products and L 32-byte stores; two entries keep 16 words of loads in flight next to one
// product's temporaries (the (bin, pending) pairs of the groups are wave-uniform: scalar registers): 69 VGPRs, seven waves a SIMD
// (profiles/r38_rangecheck_isa_table.md).  One workgroup sweeps THREADS * DECOMPOSE_ITEMS entries.
constexpr unsigned DECOMPOSE_ITEMS = 2;
// entries per lane the grid rule of the one-product kernels aims at (scale, index, m: one entry per iteration)
constexpr unsigned PLAIN_ITEMS = 4;

// In bytes from the arena's start; every part 64-byte aligned
//   [I_k: 2^k fe] [the scaled top column: 2^n fe, only when r < k] [counts: 2^k u32] [first bad entry: u64]
struct Layout {
    size_t iota = 0, scaled = 0, counts = 0, bad = 0, total = 0;
};
inline size_t aligned(size_t bytes) { return (bytes + 63) & ~(size_t)63; }
inline Layout layout(const pkr_statement& s) {
    const Plan P = plan_of(s.bits, s.k);
    Layout L;
    L.scaled = L.iota + aligned((size_t)32 << s.k);
    L.counts = L.scaled + (P.r < s.k ? aligned((size_t)32 << s.n) : 0);
    L.bad = L.counts + aligned((size_t)4 << s.k);
    L.total = L.bad + 64;
    return L;
}
// the workgroups of a launch whose lanes take `per_lane` of `rows` rows each
inline unsigned rows_grid(size_t rows, unsigned per_lane) {
    const size_t per = (size_t)THREADS * per_lane, need = (rows + per - 1) / per;
    return (unsigned)(need < 1 ? 1 : need > PKR_MAX_GRID ? PKR_MAX_GRID : need);
}

}  // namespace pkr
