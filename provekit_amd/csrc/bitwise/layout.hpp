// layout.hpp -- the prover's device arena and the constants the kernels' launch rules and the host accessors share.  Host only.
#pragma once
#include "statement.hpp"

namespace pkb {

constexpr unsigned THREADS = 256;
// Tables of up to 2^12 rows (d <= 6) are counted in a workgroup-private LDS histogram: 4096 u32 bins = 16 KiB of the CU's 160 KiB, the
// tuple-lookup library's threshold (tuplelookup/layout.hpp) for its reasons.  Wider digits count with device-memory atomics.
constexpr unsigned COUNT_LDS_MAX_D = 6;
// Entries per lane of bitwise_decompose_kernel.  An entry is two 32-byte loads (three when c is given), 2 + 1 + 3 L products and 1 + 3 L
// 32-byte stores; one entry keeps 16 words of loads in flight next to one product's temporaries (the (bin, pending) pairs of the
// groups are wave-uniform: scalar registers).  The VGPR count and the occupancy are in profiles/r39_bitwise_isa_table.md.  One
// workgroup sweeps THREADS * DECOMPOSE_ITEMS entries.
constexpr unsigned DECOMPOSE_ITEMS = 1;
// entries per lane the grid rule of the one-product kernels aims at (table, m: one entry per iteration)
constexpr unsigned PLAIN_ITEMS = 4;

// In bytes from the arena's start; every part 64-byte aligned
//   [the table's columns u, v, u op v: 2^(2d) fe each] [counts: 2^(2d) u32] [first bad entry: u64]
struct Layout {
    size_t table[3] = {0, 0, 0}, counts = 0, bad = 0, total = 0;
};
inline size_t aligned(size_t bytes) { return (bytes + 63) & ~(size_t)63; }
inline Layout layout(const pkb_statement& s) {
    const unsigned k = 2 * s.d;
    Layout L;
    for (int j = 1; j < 3; j++) L.table[j] = L.table[j - 1] + aligned((size_t)32 << k);
    L.counts = L.table[2] + aligned((size_t)32 << k);
    L.bad = L.counts + aligned((size_t)4 << k);
    L.total = L.bad + 64;
    return L;
}
// the workgroups of a launch whose lanes take `per_lane` of `rows` rows each
inline unsigned rows_grid(size_t rows, unsigned per_lane) {
    const size_t per = (size_t)THREADS * per_lane, need = (rows + per - 1) / per;
    return (unsigned)(need < 1 ? 1 : need > PKB_MAX_GRID ? PKB_MAX_GRID : need);
}

}  // namespace pkb
