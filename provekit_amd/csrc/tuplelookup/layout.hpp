// layout.hpp -- the prover's device arena and the constants the kernels' launch rules and the host accessors share.  Host only.
#pragma once
#include "statement.hpp"

namespace pkt {

constexpr unsigned THREADS = 256;
// Tables up to 2^12 entries are counted in a workgroup-private LDS histogram: 4096 u32 bins = 16 KiB of the CU's 160 KiB, the lookup
// library's limit (lookup/layout.hpp) for its reasons: nine workgroups still share a CU and zeroing plus flushing the bins (16 per
// lane) stays small against a workgroup's rows.  Larger tables count with device-memory atomics.
constexpr unsigned COUNT_LDS_MAX_K = 12;
// Rows per lane of tuple_leaf_kernel: a lane's rows are a workgroup-width apart, their W loads issued before the first product.  Two
// rows of W = 4 are 64 words of loads in flight next to one product's temporaries (profiles/r30_tuplelookup_isa_table.md).  One
// workgroup sweeps THREADS * LEAF_ITEMS rows.
constexpr unsigned LEAF_ITEMS = 2;
// rows per lane the count kernel's grid rule aims at (it takes one row per iteration)
constexpr unsigned COUNT_ITEMS = 4;

// In bytes from the arena's start; every part 64-byte aligned
//   [leafF: c 2^n fe] [leafT: 2^k fe] [counts: 2^k u32] [first bad stacked index: u64]
struct Layout {
    size_t leaf_f = 0, leaf_t = 0, counts = 0, bad = 0, total = 0;
};
inline Layout layout(const pkt_statement& s) {
    Layout L;
    L.leaf_t = L.leaf_f + ((size_t)32 << stacked_vars(s));
    L.counts = L.leaf_t + ((size_t)32 << s.k);
    L.bad = L.counts + ((((size_t)4 << s.k) + 63) & ~(size_t)63);
    L.total = L.bad + 64;
    return L;
}
// the workgroups (x dimension: one group's rows) of a launch whose lanes take `per_lane` of `rows` rows each
inline unsigned rows_grid(size_t rows, unsigned per_lane) {
    const size_t per = (size_t)THREADS * per_lane, need = (rows + per - 1) / per;
    return (unsigned)(need < 1 ? 1 : need > PKT_MAX_GRID ? PKT_MAX_GRID : need);
}

}  // namespace pkt
