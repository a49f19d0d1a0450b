// layout.hpp -- the prover's device arena and the constants the kernels' launch rules and the host accessors share.  Host only.
#pragma once
#include "statement.hpp"

namespace pkl {

constexpr unsigned THREADS = 256;
// Tables up to 2^12 entries are counted in a workgroup-private LDS histogram: 4096 u32 bins = 16 KiB of the CU's 160 KiB, so nine
// workgroups still share a CU and zeroing plus flushing the bins (16 per lane) stays small against the lookups of a workgroup.
// Larger tables count with device-memory atomics, which spread over 2^13 and more addresses.
constexpr unsigned COUNT_LDS_MAX_K = 12;
// Tables up to 2^11 entries are staged in LDS by the gather: both sources, 2 * 2^11 * 32 B = 128 KiB of the CU's 160 KiB.
constexpr unsigned GATHER_LDS_MAX_K = 11;
// Elements per lane of table_kernel's batch inversion: 3 (E - 1) products and one inverse per lane.  E = 4 keeps the lane's live
// state (4 denominators, 3 prefix products, the inverse's five 9-limb values) in registers without scratch;
// profiles/r24_lookup_isa_table.md has the kernel's resource usage.
constexpr unsigned TABLE_BATCH = 4;
// lookups per lane the count and gather kernels' grid rule aims at
constexpr unsigned ITEMS_PER_LANE = 4;

// In bytes from the arena's start; every part 64-byte aligned
//   [h_f: 2^n fe] [d_f: 2^n fe] [d_t: 2^k fe] [g: 2^k fe] [h_t: 2^k fe] [partials: PKL_MAX_GRID fe] [sum: 1 fe]
//   [counts: 2^k u32] [first bad x: u64] [flags: u32 zero denominator, u32 index out of range]
struct Layout {
    size_t h_f = 0, d_f = 0, d_t = 0, g = 0, h_t = 0, partials = 0, sum = 0, counts = 0, bad = 0, flags = 0, total = 0;
};
inline Layout layout(const pkl_statement& s) {
    const size_t N = (size_t)32 << s.n, K = (size_t)32 << s.k;
    Layout L;
    L.d_f = L.h_f + N;
    L.d_t = L.d_f + N;
    L.g = L.d_t + K;
    L.h_t = L.g + K;
    L.partials = L.h_t + K;
    L.sum = L.partials + (size_t)32 * PKL_MAX_GRID;
    L.counts = L.sum + 64;
    L.bad = L.counts + ((((size_t)4 << s.k) + 63) & ~(size_t)63);
    L.flags = L.bad + 64;
    L.total = L.flags + 64;
    return L;
}
inline unsigned lookups_grid(size_t count) {
    const size_t per = (size_t)THREADS * ITEMS_PER_LANE, need = (count + per - 1) / per;
    return (unsigned)(need < 1 ? 1 : need > PKL_MAX_GRID ? PKL_MAX_GRID : need);
}
inline unsigned table_grid(size_t count) {
    const size_t per = (size_t)THREADS * TABLE_BATCH, need = (count + per - 1) / per;
    return (unsigned)(need < 1 ? 1 : need > PKL_MAX_GRID ? PKL_MAX_GRID : need);
}

}  // namespace pkl
