// layout.hpp -- the prover's device arena and the constants the kernels' launch rules and the host accessors share.  Host only.
#pragma once
#include "statement.hpp"

namespace pkm {

constexpr unsigned THREADS = 256;
// The time side's histogram has 2^n bins.  Up to 2^11 of them are counted in a workgroup-private LDS histogram: 2048 u32 bins = 8 KiB
// of the CU's 160 KiB, below the tuple-lookup library's 2^12 (tuplelookup/layout.hpp): zeroing plus flushing the bins is 8 per lane.
// Larger ones count with device-memory atomics.
constexpr unsigned COUNT_LDS_MAX_N = 11;
// Rows per lane of the two leaf kernels: a lane's rows are a workgroup-width apart, their loads issued before the first product, as
// tuple_leaf_kernel's.  One workgroup sweeps THREADS * LEAF_ITEMS rows.
constexpr unsigned LEAF_ITEMS = 2;
// rows per lane the grid rule of the trace builder's kernels aims at (they take one row per iteration)
constexpr unsigned TRACE_ITEMS = 4;

// In bytes from the arena's start; every part 64-byte aligned
//   [q OPS: 2^(n+1) fe] [q MEM: 2^(k+1) fe] [sign OPS: 2^(n+1) fe] [sign MEM: 2^(k+1) fe] [f: 2^n fe] [t: 2^n fe]
//   [keys: 2^n u64; after the sort the u32 values of f] [sorted: 2^n u64] [counts: 2^n u32] [the sort's temporary storage] [first bad: u64]
struct Layout {
    size_t q[2] = {0, 0}, sign[2] = {0, 0}, f = 0, t = 0, keys = 0, sorted = 0, counts = 0, sort_tmp = 0, bad = 0, total = 0;
};
inline size_t aligned(size_t bytes) { return (bytes + 63) & ~(size_t)63; }
inline Layout layout(const pkm_statement& s, size_t sort_tmp_bytes) {
    Layout L;
    const size_t ops = (size_t)64 << s.n, mem = (size_t)64 << s.k, col = (size_t)32 << s.n;
    L.q[1] = L.q[0] + ops;
    L.sign[0] = L.q[1] + mem;
    L.sign[1] = L.sign[0] + ops;
    L.f = L.sign[1] + mem;
    L.t = L.f + col;
    L.keys = L.t + col;
    L.sorted = L.keys + aligned((size_t)8 << s.n);
    L.counts = L.sorted + aligned((size_t)8 << s.n);
    L.sort_tmp = L.counts + aligned((size_t)4 << s.n);
    L.bad = L.sort_tmp + aligned(sort_tmp_bytes);
    L.total = L.bad + 64;
    return L;
}
// the workgroups of a launch whose lanes take `per_lane` of `rows` rows each
inline unsigned rows_grid(size_t rows, unsigned per_lane) {
    const size_t per = (size_t)THREADS * per_lane, need = (rows + per - 1) / per;
    return (unsigned)(need < 1 ? 1 : need > PKM_MAX_GRID ? PKM_MAX_GRID : need);
}

}  // namespace pkm
