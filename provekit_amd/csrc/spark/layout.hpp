// layout.hpp -- the prover's device arena and the constants the kernels' launch rules and the host accessors share.  Host only.
#pragma once
#include "statement.hpp"

namespace pkx {

constexpr unsigned THREADS = 256;
// An index histogram has 2^s (2^t) bins.  Up to 2^12 of them are counted in a workgroup-private LDS histogram: 4096 u32 bins = 16 KiB
// of the CU's 160 KiB, the tuple-lookup library's threshold (tuplelookup/layout.hpp).  Larger ones count with device-memory atomics.
constexpr unsigned COUNT_LDS_MAX = 12;
// Entries per lane of the gather kernel: a lane's entries are a workgroup-width apart, their index loads and then their gathers issued
// before the first store.  One workgroup sweeps THREADS * GATHER_ITEMS entries.
constexpr unsigned GATHER_ITEMS = 2;
// entries per lane the grid rule of the preprocessing kernels aims at (they take one entry per iteration)
constexpr unsigned MATRIX_ITEMS = 4;

// In bytes from the arena's start; every part 64-byte aligned
//   [eq(rx, .): 2^s fe] [eq(ry, .): 2^t fe] [the index column: 2^max(s, t) fe] [counts ROW: 2^s u32] [counts COL: 2^t u32] [first bad: u64]
struct Layout {
    size_t eq[2] = {0, 0}, iota = 0, counts[2] = {0, 0}, bad = 0, total = 0;
};
inline size_t aligned(size_t bytes) { return (bytes + 63) & ~(size_t)63; }
inline Layout layout(const pkx_statement& st) {
    Layout L;
    const unsigned widest = st.s > st.t ? st.s : st.t;
    L.eq[1] = L.eq[0] + aligned((size_t)32 << st.s);
    L.iota = L.eq[1] + aligned((size_t)32 << st.t);
    L.counts[0] = L.iota + aligned((size_t)32 << widest);
    L.counts[1] = L.counts[0] + aligned((size_t)4 << st.s);
    L.bad = L.counts[1] + aligned((size_t)4 << st.t);
    L.total = L.bad + 64;
    return L;
}
// the workgroups of a launch whose lanes take `per_lane` of `rows` rows each
inline unsigned rows_grid(size_t rows, unsigned per_lane) {
    const size_t per = (size_t)THREADS * per_lane, need = (rows + per - 1) / per;
    return (unsigned)(need < 1 ? 1 : need > PKX_MAX_GRID ? PKX_MAX_GRID : need);
}

}  // namespace pkx
