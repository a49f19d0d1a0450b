// layout.hpp -- the prover's device arena and the constants the kernels' launch rules and the host accessors share.  Host only.
#pragma once
#include "statement.hpp"

namespace pkg {

constexpr unsigned THREADS = 256;
// A layer of at most 2^TAIL_MAX_N entries is finished by one workgroup out of LDS: its first products (2^(TAIL_MAX_N - 1) elements,
// 16 KiB) are the largest layer the workgroup keeps, two products per lane; every layer below costs one barrier instead of a launch.
constexpr unsigned TAIL_MAX_N = 10;
// Layers per launch of tree_kernel: a lane holds 2^S elements (8 words each) and stores every intermediate layer.  1, 2 or 3; a
// prover's own value is a test and benchmark knob (tools/probes/grandproduct.hip).
constexpr unsigned TREE_MAX_LAYERS = 3;
constexpr unsigned TREE_LAYERS = 2;

// The arena of a pkg_prover: the tree in heap layout, tree[2^d + x] = V_d[x], 2^n elements (element 0 unused).  The n - 1 pks
// provers hold their own arenas (sumcheck/round.hpp's rule).
inline size_t tree_bytes(unsigned n) { return (size_t)32 << n; }
// the workgroups of a launch whose lanes own `lanes` low indices
inline unsigned lanes_grid(size_t lanes) {
    const size_t need = (lanes + THREADS - 1) / THREADS;
    return (unsigned)(need < 1 ? 1 : need > PKG_MAX_GRID ? PKG_MAX_GRID : need);
}

}  // namespace pkg
