// layout.hpp -- the prover's device arena and the constants the kernels' launch rules and the host accessors share.  Host only.
#pragma once
#include "../gkr/launch.hpp"
#include "statement.hpp"

namespace pkg {

// the width of a workgroup, the layers per launch of tree_kernel (a lane holds 2^S elements of 8 words) and the launch rules: gkr/launch.hpp
using pk::gkr::THREADS;
using pk::gkr::TREE_LAYERS;
using pk::gkr::TREE_MAX_LAYERS;
// A layer of at most 2^TAIL_MAX_N entries is finished by one workgroup out of LDS: its first products (2^(TAIL_MAX_N - 1) elements,
// 16 KiB) are the largest layer the workgroup keeps, two products per lane; every layer below costs one barrier instead of a launch.
constexpr unsigned TAIL_MAX_N = 10;

// The arena of a pkg_prover: the tree in heap layout, tree[2^d + x] = V_d[x], 2^n elements (element 0 unused).  The n - 1 pks
// provers hold their own arenas (sumcheck/round.hpp's rule).
inline size_t tree_bytes(unsigned n) { return (size_t)32 << n; }
// the workgroups of a launch whose lanes own `lanes` low indices
inline unsigned lanes_grid(size_t lanes) { return pk::gkr::lanes_grid(lanes, PKG_MAX_GRID); }

}  // namespace pkg
