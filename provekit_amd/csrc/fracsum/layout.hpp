// layout.hpp -- the prover's device arena and the constants the kernels' launch rules and the host accessors share.  Host only.
#pragma once
#include "../gkr/launch.hpp"
#include "statement.hpp"

namespace pkf {

// the width of a workgroup, the layers per launch of frac_tree_kernel (a lane holds 2^S (p, q) pairs of 16 words) and the launch rules:
// gkr/launch.hpp
using pk::gkr::THREADS;
using pk::gkr::TREE_LAYERS;
using pk::gkr::TREE_MAX_LAYERS;
// A layer of at most 2^TAIL_MAX_N entries is finished by one workgroup out of LDS.  Two arrays are live (numerators and
// denominators), so the limit is one less than the grand product's 10: the first combined layer is 2 x 2^(TAIL_MAX_N - 1) elements,
// 16 KiB, one node per lane; every layer below costs one barrier instead of a launch.
constexpr unsigned TAIL_MAX_N = 9;

// The arena of a pkf_prover, in elements: the numerator tree and the denominator tree in heap layout, tree[2^d + x] = layer d's
// entry x (2^n elements each, element 0 unused), then the combined table u of the layer being proved (at most 2^(n-1) elements).  The
// n - 1 pks provers hold their own arenas (sumcheck/round.hpp's rule).
inline size_t tree_fes(unsigned n) { return (size_t)1 << n; }
inline size_t combined_fes(unsigned n) { return n > 1 ? (size_t)1 << (n - 1) : 0; }
inline size_t arena_bytes(unsigned n) { return 32 * (2 * tree_fes(n) + combined_fes(n)); }
// the workgroups of a launch whose lanes own `lanes` indices
inline unsigned lanes_grid(size_t lanes) { return pk::gkr::lanes_grid(lanes, PKF_MAX_GRID); }

}  // namespace pkf
