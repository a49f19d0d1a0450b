// kernels.hpp -- the launches of tree.hip, for prover.cpp.  Everything is enqueued on `stream`; grids are 1 .. PKF_MAX_GRID
// workgroups of 256; the bits of every layer depend neither on the grid nor on the layers per launch.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.hpp"

namespace pkf {

// All layers n-1 .. 0 of the leaves (d_p, d_q) (2^n elements each; d_p NULL: every numerator is 1) into d_ptree and d_qtree in heap
// layout (2^n elements each; element 0 is not written): frac_tree_kernel takes `layers` (1 .. TREE_MAX_LAYERS; 0: TREE_LAYERS) layers
// per launch while the layer it reads has more than 2^TAIL_MAX_N entries, tail_kernel finishes in one launch.  grid_or_0: the
// workgroups of every frac_tree_kernel launch; 0: one lane per low index.
int tree_launch(hipStream_t stream, unsigned n, const uint64_t* d_p_or_null, const uint64_t* d_q, uint64_t* d_ptree, uint64_t* d_qtree, unsigned layers_or_0,
                unsigned grid_or_0);

// The same for a side of the lookup: lookup_leaf_kernel writes the leaf table d_leaf[x] = alpha - d_table[x] (2^n elements) AND the
// first layers of both trees in one pass (the leaves are never re-read for the tree); the numerators are d_m, read in place, or 1
// where d_m is NULL; then as tree_launch.
int lookup_leaf_launch(hipStream_t stream, unsigned n, const uint64_t* d_table, const uint64_t* d_m_or_null, const uint64_t alpha[4], uint64_t* d_leaf,
                       uint64_t* d_ptree, uint64_t* d_qtree, unsigned layers_or_0, unsigned grid_or_0);

// d_u[x] = d_pR[x] + lambda d_qR[x] for x < count (d_pR NULL: 1 + lambda d_qR[x]): one coalesced pass.  grid_or_0 as above.
int combine_launch(hipStream_t stream, size_t count, const uint64_t* d_pR_or_null, const uint64_t* d_qR, const uint64_t lambda[4], uint64_t* d_u,
                   unsigned grid_or_0);

}  // namespace pkf
