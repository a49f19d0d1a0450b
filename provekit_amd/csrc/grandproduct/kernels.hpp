// kernels.hpp -- the launches of tree.hip, for prover.cpp.  Everything is enqueued on `stream`; grids are 1 .. PKG_MAX_GRID
// workgroups of 256; the bits of every layer depend neither on the grid nor on the layers per launch.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.hpp"

namespace pkg {

// The columns of one side and the two challenges of the leaves, leaf[x] = gamma - sum_j beta^j col[j][x]
struct Leaves {
    const uint64_t* col[PKG_MAX_COLUMNS];
    unsigned w;
    uint64_t gamma[4], beta[4];
};

// All layers V_{n-1} .. V_0 of d_v (2^n elements) into d_tree in heap layout (2^n elements; element 0 is not written): tree_kernel
// takes `layers` (1 .. TREE_MAX_LAYERS; 0: TREE_LAYERS) layers per launch while the layer it reads has more than 2^TAIL_MAX_N entries,
// tail_kernel finishes in one launch.  grid_or_0: the workgroups of every tree_kernel launch; 0: one lane per low index.
int tree_launch(hipStream_t stream, unsigned n, const uint64_t* d_v, uint64_t* d_tree, unsigned layers_or_0, unsigned grid_or_0);

// The same from columns: leaf_kernel writes the leaf table d_leaf (2^n elements) AND the first layers of its tree in one pass (the
// leaves are never re-read for the tree); then as tree_launch.
int leaf_tree_launch(hipStream_t stream, unsigned n, const Leaves& lv, uint64_t* d_leaf, uint64_t* d_tree, unsigned layers_or_0, unsigned grid_or_0);

}  // namespace pkg
