// launch.hpp -- the host side of a launch that grandproduct/tree.hip and fracsum/tree.hip share: the workgroup's width, how many
// layers a launch takes, the grid rule, the check of a prover's knobs and the step from the run-time number of layers to the kernel's
// template argument.  The device bodies are each library's own (EXPERIMENTS.md, round 31: merging the two descents changes the
// fraction kernels' registers).  TAIL_MAX_N is each library's too (fracsum/layout.hpp says why they differ) and comes in as an
// argument.  Host only.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <type_traits>

#include "../../../include/provekit_hip.h"

namespace pk::gkr {

constexpr unsigned THREADS = 256;
// Layers per launch of a tree kernel: a lane holds 2^S nodes and stores every intermediate layer.  1, 2 or 3; a prover's own value is a
// test and benchmark knob (tools/probes/).
constexpr unsigned TREE_MAX_LAYERS = 3;
constexpr unsigned TREE_LAYERS = 2;

// the workgroups of a launch whose lanes own `lanes` indices
inline unsigned lanes_grid(size_t lanes, unsigned max_grid) {
    const size_t need = (lanes + THREADS - 1) / THREADS;
    return (unsigned)(need < 1 ? 1 : need > max_grid ? max_grid : need);
}
// how many layers the next launch takes when it reads layer D; 0: the tail takes the rest
inline unsigned step(unsigned D, unsigned layers, unsigned tail_max_n) { return D > tail_max_n ? (layers < D - tail_max_n ? layers : D - tail_max_n) : 0; }
inline bool knobs_ok(unsigned layers, unsigned grid, unsigned max_grid) { return layers <= TREE_MAX_LAYERS && grid <= max_grid; }
inline int launched() { return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP; }

// f(std::integral_constant<int, s>{}) for the run-time s in LOWEST .. 3: the kernels take the layers of a launch as a template argument.
// LOWEST is 1 for a tree kernel and 0 for a leaf kernel (no layer: the leaves alone); nothing below it is instantiated.
template <int LOWEST, class F>
void dispatch_layers(unsigned s, F&& f) {
    static_assert(LOWEST == 0 || LOWEST == 1, "a launch takes 0 .. 3 or 1 .. 3 layers");
    if constexpr (LOWEST == 0) {
        if (s == 0) return f(std::integral_constant<int, 0>{});
    }
    if (s == 1) return f(std::integral_constant<int, 1>{});
    if (s == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 3>{});
}

}  // namespace pk::gkr
