// tree.hip -- the HIP kernels libprovekit_grandproduct.so adds (gfx950): the layers of a product tree, V_d[x] = V_{d+1}[x] *
// V_{d+1}[x + 2^d], written in heap layout (tree[2^d + x] = V_d[x]) for the layered sumchecks that read every one of them.
//
// tree_kernel<S>: S layers per launch.  Reading layer D, a lane owns a low index x < 2^(D-S): it loads the 2^S elements
// in[x + j * 2^(D-S)] (each load coalesced across the lanes), multiplies them pairwise in registers -- element j with element
// j + 2^(S-k) at step k, which are x + j * stride and that plus 2^(D-k) -- and stores every intermediate layer.  So each layer
// is read once and not twice, and S - 1 of every S layers are never read back at all.  The lane's state is 2^S elements of 8 words and
// one product's temporaries.  A product of two values below p is one exact value below p: the bits of a layer depend neither on S nor
// on the grid.
//
// tail_kernel: once the layer to read has at most 2^TAIL_MAX_N entries, one workgroup finishes: its first products come from device
// memory, every layer below from LDS, one barrier per layer and one launch for all of them.  A lane reads its own entry y and entry
// y + half, which no lane writes in that step, and overwrites its own: one barrier per layer is enough.
//
// leaf_kernel<S> (multiset equality): the same descent, but the elements it starts from are made on the way: the w columns' entries
// combined by Horner with beta, subtracted from gamma, stored to the leaf table (the last layer's sumcheck reads it) and kept in
// registers for the first S layers.  S = 0 writes the leaves alone (tables that the tail takes whole).
//
// All stores are ordinary vector stores.
#include <hip/hip_runtime.h>

#include "../fe29.hpp"
#include "kernels.hpp"

using namespace pk;

namespace pkg {

namespace {

struct TableSource {
    const fe* in;
    __device__ __forceinline__ fe operator()(size_t i) const { return fe_load(in + i); }
};
struct LeafSource {
    const fe* col[PKG_MAX_COLUMNS];
    unsigned w;
    fe gamma, beta;
    fe* leaf;
    __device__ __forceinline__ fe operator()(size_t i) const {
        fe acc = fe_zero();
#pragma unroll
        for (int j = PKG_MAX_COLUMNS - 1; j >= 0; j--) {  // w is uniform: col[] keeps constant indices
            if ((unsigned)j >= w) continue;
            const fe a = fe_load(col[j] + i);
            acc = (unsigned)j == w - 1 ? a : fe_add(fe_mulx(acc, beta), a);
        }
        const fe v = fe_sub(gamma, acc);
        fe_store(leaf + i, v);
        return v;
    }
};

// the S layers below layer D (2^D elements, read through src); D >= S
template <int S, class Source>
__device__ __forceinline__ void descend(const Source& src, unsigned D, fe* __restrict__ tree) {
    const size_t stride = (size_t)1 << (D - S);
    for (size_t x = (size_t)blockIdx.x * THREADS + threadIdx.x; x < stride; x += (size_t)gridDim.x * THREADS) {
        fe cur[1 << S];
#pragma unroll
        for (int j = 0; j < (1 << S); j++) cur[j] = src(x + (size_t)j * stride);
#pragma unroll
        for (int k = 1; k <= S; k++) {
            fe* const out = tree + ((size_t)1 << (D - k));
#pragma unroll
            for (int j = 0; j < (1 << (S - k)); j++) {
                cur[j] = fe_mulx(cur[j], cur[j + (1 << (S - k))]);
                fe_store(out + x + (size_t)j * stride, cur[j]);
            }
        }
    }
}

template <int S>
__global__ __launch_bounds__(THREADS) void tree_kernel(const fe* __restrict__ in, unsigned D, fe* __restrict__ tree) {
    descend<S>(TableSource{in}, D, tree);
}
template <int S>
__global__ __launch_bounds__(THREADS) void leaf_kernel(LeafSource src, unsigned D, fe* __restrict__ tree) {
    descend<S>(src, D, tree);
}

// all layers below layer D (1 <= D <= TAIL_MAX_N); one workgroup
__global__ __launch_bounds__(THREADS) void tail_kernel(const fe* __restrict__ in, unsigned D, fe* __restrict__ tree) {
    __shared__ __align__(16) fe layer[1u << (TAIL_MAX_N - 1)];
    unsigned half = 1u << (D - 1);
    for (unsigned y = threadIdx.x; y < half; y += THREADS) {
        const fe prod = fe_mulx(fe_load(in + y), fe_load(in + y + half));
        fe_store(layer + y, prod);
        fe_store(tree + half + y, prod);
    }
    __syncthreads();
    while (half > 1) {  // workgroup-uniform
        half >>= 1;
        for (unsigned y = threadIdx.x; y < half; y += THREADS) {
            const fe prod = fe_mulx(fe_load(layer + y), fe_load(layer + y + half));
            fe_store(layer + y, prod);
            fe_store(tree + half + y, prod);
        }
        __syncthreads();
    }
}

using pk::gkr::dispatch_layers;
using pk::gkr::launched;
bool knobs_ok(unsigned layers, unsigned grid) { return pk::gkr::knobs_ok(layers, grid, PKG_MAX_GRID); }
unsigned step(unsigned D, unsigned layers) { return pk::gkr::step(D, layers, TAIL_MAX_N); }

// every layer below layer D, which `in` holds
int finish(hipStream_t stream, unsigned D, const fe* in, fe* tree, unsigned layers, unsigned grid_or_0) {
    while (unsigned s = step(D, layers)) {
        const unsigned grid = grid_or_0 ? grid_or_0 : lanes_grid((size_t)1 << (D - s));
        dispatch_layers<1>(s, [&](auto S) { tree_kernel<S()><<<grid, THREADS, 0, stream>>>(in, D, tree); });
        D -= s;
        in = tree + ((size_t)1 << D);
    }
    tail_kernel<<<1, THREADS, 0, stream>>>(in, D, tree);
    return launched();
}

}  // namespace

int tree_launch(hipStream_t stream, unsigned n, const uint64_t* d_v, uint64_t* d_tree, unsigned layers_or_0, unsigned grid_or_0) {
    if (n < 1 || n > PKG_MAX_VARS || !d_v || !d_tree || !knobs_ok(layers_or_0, grid_or_0)) return PK_ERR_BAD_ARG;
    return finish(stream, n, (const fe*)d_v, (fe*)d_tree, layers_or_0 ? layers_or_0 : TREE_LAYERS, grid_or_0);
}

int leaf_tree_launch(hipStream_t stream, unsigned n, const Leaves& lv, uint64_t* d_leaf, uint64_t* d_tree, unsigned layers_or_0, unsigned grid_or_0) {
    if (n < 1 || n > PKG_MAX_VARS || !d_leaf || !d_tree || lv.w < 1 || lv.w > PKG_MAX_COLUMNS || !knobs_ok(layers_or_0, grid_or_0)) return PK_ERR_BAD_ARG;
    LeafSource src{};
    for (unsigned j = 0; j < lv.w; j++) {
        if (!lv.col[j]) return PK_ERR_BAD_ARG;
        src.col[j] = (const fe*)lv.col[j];
    }
    src.w = lv.w, src.leaf = (fe*)d_leaf;
    memcpy(src.gamma.v, lv.gamma, 32);
    memcpy(src.beta.v, lv.beta, 32);
    const unsigned layers = layers_or_0 ? layers_or_0 : TREE_LAYERS, s = step(n, layers);
    const unsigned grid = grid_or_0 ? grid_or_0 : lanes_grid((size_t)1 << (n - s));
    fe* const tree = (fe*)d_tree;
    dispatch_layers<0>(s, [&](auto S) { leaf_kernel<S()><<<grid, THREADS, 0, stream>>>(src, n, tree); });
    const unsigned D = n - s;
    return finish(stream, D, s ? tree + ((size_t)1 << D) : (const fe*)d_leaf, tree, layers, grid_or_0);
}

}  // namespace pkg
