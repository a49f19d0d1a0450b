// tree.hip -- the HIP kernels libprovekit_fracsum.so adds (gfx950): the layers of a tree of fractions,
//     p_d[x] = p_{d+1}[x] q_{d+1}[x + 2^d] + p_{d+1}[x + 2^d] q_{d+1}[x],      q_d[x] = q_{d+1}[x] q_{d+1}[x + 2^d],
// written as two trees in heap layout (tree[2^d + x] = layer d's entry x) for the layered sumchecks that read every one of them.
//
// frac_tree_kernel<S, UNIT>: S layers per launch, the grand product's descent on pairs.  Reading layer D, a lane owns a low index
// x < 2^(D-S): it loads the 2^S pairs at x + j * 2^(D-S) (each load coalesced across the lanes), combines them in registers --
// node j with node j + 2^(S-k) at step k, 3 products and 1 add per node -- and stores every intermediate layer of both trees.  So
// each layer is read once and not twice, and S - 1 of every S layers are never read back.  The lane's state is 2^S pairs of 16 words
// and one product's temporaries.  UNIT: the layer read has no numerators, they are all 1: the first step is p = qL + qR, one product
// per node and no numerator loads.  Products and sums of values below p are exact values below p: the bits of a layer depend neither
// on S nor on the grid.
//
// tail_kernel: once the layer to read has at most 2^TAIL_MAX_N entries, one workgroup finishes: its first nodes come from device
// memory, every layer below from LDS (two arrays), one barrier per layer and one launch for all of them.  A lane reads its own
// entry y and entry y + half, which no lane writes in that step, and overwrites its own: one barrier per layer is enough.
//
// lookup_leaf_kernel<S, UNIT>: the same descent, but the denominators it starts from are made on the way: alpha - table[x], stored to
// the leaf table (the last layer's sumcheck reads it) and kept in registers for the first S layers.  The numerators are the
// multiplicities, read in place, or 1 (UNIT).  S = 0 writes the leaves alone (tables that the tail takes whole).
//
// combine_kernel: u = pR + lambda qR (or 1 + lambda qR), the table that keeps lambda out of a layer's coefficients.
//
// All stores are ordinary vector stores.
#include <hip/hip_runtime.h>

#include "../fe29.hpp"
#include "kernels.hpp"

using namespace pk;

namespace pkf {

namespace {

// where a descent's leaves come from: q(i) always, p(i) unless the kernel is instantiated UNIT
struct TableSource {
    const fe* p_in;
    const fe* q_in;
    __device__ __forceinline__ fe p(size_t i) const { return fe_load(p_in + i); }
    __device__ __forceinline__ fe q(size_t i) const { return fe_load(q_in + i); }
};
struct LookupSource {
    const fe* table;
    const fe* m;
    fe alpha;
    fe* leaf;
    __device__ __forceinline__ fe p(size_t i) const { return fe_load(m + i); }
    __device__ __forceinline__ fe q(size_t i) const {
        const fe v = fe_sub(alpha, fe_load(table + i));
        fe_store(leaf + i, v);
        return v;
    }
};

// (pL, qL) + (pR, qR) as fractions, into (pL, qL)
__device__ __forceinline__ void add_fractions(fe& pl, fe& ql, const fe& pr, const fe& qr) {
    pl = fe_add(fe_mulx(pl, qr), fe_mulx(pr, ql));
    ql = fe_mulx(ql, qr);
}
// the same for unit numerators
__device__ __forceinline__ void add_unit_fractions(fe& pl, fe& ql, const fe& qr) {
    pl = fe_add(ql, qr);
    ql = fe_mulx(ql, qr);
}

// the S layers below layer D (2^D nodes, read through src); D >= S
template <int S, bool UNIT, class Source>
__device__ __forceinline__ void descend(const Source& src, unsigned D, fe* __restrict__ ptree, fe* __restrict__ qtree) {
    const size_t stride = (size_t)1 << (D - S);
    for (size_t x = (size_t)blockIdx.x * THREADS + threadIdx.x; x < stride; x += (size_t)gridDim.x * THREADS) {
        fe cp[1 << S], cq[1 << S];
#pragma unroll
        for (int j = 0; j < (1 << S); j++) {
            cq[j] = src.q(x + (size_t)j * stride);
            if (!UNIT) cp[j] = src.p(x + (size_t)j * stride);
        }
#pragma unroll
        for (int k = 1; k <= S; k++) {
            const size_t at = (size_t)1 << (D - k);
#pragma unroll
            for (int j = 0; j < (1 << (S - k)); j++) {
                const int r = j + (1 << (S - k));
                if (UNIT && k == 1)
                    add_unit_fractions(cp[j], cq[j], cq[r]);
                else
                    add_fractions(cp[j], cq[j], cp[r], cq[r]);
                fe_store(ptree + at + x + (size_t)j * stride, cp[j]);
                fe_store(qtree + at + x + (size_t)j * stride, cq[j]);
            }
        }
    }
}

template <int S, bool UNIT>
__global__ __launch_bounds__(THREADS) void frac_tree_kernel(TableSource src, unsigned D, fe* __restrict__ ptree, fe* __restrict__ qtree) {
    descend<S, UNIT>(src, D, ptree, qtree);
}
template <int S, bool UNIT>
__global__ __launch_bounds__(THREADS) void lookup_leaf_kernel(LookupSource src, unsigned D, fe* __restrict__ ptree, fe* __restrict__ qtree) {
    descend<S, UNIT>(src, D, ptree, qtree);
}

// all layers below layer D (1 <= D <= TAIL_MAX_N) of (p_in, q_in); p_in NULL: unit numerators.  One workgroup
__global__ __launch_bounds__(THREADS) void tail_kernel(const fe* __restrict__ p_in, const fe* __restrict__ q_in, unsigned D, fe* __restrict__ ptree,
                                                       fe* __restrict__ qtree) {
    __shared__ __align__(16) fe lp[1u << (TAIL_MAX_N - 1)];
    __shared__ __align__(16) fe lq[1u << (TAIL_MAX_N - 1)];
    unsigned half = 1u << (D - 1);
    for (unsigned y = threadIdx.x; y < half; y += THREADS) {
        fe pl, ql = fe_load(q_in + y);
        const fe qr = fe_load(q_in + y + half);
        if (p_in) {  // workgroup-uniform
            pl = fe_load(p_in + y);
            add_fractions(pl, ql, fe_load(p_in + y + half), qr);
        } else {
            add_unit_fractions(pl, ql, qr);
        }
        fe_store(lp + y, pl), fe_store(lq + y, ql);
        fe_store(ptree + half + y, pl), fe_store(qtree + half + y, ql);
    }
    __syncthreads();
    while (half > 1) {  // workgroup-uniform
        half >>= 1;
        for (unsigned y = threadIdx.x; y < half; y += THREADS) {
            fe pl = fe_load(lp + y), ql = fe_load(lq + y);
            add_fractions(pl, ql, fe_load(lp + y + half), fe_load(lq + y + half));
            fe_store(lp + y, pl), fe_store(lq + y, ql);
            fe_store(ptree + half + y, pl), fe_store(qtree + half + y, ql);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(THREADS) void combine_kernel(size_t count, const fe* __restrict__ pR, const fe* __restrict__ qR, fe lambda, fe* __restrict__ u) {
    const fe one = fe_one();
    for (size_t x = (size_t)blockIdx.x * THREADS + threadIdx.x; x < count; x += (size_t)gridDim.x * THREADS)
        fe_store(u + x, fe_add(pR ? fe_load(pR + x) : one, fe_mulx(lambda, fe_load(qR + x))));
}

using pk::gkr::dispatch_layers;
using pk::gkr::launched;
bool knobs_ok(unsigned layers, unsigned grid) { return pk::gkr::knobs_ok(layers, grid, PKF_MAX_GRID); }
unsigned step(unsigned D, unsigned layers) { return pk::gkr::step(D, layers, TAIL_MAX_N); }

template <bool UNIT>
void tree_step(hipStream_t stream, unsigned s, unsigned grid, const TableSource& src, unsigned D, fe* ptree, fe* qtree) {
    dispatch_layers<1>(s, [&](auto S) { frac_tree_kernel<S(), UNIT><<<grid, THREADS, 0, stream>>>(src, D, ptree, qtree); });
}
template <bool UNIT>
void leaf_step(hipStream_t stream, unsigned s, unsigned grid, const LookupSource& src, unsigned D, fe* ptree, fe* qtree) {
    dispatch_layers<0>(s, [&](auto S) { lookup_leaf_kernel<S(), UNIT><<<grid, THREADS, 0, stream>>>(src, D, ptree, qtree); });
}

// every layer below layer D, which (p_in, q_in) hold; p_in NULL: unit numerators
int finish(hipStream_t stream, unsigned D, const fe* p_in, const fe* q_in, fe* ptree, fe* qtree, unsigned layers, unsigned grid_or_0) {
    while (unsigned s = step(D, layers)) {
        const unsigned grid = grid_or_0 ? grid_or_0 : lanes_grid((size_t)1 << (D - s));
        const TableSource src{p_in, q_in};
        if (p_in)
            tree_step<false>(stream, s, grid, src, D, ptree, qtree);
        else
            tree_step<true>(stream, s, grid, src, D, ptree, qtree);
        D -= s;
        p_in = ptree + ((size_t)1 << D), q_in = qtree + ((size_t)1 << D);
    }
    tail_kernel<<<1, THREADS, 0, stream>>>(p_in, q_in, D, ptree, qtree);
    return launched();
}

}  // namespace

int tree_launch(hipStream_t stream, unsigned n, const uint64_t* d_p_or_null, const uint64_t* d_q, uint64_t* d_ptree, uint64_t* d_qtree, unsigned layers_or_0,
                unsigned grid_or_0) {
    if (n < 1 || n > PKF_MAX_VARS || !d_q || !d_ptree || !d_qtree || !knobs_ok(layers_or_0, grid_or_0)) return PK_ERR_BAD_ARG;
    return finish(stream, n, (const fe*)d_p_or_null, (const fe*)d_q, (fe*)d_ptree, (fe*)d_qtree, layers_or_0 ? layers_or_0 : TREE_LAYERS, grid_or_0);
}

int lookup_leaf_launch(hipStream_t stream, unsigned n, const uint64_t* d_table, const uint64_t* d_m_or_null, const uint64_t alpha[4], uint64_t* d_leaf,
                       uint64_t* d_ptree, uint64_t* d_qtree, unsigned layers_or_0, unsigned grid_or_0) {
    if (n < 1 || n > PKF_MAX_VARS || !d_table || !alpha || !d_leaf || !d_ptree || !d_qtree || !knobs_ok(layers_or_0, grid_or_0)) return PK_ERR_BAD_ARG;
    LookupSource src{};
    src.table = (const fe*)d_table, src.m = (const fe*)d_m_or_null, src.leaf = (fe*)d_leaf;
    memcpy(src.alpha.v, alpha, 32);
    const unsigned layers = layers_or_0 ? layers_or_0 : TREE_LAYERS, s = step(n, layers);
    const unsigned grid = grid_or_0 ? grid_or_0 : lanes_grid((size_t)1 << (n - s));
    fe *const ptree = (fe*)d_ptree, *const qtree = (fe*)d_qtree;
    if (d_m_or_null)
        leaf_step<false>(stream, s, grid, src, n, ptree, qtree);
    else
        leaf_step<true>(stream, s, grid, src, n, ptree, qtree);
    const unsigned D = n - s;
    if (s) return finish(stream, D, ptree + ((size_t)1 << D), qtree + ((size_t)1 << D), ptree, qtree, layers, grid_or_0);
    return finish(stream, D, (const fe*)d_m_or_null, (const fe*)d_leaf, ptree, qtree, layers, grid_or_0);
}

int combine_launch(hipStream_t stream, size_t count, const uint64_t* d_pR_or_null, const uint64_t* d_qR, const uint64_t lambda[4], uint64_t* d_u,
                   unsigned grid_or_0) {
    if (!count || !d_qR || !lambda || !d_u || grid_or_0 > PKF_MAX_GRID) return PK_ERR_BAD_ARG;
    fe lam;
    memcpy(lam.v, lambda, 32);
    combine_kernel<<<grid_or_0 ? grid_or_0 : lanes_grid(count), THREADS, 0, stream>>>(count, (const fe*)d_pR_or_null, (const fe*)d_qR, lam, (fe*)d_u);
    return launched();
}

}  // namespace pkf
