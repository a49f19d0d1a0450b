// mle.hip -- multilinear-extension kernels of the Spartan sumcheck and the WHIR rounds
// (SURVEY 8a rows T1, S2, S3, S5, E1, W1, W2, W3).
//
// All of these stream 32-byte field elements with a handful of modular multiplies per
// element, so each is laid out for coalesced 32 B/lane access, keeps its arrays resident
// in HBM across rounds, and returns only the 3-4 field elements the Fiat-Shamir
// transcript needs per round (grid reduction in reduce.hpp).
// memory- / latency-bound kernels: their wavefronts issue ahead of the ALU-bound hash / NTT / grinder kernels they share SIMDs with
#define PK_BASE_PRIO 2
#include "internal.hpp"
#include "fe29.hpp"
#include "reduce.hpp"

using namespace pk;

namespace {

struct fe_arg {
    u32 v[8];
};
__device__ __forceinline__ fe from_arg(const fe_arg& a) {
    fe r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = a.v[i];
    return r;
}
inline fe_arg to_arg(const uint64_t* h) {
    fe_arg a;
    memcpy(a.v, h, 32);
    return a;
}

__device__ __forceinline__ fe lds_get(const uint4* lo, const uint4* hi, int i) {
    uint4 l = lo[i], h = hi[i];
    fe x;
    x.v[0] = l.x; x.v[1] = l.y; x.v[2] = l.z; x.v[3] = l.w;
    x.v[4] = h.x; x.v[5] = h.y; x.v[6] = h.z; x.v[7] = h.w;
    return x;
}
__device__ __forceinline__ void lds_put(uint4* lo, uint4* hi, int i, const fe& x) {
    lo[i] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
    hi[i] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}

// per-limb select: no divergent branch where the lanes of a wavefront differ in `pick`
__device__ __forceinline__ fe fe_select(bool pick, const fe& x, const fe& y) {
    fe r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = pick ? x.v[i] : y.v[i];
    return r;
}
// a lane's contribution to a grid reduction of K sums when it holds a term of sum `slot` only: t in acc[slot], zero elsewhere
// (slot by reference: by value the two-sum quadratic kernel comes out one compare shorter than the loops written out in it gave)
template <int K>
__device__ __forceinline__ void acc_only(fe (&acc)[K], const unsigned& slot, const fe& t) {
#pragma unroll
    for (int q = 0; q < K; q++)
#pragma unroll
        for (int i = 0; i < 8; i++) acc[q].v[i] = slot == (unsigned)q ? t.v[i] : 0u;
}

// ---------------------------------------------------------------- T1: evals <-> coeffs
// EvaluationsList::to_coeffs (call sites provekit/prover/src/whir_r1cs.rs:195,198): for every
// variable (index bit) h: v[i | h] -= v[i].  SUB=false gives the inverse (to_evals).
// low kernel: bits [0, LOGT) on a contiguous tile of 2^LOGT elements held in LDS.
template <bool SUB>
__global__ __launch_bounds__(256) void wavelet_low_kernel(const fe* src, fe* data, unsigned logt) {
    PK_LATENCY_PRIO();
    extern __shared__ uint4 lds[];
    const int T = 1 << logt;
    uint4* lo = lds;
    uint4* hi = lds + T;
    fe* base = data + (size_t)blockIdx.x * T;
    const fe* sbase = src + (size_t)blockIdx.x * T;  // src == data for the in-place form
    for (int e = threadIdx.x; e < T; e += 256) {
        const uint4* q = reinterpret_cast<const uint4*>(sbase + e);
        lo[e] = q[0];
        hi[e] = q[1];
    }
    __syncthreads();
    for (unsigned s = 0; s < logt; s++) {
        const int h = 1 << s;
        for (int t = threadIdx.x; t < T / 2; t += 256) {
            int pos = t & (h - 1);
            int i0 = ((t - pos) << 1) + pos, i1 = i0 + h;
            fe a = lds_get(lo, hi, i0), b = lds_get(lo, hi, i1);
            lds_put(lo, hi, i1, SUB ? fe_sub(b, a) : fe_add(b, a));
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < T; e += 256) {
        uint4* q = reinterpret_cast<uint4*>(base + e);
        q[0] = lo[e];
        q[1] = hi[e];
    }
}
// high kernel: bits [s, s+logr): element index = u*2^(s+logr) + r*2^s + v; tile = [2^logr][4 adjacent v]
template <bool SUB, int BT>
__global__ __launch_bounds__(256) void wavelet_high_kernel(fe* __restrict__ data, unsigned s, unsigned logr) {
    PK_LATENCY_PRIO();
    extern __shared__ uint4 lds[];
    const int R = 1 << logr;
    const int TILE = R * BT;
    uint4* lo = lds;
    uint4* hi = lds + TILE;
    const size_t vblocks = ((size_t)1 << s) / BT;
    const size_t u = blockIdx.x / vblocks, vb = blockIdx.x % vblocks;
    fe* base = data + (u << (s + logr)) + vb * BT;
    for (int e = threadIdx.x; e < TILE; e += 256) {
        int b = e % BT, r = e / BT;
        const uint4* q = reinterpret_cast<const uint4*>(base + ((size_t)r << s) + b);
        lo[e] = q[0];
        hi[e] = q[1];
    }
    __syncthreads();
    for (unsigned st = 0; st < logr; st++) {
        const int h = 1 << st;
        for (int t = threadIdx.x; t < (R / 2) * BT; t += 256) {
            int b = t % BT, j = t / BT;
            int pos = j & (h - 1);
            int i0 = ((j - pos) << 1) + pos, i1 = i0 + h;
            fe a = lds_get(lo, hi, i0 * BT + b), c = lds_get(lo, hi, i1 * BT + b);
            lds_put(lo, hi, i1 * BT + b, SUB ? fe_sub(c, a) : fe_add(c, a));
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < TILE; e += 256) {
        int b = e % BT, r = e / BT;
        uint4* q = reinterpret_cast<uint4*>(base + ((size_t)r << s) + b);
        q[0] = lo[e];
        q[1] = hi[e];
    }
}

// The first to_coeffs sweep of a committed polynomial that does not exist yet (prover.hip batch_commit_compute): the tile is assembled
// where it is first read.  Element i of the table is witness[i] for i < n_wit, zero up to rand_from, and from there element i - rand_from
// of the draw `stream` of n_draw elements (rng_core.hpp).  Each element goes to the evaluation table (kept whole for the batch
// combination and the weighted sums) and into the tile, whose sweep then runs as wavelet_low_kernel's.  blockIdx.y picks the table.
struct gen_table {
    const fe* wit;
    size_t n_wit, rand_from, n_draw;
    u32 stream;
    fe* evals;
    fe* coeffs;
};
__global__ __launch_bounds__(256) void wavelet_low_generated_kernel(gen_table ta, gen_table tb, RngKey key, unsigned logt) {
    PK_LATENCY_PRIO();
    extern __shared__ uint4 lds[];
    const gen_table& S = blockIdx.y ? tb : ta;
    const int T = 1 << logt;
    uint4* lo = lds;
    uint4* hi = lds + T;
    const size_t t0 = (size_t)blockIdx.x * T;
    for (int e = threadIdx.x; e < T && t0 + e < S.rand_from; e += 256) {  // a tile may straddle n_wit: per element
        uint4 a = make_uint4(0, 0, 0, 0), b = a;
        if (t0 + e < S.n_wit) {
            const uint4* q = reinterpret_cast<const uint4*>(S.wit + t0 + e);
            a = q[0];
            b = q[1];
        }
        lo[e] = a;
        hi[e] = b;
        uint4* o = reinterpret_cast<uint4*>(S.evals + t0 + e);
        o[0] = a;
        o[1] = b;
    }
    if (t0 + T > S.rand_from) {  // rand_from is 0 or a power of two, t0 a multiple of T: the drawn part starts at an even element of the draw
        const size_t d0 = (t0 > S.rand_from ? t0 : S.rand_from) - S.rand_from, d1 = t0 + T - S.rand_from;
        fe* ev = S.evals + S.rand_from;
        const size_t shift = S.rand_from - t0;  // tile slot of draw element i: i + rand_from - t0 (mod 2^64 where t0 > rand_from)
        rng_draw_pairs(key, S.stream, d0 / 2 + threadIdx.x, 256, (d1 + 1) / 2, S.n_draw, [&](size_t i, const fe& x) {
            fe_store(ev + i, x);
            lds_put(lo, hi, (int)(i + shift), x);
        });
    }
    __syncthreads();
    for (unsigned s = 0; s < logt; s++) {
        const int h = 1 << s;
        for (int t = threadIdx.x; t < T / 2; t += 256) {
            int pos = t & (h - 1);
            int i0 = ((t - pos) << 1) + pos, i1 = i0 + h;
            fe a = lds_get(lo, hi, i0), b = lds_get(lo, hi, i1);
            lds_put(lo, hi, i1, fe_sub(b, a));
        }
        __syncthreads();
    }
    fe* base = S.coeffs + t0;
    for (int e = threadIdx.x; e < T; e += 256) {
        uint4* q = reinterpret_cast<uint4*>(base + e);
        q[0] = lo[e];
        q[1] = hi[e];
    }
}

inline unsigned wavelet_low_bits(unsigned n_vars) { return n_vars < 11 ? n_vars : 11; }
// the sweeps over the index bits [s, n_vars), in place
template <bool SUB>
int wavelet_high_sweeps(pk_ctx* ctx, fe* D, unsigned s, unsigned n_vars) {
    PK_HIP(ctx, hipFuncSetAttribute((const void*)wavelet_high_kernel<SUB, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, 1 << 16));
    PK_HIP(ctx, hipFuncSetAttribute((const void*)wavelet_high_kernel<SUB, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 1 << 16));
    while (s < n_vars) {
        // up to 10 index bits per sweep (2^10 rows x 2 adjacent elements = 64 KiB of LDS), 9 with 4-element rows otherwise
        unsigned left = n_vars - s;
        if (left == 10 && s >= 1) {
            size_t tiles = ((size_t)1 << (n_vars - 10)) / 2;
            wavelet_high_kernel<SUB, 2><<<(unsigned)tiles, 256, ((size_t)2 << 10) * 2 * 16, ctx->stream>>>(D, s, 10);
            s += 10;
        } else {
            unsigned logr = left < 9 ? left : 9;
            size_t tiles = ((size_t)1 << (n_vars - logr)) / 4;
            wavelet_high_kernel<SUB, 4><<<(unsigned)tiles, 256, ((size_t)2 << logr) * 4 * 16, ctx->stream>>>(D, s, logr);
            s += logr;
        }
    }
    PK_LAUNCH_CHECK(ctx);
    return PK_OK;
}

// d_src == nullptr: in place; otherwise the first sweep reads d_src and writes d_data (saves a 32 B/element copy)
template <bool SUB>
int wavelet(pk_ctx* ctx, const uint64_t* d_src, uint64_t* d_data, unsigned n_vars) {
    PK_REQUIRE(ctx, d_data, "null pointer");
    PK_REQUIRE(ctx, n_vars <= 30, "too many variables");
    fe* D = (fe*)d_data;
    const fe* S = d_src ? (const fe*)d_src : D;
    if (n_vars == 0) {
        if (d_src && d_src != d_data) PK_HIP(ctx, hipMemcpyAsync(D, S, 32, hipMemcpyDeviceToDevice, ctx->stream));
        return PK_OK;
    }
    ProfScope prof(ctx, SUB ? "to_coeffs" : "to_evals");
    const unsigned logt = wavelet_low_bits(n_vars);
    size_t lds = ((size_t)2 << logt) * 16;
    PK_HIP(ctx, hipFuncSetAttribute((const void*)wavelet_low_kernel<SUB>, hipFuncAttributeMaxDynamicSharedMemorySize, 1 << 16));
    wavelet_low_kernel<SUB><<<(unsigned)((size_t)1 << (n_vars - logt)), 256, lds, ctx->stream>>>(S, D, logt);
    return wavelet_high_sweeps<SUB>(ctx, D, logt, n_vars);
}

// ---------------------------------------------------------------- S2 / W2: eq tables
// eval_eq (provekit/common/src/utils/sumcheck.rs:146-171): out[i] += scalar * prod_j (bit_j(i) ? x_j : 1-x_j),
// variable 0 <-> most significant index bit.  eq(x, i) = eq_hi(x[0..nhi), i >> nlo) * eq_lo(x[nhi..n), i & mask):
// one block builds each half table (level by level, in global memory), then one streaming kernel
// accumulates all q points into w -- one multiply per (point, element).
// tables layout: [pt][ 2^nhi hi entries | 2^nlo lo entries ]
__global__ __launch_bounds__(256) void eq_half_tables_kernel(const fe* __restrict__ points, const fe* __restrict__ scales,
                                                             unsigned n_vars, unsigned nhi, unsigned nlo, fe* __restrict__ tables) {
    PK_LATENCY_PRIO();
    // points / scales sit in pinned host memory (the mailbox): fetch this half's <= 15 coordinates in one go
    __shared__ uint4 xs[2 * 16];
    const unsigned pt = blockIdx.x, half = blockIdx.y;
    const size_t per_pt = ((size_t)1 << nhi) + ((size_t)1 << nlo);
    fe* T = tables + pt * per_pt + (half ? ((size_t)1 << nhi) : 0);
    const fe* x = points + (size_t)pt * n_vars + (half ? nhi : 0);
    const unsigned nv = half ? nlo : nhi;
    if (threadIdx.x < nv) lds_put(xs, xs + 16, threadIdx.x, fe_load(x + threadIdx.x));
    if (threadIdx.x == 32) fe_store(T, half ? fe_one() : fe_load(scales + pt));
    __threadfence_block();
    __syncthreads();
    // Level l appends variable nv-1-l as index bit l, so the last variable is the LSB and variable 0
    // ends up as the MSB, as eval_eq's recursion orders it: T[h+i] = x*T[i] (s1), T[i] -= that (s0).
    for (unsigned l = 0; l < nv; l++) {
        const size_t h = (size_t)1 << l;
        fe xv = lds_get(xs, xs + 16, nv - 1 - l);
        for (size_t i = threadIdx.x; i < h; i += 256) {
            fe t = fe_load(T + i);
            fe up = fe_mulx(t, xv);  // s1 = s * x
            fe_store(T + h + i, up);
            fe_store(T + i, fe_sub(t, up));  // s0 = s - s1
        }
        __threadfence_block();
        __syncthreads();
    }
}
// Two adjacent outputs per lane (they share the high half-table entry) and the q products of each output summed with one
// Montgomery reduction per DOT29_GROUP terms (fe29.hpp dot29): ~100 multiply-adds per (point, element) instead of 162+.
__global__ __launch_bounds__(256) void eq_accumulate_kernel(fe* __restrict__ w, size_t n, unsigned nhi, unsigned nlo, unsigned q,
                                                            const fe* __restrict__ tables, int overwrite) {
    PK_LATENCY_PRIO();
    const size_t per_pt = ((size_t)1 << nhi) + ((size_t)1 << nlo);
    const size_t mask = ((size_t)1 << nlo) - 1;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    if (nlo == 0) {  // a single low entry per point: one output per lane
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
            dot29 d;
            dot29_init(d);
            const fe* T = tables;
            for (unsigned pt = 0; pt < q; pt++, T += per_pt)
                dot29_add(d, unpack29<0>(fe_load(T + (i >> nlo))), unpack29<5>(fe_load(T + ((size_t)1 << nhi) + (i & mask))));
            fe r = dot29_result(d);
            fe_store(w + i, overwrite ? r : fe_add(fe_load(w + i), r));
        }
        return;
    }
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n / 2; j += stride) {
        const size_t i = 2 * j;  // i and i + 1 differ in the lowest index bit only: same high entry
        dot29 d0, d1;
        dot29_init(d0);
        dot29_init(d1);
        const fe* T = tables;
        for (unsigned pt = 0; pt < q; pt++, T += per_pt) {
            const fe29 h = unpack29<0>(fe_load(T + (i >> nlo)));
            const fe* lo = T + ((size_t)1 << nhi) + (i & mask);
            dot29_add(d0, h, unpack29<5>(fe_load(lo)));
            dot29_add(d1, h, unpack29<5>(fe_load(lo + 1)));
        }
        fe r0 = dot29_result(d0), r1 = dot29_result(d1);
        fe_store(w + i, overwrite ? r0 : fe_add(fe_load(w + i), r0));
        fe_store(w + i + 1, overwrite ? r1 : fe_add(fe_load(w + i + 1), r1));
    }
}

// ---------------------------------------------------------------- S3: cubic sumcheck round
// sumcheck_fold_map_reduce::<4,3> (provekit/common/src/utils/sumcheck.rs:16-104) with the map of
// provekit/prover/src/whir_r1cs.rs:284-291.  The weight of a pair comes in one of two ways:
//   CubicWeight::EqArray: a fourth array, folded with a, b, c; it enters the evaluations as eq0, eq1 and the sums are f(0), f(-1), f_inf;
//   CubicWeight::Level:   one read-only entry E_i[i] per pair ("without the folded eq array" below); the sums are Q(0), Q(-1), Q_inf.
template <CubicWeight W>
using weight_elem = std::conditional_t<W == CubicWeight::Level, const fe, fe>;

// A lane per pair.  The workgroup size is read through the builtin: blockDim.x in a function that is inlined into the kernel is not
// folded to the dispatch's group size (that needs the kernel's own uniform-work-group-size attribute) and costs a vector load.
template <bool FOLD, CubicWeight W>
__device__ __forceinline__ void cubic_round_wide(fe* __restrict__ a, fe* __restrict__ b, fe* __restrict__ c, weight_elem<W>* __restrict__ wt, size_t len,
                                                 fe_arg fold_arg, gate_args gate, red_out red) {
    constexpr bool LEVEL = W == CubicWeight::Level;
    constexpr int NA = LEVEL ? 3 : 4;  // arrays that fold
    PK_LATENCY_PRIO();
    const fe alpha = (FOLD && gate.host) ? gate_wait(gate) : from_arg(fold_arg);
    const size_t npairs = FOLD ? len / 4 : len / 2;
    const size_t off = npairs;          // partner of i is i + off (quarter 1 after folding, or the upper half)
    const size_t foff = len / 2;        // fold partner: p2 = p0 + len/2
    fe acc[3] = {fe_zero(), fe_zero(), fe_zero()};
    const size_t stride = (size_t)gridDim.x * __builtin_amdgcn_workgroup_size_x();
    for (size_t i = (size_t)blockIdx.x * __builtin_amdgcn_workgroup_size_x() + threadIdx.x; i < npairs; i += stride) {
        fe v[NA][2];
        fe* arr[4] = {a, b, c, nullptr};
        if constexpr (!LEVEL) arr[3] = wt;
#pragma unroll
        for (int k = 0; k < NA; k++) {
            fe x0 = fe_load(arr[k] + i), x1 = fe_load(arr[k] + i + off);
            if (FOLD) {  // sumcheck.rs:95-96: p0 += fold*(p2-p0); p1 += fold*(p3-p1)
                fe x2 = fe_load(arr[k] + i + foff), x3 = fe_load(arr[k] + i + off + foff);
                x0 = fe_fold(x0, x2, alpha);
                x1 = fe_fold(x1, x3, alpha);
                fe_store(arr[k] + i, x0);
                fe_store(arr[k] + i + off, x1);
            }
            v[k][0] = x0;
            v[k][1] = x1;
        }
        const fe &a0 = v[0][0], &a1 = v[0][1], &b0 = v[1][0], &b1 = v[1][1], &c0 = v[2][0], &c1 = v[2][1];
        fe e0, e1;  // Level: e0 = E_i[i] weighs all three sums
        if constexpr (LEVEL) {
            e0 = fe_load(wt + i);
        } else {
            e0 = v[NA - 1][0];
            e1 = v[NA - 1][1];
        }
        // f0 = eq0 * (a0*b0 - c0)
        acc[0] = fe_add(acc[0], fe_mulx(e0, fe_sub(fe_mulx(a0, b0), c0)));
        // f(-1) = (2eq0-eq1) * ((2a0-a1)(2b0-b1) - (2c0-c1))
        fe ta = fe_sub(fe_dbl(a0), a1), tb = fe_sub(fe_dbl(b0), b1), tc = fe_sub(fe_dbl(c0), c1), te = e0;
        if constexpr (!LEVEL) te = fe_sub(fe_dbl(e0), e1);
        acc[1] = fe_add(acc[1], fe_mulx(te, fe_sub(fe_mulx(ta, tb), tc)));
        // f_inf = (eq1-eq0)(a1-a0)(b1-b0)
        if constexpr (LEVEL) acc[2] = fe_add(acc[2], fe_mulx(e0, fe_mulx(fe_sub(a1, a0), fe_sub(b1, b0))));
        else acc[2] = fe_add(acc[2], fe_mulx(fe_mulx(fe_sub(e1, e0), fe_sub(a1, a0)), fe_sub(b1, b0)));
    }
    grid_finish_fe<3>(acc, red);
}
template <bool FOLD>
__global__ __launch_bounds__(RED_THREADS) void sumcheck_cubic_kernel(fe* __restrict__ a, fe* __restrict__ b, fe* __restrict__ c,
                                                                     fe* __restrict__ eq, size_t len, fe_arg fold_arg, gate_args gate, red_out red) {
    cubic_round_wide<FOLD, CubicWeight::EqArray>(a, b, c, eq, len, fold_arg, gate, red);
}

// ---------------------------------------------------------------- W3: quadratic sumcheck round
// adjacent pairs (2i, 2i+1): h(0)=sum f0 w0, h(1)=sum f1 w1, h(2)=sum (2f1-f0)(2w1-w0)
// (recursive-verifier/app/circuit/whir_utilities.go:102-125; utilities.go:148-154).
// FOLD: first v'[i] = v[2i] + r (v[2i+1]-v[2i]) written to the *_out arrays (out-of-place).
// NS = 3: h(0), h(1), h(2).  NS = 2: h(0), h(2) only -- a caller that holds the round's claim h(0) + h(1) (the prover's own
// sumcheck loop does: it is what the verifier checks) takes h(1) = claim - h(0) on the host; one product per pair less.
template <bool FOLD, int NS>
__global__ __launch_bounds__(RED_THREADS) void sumcheck_quadratic_kernel(const fe* __restrict__ f, const fe* __restrict__ w,
                                                                         size_t out_len, fe_arg fold_arg, gate_args gate, fe* __restrict__ f_out,
                                                                         fe* __restrict__ w_out, red_out red) {
    PK_LATENCY_PRIO();
    static_assert(NS == 2 || NS == 3, "two or three sums");
    const fe r = (FOLD && gate.host) ? gate_wait(gate) : from_arg(fold_arg);
    fe acc[NS];
#pragma unroll
    for (int q = 0; q < NS; q++) acc[q] = fe_zero();
    const size_t npairs = out_len / 2;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npairs; i += stride) {
        fe f0, f1, w0, w1;
        if (FOLD) {
            fe x0 = fe_load(f + 4 * i), x1 = fe_load(f + 4 * i + 1), x2 = fe_load(f + 4 * i + 2), x3 = fe_load(f + 4 * i + 3);
            f0 = fe_fold(x0, x1, r);
            f1 = fe_fold(x2, x3, r);
            fe y0 = fe_load(w + 4 * i), y1 = fe_load(w + 4 * i + 1), y2 = fe_load(w + 4 * i + 2), y3 = fe_load(w + 4 * i + 3);
            w0 = fe_fold(y0, y1, r);
            w1 = fe_fold(y2, y3, r);
            fe_store(f_out + 2 * i, f0);
            fe_store(f_out + 2 * i + 1, f1);
            fe_store(w_out + 2 * i, w0);
            fe_store(w_out + 2 * i + 1, w1);
        } else {
            f0 = fe_load(f + 2 * i);
            f1 = fe_load(f + 2 * i + 1);
            w0 = fe_load(w + 2 * i);
            w1 = fe_load(w + 2 * i + 1);
        }
        acc[0] = fe_add(acc[0], fe_mulx(f0, w0));
        if (NS == 3) acc[1] = fe_add(acc[1], fe_mulx(f1, w1));
        acc[NS - 1] = fe_add(acc[NS - 1], fe_mulx(fe_sub(fe_dbl(f1), f0), fe_sub(fe_dbl(w1), w0)));
    }
    grid_finish_fe<NS>(acc, red);
}
// The round-0 launch of a quadratic sumcheck whose tables are still to be formed: one lane per adjacent pair (2i, 2i + 1) -- the pair the
// round sums over, and the pair eq_accumulate_kernel shares a high half-table entry across -- makes the pair's entries of p and w where
// they are first read, stores them and adds the pair's terms to the round's sums.  What is formed is chosen by flags; one body:
//   COMBINE    p = e0 + beta e1 (lincomb_kernel's expression), stored; else p stands as it is and is only read
//   q points   w = (overwrite ? 0 : w) + sum_j hi_j lo_j over the half tables (eq_accumulate_kernel's pair loop), stored
//   NR rows    below row_len, w += g_0 r_0 (axpy_kernel's expression) or g_0 r_0 + g_1 r_1 + g_2 r_2 (axpy3_kernel's)
// Every step gives the reduced representative, so p, w and the sums carry the bits the launches it replaces leave: eq_accumulate_kernel,
// axpy_kernel / axpy3_kernel, lincomb_kernel and sumcheck_quadratic_kernel<false, NS>.  n >= 2 entries, so nlo >= 1.
struct fe3_arg {
    fe_arg g[3];
};
struct first_rows {
    const fe* rows;  // row k at rows + k * stride
    size_t stride, len;
    fe3_arg g;
};
template <int NR>
__device__ __forceinline__ fe first_rows_term(const first_rows& R, size_t i) {
    static_assert(NR == 1 || NR == 3, "one row or three");
    if constexpr (NR == 1) {
        return fe_mulx(from_arg(R.g.g[0]), fe_load(R.rows + i));
    } else {
        dot29 d;
        dot29_init(d);
#pragma unroll
        for (int k = 0; k < 3; k++) dot29_add(d, unpack29<0>(fe_load(R.rows + k * R.stride + i)), unpack29<5>(from_arg(R.g.g[k])));
        return dot29_result(d);
    }
}
template <bool COMBINE, int NR, int NS>
__global__ __launch_bounds__(RED_THREADS) void opening_first_kernel(const fe* __restrict__ e0, const fe* __restrict__ e1, fe_arg beta_arg,
                                                                    fe* __restrict__ p, fe* __restrict__ w, size_t n, unsigned nhi, unsigned nlo,
                                                                    unsigned q, const fe* __restrict__ tables, int overwrite, first_rows R, red_out red) {
    PK_LATENCY_PRIO();
    static_assert(NS == 2 || NS == 3, "two or three sums");
    const size_t per_pt = ((size_t)1 << nhi) + ((size_t)1 << nlo);
    const size_t mask = ((size_t)1 << nlo) - 1;
    fe acc[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) acc[s] = fe_zero();
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n / 2; j += stride) {
        const size_t i = 2 * j;
        dot29 d0, d1;
        dot29_init(d0);
        dot29_init(d1);
        const fe* T = tables;
        for (unsigned pt = 0; pt < q; pt++, T += per_pt) {
            const fe29 h = unpack29<0>(fe_load(T + (i >> nlo)));
            const fe* lo = T + ((size_t)1 << nhi) + (i & mask);
            dot29_add(d0, h, unpack29<5>(fe_load(lo)));
            dot29_add(d1, h, unpack29<5>(fe_load(lo + 1)));
        }
        fe w0 = dot29_result(d0), w1 = dot29_result(d1);
        if (!overwrite) {
            w0 = fe_add(fe_load(w + i), w0);
            w1 = fe_add(fe_load(w + i + 1), w1);
        }
        if constexpr (NR > 0) {  // a pair may straddle the rows' end
            if (i < R.len) w0 = fe_add(w0, first_rows_term<NR>(R, i));
            if (i + 1 < R.len) w1 = fe_add(w1, first_rows_term<NR>(R, i + 1));
        }
        fe_store(w + i, w0);
        fe_store(w + i + 1, w1);
        fe f0, f1;
        if constexpr (COMBINE) {
            const fe beta = from_arg(beta_arg);
            f0 = fe_add(fe_load(e0 + i), fe_mulx(beta, fe_load(e1 + i)));
            f1 = fe_add(fe_load(e0 + i + 1), fe_mulx(beta, fe_load(e1 + i + 1)));
            fe_store(p + i, f0);
            fe_store(p + i + 1, f1);
        } else {
            f0 = fe_load(p + i);
            f1 = fe_load(p + i + 1);
        }
        acc[0] = fe_add(acc[0], fe_mulx(f0, w0));
        if (NS == 3) acc[1] = fe_add(acc[1], fe_mulx(f1, w1));
        acc[NS - 1] = fe_add(acc[NS - 1], fe_mulx(fe_sub(fe_dbl(f1), f0), fe_sub(fe_dbl(w1), w0)));
    }
    grid_finish_fe<NS>(acc, red);
}

// ---- small rounds: the work of ONE pair spread over several lanes ------------------------------------------------------
// Late sumcheck rounds have a handful of pairs; with a lane per pair the round is a chain of 16 (cubic, folding) or 7
// (quadratic, folding) dependent modular multiplications on one lane of one wavefront -- ~1 us each -- and the kernel holds a
// hardware queue for that long.  Here the independent products of a pair go to neighbouring lanes (8 resp. 4 per pair),
// the folded values are exchanged through LDS, and three lanes form the three evaluations: 3 resp. 2 multiplications deep.
// Same arithmetic, same order of the (exact) field operations per value: results are bit-identical to the wide kernels.
constexpr size_t SMALL_ROUND_PAIRS = 16384;
constexpr unsigned EQ_SUFFIX_ONE_WG_VARS = 11;  // suffix equality tables of up to this many variables come from one workgroup

// eight lanes per pair, folding rounds only: lane 2k + j of a pair folds value j of array k (a, b, c; EqArray: and eq); Level: six fold, the
// seventh fetches the pair's E entry.  Then three lanes form one evaluation each: one fold product and two more deep.
template <CubicWeight W>
__device__ __forceinline__ void cubic_round_small(fe* __restrict__ a, fe* __restrict__ b, fe* __restrict__ c, weight_elem<W>* __restrict__ wt, size_t len,
                                                  fe_arg fold_arg, gate_args gate, red_out red) {
    constexpr bool LEVEL = W == CubicWeight::Level;
    PK_LATENCY_PRIO();
    __shared__ uint4 xs[2 * RED_THREADS];  // folded value of lane t at [t] (lo) and [RED_THREADS + t] (hi)
    const fe alpha = gate.host ? gate_wait(gate) : from_arg(fold_arg);
    const size_t npairs = len / 4, off = npairs, foff = len / 2;
    const unsigned tid = threadIdx.x, g = tid >> 3, role = tid & 7, k = role >> 1, which = role & 1;
    const size_t i = (size_t)blockIdx.x * (RED_THREADS / 8) + g;
    fe* arr = k == 0 ? a : k == 1 ? b : c;
    if constexpr (!LEVEL) arr = k == 0 ? a : k == 1 ? b : k == 2 ? c : wt;
    if (i < npairs && (!LEVEL || k < 3)) {  // sumcheck.rs:95-96: p0 += fold*(p2-p0); p1 += fold*(p3-p1)
        fe* p = arr + i + (which ? off : 0);
        fe x = fe_load(p), x2 = fe_load(p + foff);
        x = fe_fold(x, x2, alpha);
        fe_store(p, x);
        lds_put(xs, xs + RED_THREADS, tid, x);
    } else if (LEVEL && i < npairs && role == 6) {
        lds_put(xs, xs + RED_THREADS, tid, fe_load(wt + i));
    }
    __syncthreads();
    fe acc[3] = {fe_zero(), fe_zero(), fe_zero()};
    if (i < npairs && role < 3) {
        const unsigned base = tid & ~7u;
        auto v = [&](unsigned kk, unsigned w) { return lds_get(xs, xs + RED_THREADS, base + 2 * kk + w); };
        const fe a0 = v(0, 0), a1 = v(0, 1), b0 = v(1, 0), b1 = v(1, 1), c0 = v(2, 0), c1 = v(2, 1), e0 = v(3, 0);
        fe e1;  // EqArray only
        if constexpr (!LEVEL) e1 = v(3, 1);
        // the three evaluations share one shape, X * (Y*Z - S), so the lanes of a pair run the same two multiplications on
        // operands selected by role (no divergent branches):
        //            EqArray                                                  Level
        //   role 0:  f0    = eq0 * (a0*b0 - c0)                               Q(0)  = E * (a0*b0 - c0)
        //   role 1:  f(-1) = (2eq0-eq1) * ((2a0-a1)(2b0-b1) - (2c0-c1))       Q(-1) = E * ((2a0-a1)(2b0-b1) - (2c0-c1))
        //   role 2:  f_inf = (b1-b0) * ((eq1-eq0)(a1-a0) - 0)                 Q_inf = E * ((a1-a0)(b1-b0) - 0)
        auto pick = [&](const fe& x0, const fe& x1) {  // written out: as two fe_select the compiler holds all three operands, 7 VGPRs more
            fe m1 = fe_sub(fe_dbl(x0), x1), d = fe_sub(x1, x0), r;
#pragma unroll
            for (int w = 0; w < 8; w++) r.v[w] = role == 0 ? x0.v[w] : role == 1 ? m1.v[w] : d.v[w];
            return r;
        };
        const fe pa = pick(a0, a1), pb = pick(b0, b1), pc = pick(c0, c1);
        fe X, Y, Z;
        if constexpr (LEVEL) {
            X = e0;
            Y = pa;
            Z = pb;
        } else {
            const fe pe = pick(e0, e1);
            X = fe_select(role == 2, pb, pe);
            Y = fe_select(role == 2, pe, pb);
            Z = pa;
        }
        const fe S = fe_select(role == 2, fe_zero(), pc);
        acc_only(acc, role, fe_mulx(X, fe_sub(fe_mulx(Y, Z), S)));
    }
    grid_finish_fe<3>(acc, red);
}
__global__ __launch_bounds__(RED_THREADS) void sumcheck_cubic_small_kernel(fe* __restrict__ a, fe* __restrict__ b, fe* __restrict__ c,
                                                                           fe* __restrict__ eq, size_t len, fe_arg fold_arg, gate_args gate, red_out red) {
    cubic_round_small<CubicWeight::EqArray>(a, b, c, eq, len, fold_arg, gate, red);
}

template <bool FOLD, int NS>
__global__ __launch_bounds__(RED_THREADS) void sumcheck_quadratic_small_kernel(const fe* __restrict__ f, const fe* __restrict__ w, size_t out_len,
                                                                               fe_arg fold_arg, gate_args gate, fe* __restrict__ f_out, fe* __restrict__ w_out,
                                                                               red_out red) {
    PK_LATENCY_PRIO();
    __shared__ uint4 xs[2 * RED_THREADS];
    const fe r = (FOLD && gate.host) ? gate_wait(gate) : from_arg(fold_arg);
    const size_t npairs = out_len / 2;
    const unsigned tid = threadIdx.x, g = tid >> 2, role = tid & 3;  // role: 0 f0, 1 f1, 2 w0, 3 w1
    const size_t i = (size_t)blockIdx.x * (RED_THREADS / 4) + g;
    if (i < npairs) {
        const fe* src = role < 2 ? f : w;
        const unsigned j = role & 1;
        fe x;
        if (FOLD) {
            fe x0 = fe_load(src + 4 * i + 2 * j), x1 = fe_load(src + 4 * i + 2 * j + 1);
            x = fe_fold(x0, x1, r);
            fe_store((role < 2 ? f_out : w_out) + 2 * i + j, x);
        } else {
            x = fe_load(src + 2 * i + j);
        }
        lds_put(xs, xs + RED_THREADS, tid, x);
    }
    __syncthreads();
    fe acc[NS];
#pragma unroll
    for (int q = 0; q < NS; q++) acc[q] = fe_zero();
    if (i < npairs && role < NS) {
        const unsigned base = tid & ~3u;
        const fe f0 = lds_get(xs, xs + RED_THREADS, base), f1 = lds_get(xs, xs + RED_THREADS, base + 1);
        const fe w0 = lds_get(xs, xs + RED_THREADS, base + 2), w1 = lds_get(xs, xs + RED_THREADS, base + 3);
        // one multiplication on operands selected by role: h(0) = f0 w0, h(1) = f1 w1, h(2) = (2f1-f0)(2w1-w0); two sums: role 1 forms h(2)
        const unsigned ev = NS == 3 ? role : 2 * role;
        const fe tf = fe_sub(fe_dbl(f1), f0), tw = fe_sub(fe_dbl(w1), w0);
        const fe X = fe_select(ev == 0, f0, fe_select(ev == 1, f1, tf)), Y = fe_select(ev == 0, w0, fe_select(ev == 1, w1, tw));
        acc_only(acc, role, fe_mulx(X, Y));
    }
    grid_finish_fe<NS>(acc, red);
}

// ---------------------------------------------------------------- S2 / S3 without the folded eq array
// eq is a product table: with variables 0 .. i-1 bound to alpha, the folded eq array of round i is
//   eq0[x] = P_i (1 - r_i) E_i[x],  eq1[x] = P_i r_i E_i[x],   P_i = prod_{k<i} eq(r_k, alpha_k),  E_i = eq(r[i+1 .. n), .),
// so the round's three sums are P_i (1 - r_i) Q(0), P_i (2 - 3 r_i) Q(-1), P_i (2 r_i - 1) Q_inf with
//   Q(0) = sum E (a0 b0 - c0),  Q(-1) = sum E ((2a0-a1)(2b0-b1) - (2c0-c1)),  Q_inf = sum E (a1-a0)(b1-b0):
// the kernels below fold a, b, c only, read one entry of the read-only level E_i per pair and return the three Q; the scalars are
// three host products (sumcheck_spliteq_correct).  12 products per folding pair instead of 15, three arrays moved instead of four.
//
// The levels E_0 .. E_{n-1} (2^(n-1), ..., 1 entries; variable 0 <-> most significant index bit, eval_eq's order) sit back to back
// in one buffer of 2^n elements: E_i at 2^n - 2^(n-i).  E_{n-1} = {1}; E_{i-1}[h + j] = r_i E_i[j], E_{i-1}[j] = E_i[j] - that, h = |E_i|.
struct point_args {
    fe_arg x[27];  // m_0 <= 27 (pk_scheme_create)
};
// one workgroup per point (blockIdx.x: 0 or 1): every level of the nv-variable point x[first, first + nv) by the recursion above,
// level by level as eq_half_tables_kernel, each level kept.  nv <= 14: the largest level has 2^13 entries.
__global__ __launch_bounds__(256) void eq_suffix_levels_kernel(point_args pt, unsigned first0, unsigned nv0, fe* __restrict__ out0, unsigned first1,
                                                               unsigned nv1, fe* __restrict__ out1) {
    PK_LATENCY_PRIO();
    __shared__ uint4 xs[2 * 16];
    const unsigned first = blockIdx.x ? first1 : first0, nv = blockIdx.x ? nv1 : nv0;
    fe* const out = blockIdx.x ? out1 : out0;
    const size_t N = (size_t)1 << nv;
    if (threadIdx.x < nv) lds_put(xs, xs + 16, threadIdx.x, from_arg(pt.x[first + threadIdx.x]));
    if (threadIdx.x == 32) fe_store(out + N - 2, fe_one());  // level nv - 1
    __threadfence_block();
    __syncthreads();
    for (unsigned l = nv - 1; l >= 1; l--) {  // level l - 1 from level l
        const size_t h = N >> (l + 1);
        const fe* in = out + N - (N >> l);
        fe* o = out + N - (N >> (l - 1));
        const fe xv = lds_get(xs, xs + 16, l);
        for (size_t j = threadIdx.x; j < h; j += 256) {
            const fe t = fe_load(in + j);
            const fe up = fe_mulx(t, xv);
            fe_store(o + h + j, up);
            fe_store(o + j, fe_sub(t, up));
        }
        __threadfence_block();
        __syncthreads();
    }
}
// the long levels 0 .. L-1 of an n-variable point, grid-wide, one product per entry: E_i[xhi, xlo] = F_i[xhi] E_L[xlo], where E_L (the
// tail of E itself, n-1-L index bits) and F = the levels of the point r[0, L] (F_i = eq(r[i+1 .. L], .)) come from the kernel above
__global__ __launch_bounds__(256) void eq_suffix_expand_kernel(fe* __restrict__ E, const fe* __restrict__ F, unsigned n, unsigned L) {
    PK_LATENCY_PRIO();
    const size_t N = (size_t)1 << n, total = N - (N >> L), NF = (size_t)2 << L;
    const unsigned nlo = n - 1 - L;
    const fe* EL = E + total;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const unsigned i = n - 1 - (63 - (unsigned)__clzll((long long)(N - g - 1)));  // N - g lies in (2^(n-i-1), 2^(n-i)]
        const size_t x = g - (N - (N >> i));
        fe_store(E + g, fe_mulx(fe_load(F + (NF - (NF >> i)) + (x >> nlo)), fe_load(EL + (x & (((size_t)1 << nlo) - 1)))));
    }
}

template <bool FOLD>
__global__ __launch_bounds__(RED_THREADS) void sumcheck_cubic_spliteq_kernel(fe* __restrict__ a, fe* __restrict__ b, fe* __restrict__ c,
                                                                             const fe* __restrict__ E, size_t len, fe_arg fold_arg, gate_args gate,
                                                                             red_out red) {
    cubic_round_wide<FOLD, CubicWeight::Level>(a, b, c, E, len, fold_arg, gate, red);
}
__global__ __launch_bounds__(RED_THREADS) void sumcheck_cubic_spliteq_small_kernel(fe* __restrict__ a, fe* __restrict__ b, fe* __restrict__ c,
                                                                                   const fe* __restrict__ E, size_t len, fe_arg fold_arg, gate_args gate,
                                                                                   red_out red) {
    cubic_round_small<CubicWeight::Level>(a, b, c, E, len, fold_arg, gate, red);
}

// the single-element tail of the fold (out_len == 1): v'[0] = v[0] + r (v[1]-v[0]); no pair to sum.  blockIdx.y selects
// one of up to two arrays folded by the same challenge (the sumcheck's polynomial and its weights) in one launch.
__global__ void fold_pairs_kernel(const fe* __restrict__ v0, fe* __restrict__ out0, const fe* __restrict__ v1, fe* __restrict__ out1,
                                  size_t out_len, fe_arg r_arg, gate_args gate) {
    PK_LATENCY_PRIO();
    const fe r = gate.host ? gate_wait(gate) : from_arg(r_arg);
    const fe* v = blockIdx.y ? v1 : v0;
    fe* out = blockIdx.y ? out1 : out0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < out_len; i += stride) {
        fe x0 = fe_load(v + 2 * i), x1 = fe_load(v + 2 * i + 1);
        fe_store(out + i, fe_fold(x0, x1, r));
    }
}

// up to four runs of elements, back to back into dst -- the context's mailbox, pinned host memory the device writes directly: the short
// tables of a sumcheck reach the host thread in one launch and no copy operation (prover.hip, the host tail)
struct table_runs {
    const fe* src[4];
    size_t n[4];
};
__global__ __launch_bounds__(256) void tables_to_host_kernel(table_runs R, fe* __restrict__ dst) {
    PK_LATENCY_PRIO();
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t base = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < R.n[k]; i += stride) fe_store(dst + base + i, fe_load(R.src[k] + i));
        base += R.n[k];
    }
}

// ---------------------------------------------------------------- S5: dot product(s)
// <w,f> and optionally <w,g> in one pass over w (the statement needs both sums, whir_r1cs.rs:401-405)
template <int NV>
__global__ __launch_bounds__(RED_THREADS) void dot_kernel(const fe* __restrict__ w, const fe* __restrict__ f, const fe* __restrict__ g,
                                                          size_t n, red_out red) {
    PK_LATENCY_PRIO();
    fe acc[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) acc[k] = fe_zero();
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        fe wi = fe_load(w + i);
        acc[0] = fe_add(acc[0], fe_mulx(wi, fe_load(f + i)));
        if (NV == 2) acc[NV - 1] = fe_add(acc[NV - 1], fe_mulx(wi, fe_load(g + i)));
    }
    grid_finish_fe<NV>(acc, red);
}

// NR weight rows (row k at w + k * row_stride) against f (and g): <w_k, f>, <w_k, g> for every k in ONE pass over f and g -- the
// three statement weights of whir_r1cs.rs:382-412 share their polynomials, so this is one launch and one round trip instead of three
// EQF: f is the equality table of ONE point that is never written out -- `f` points at the point's half tables (eq_half_tables_kernel,
// scale one) and the lane forms f[i] = hi[i >> nlo] lo[i & mask], the reduced product eq_accumulate_kernel would have stored
template <int NR, int NV, bool EQF = false>
__global__ __launch_bounds__(RED_THREADS) void dot_rows_kernel(const fe* __restrict__ w, size_t row_stride, const fe* __restrict__ f,
                                                               const fe* __restrict__ g, size_t n, unsigned nhi, unsigned nlo, red_out red) {
    PK_LATENCY_PRIO();
    static_assert(!EQF || NV == 1, "the equality table stands in for f alone");
    fe acc[NR * NV];
#pragma unroll
    for (int k = 0; k < NR * NV; k++) acc[k] = fe_zero();
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        fe fi;
        if constexpr (EQF) fi = fe_mulx(fe_load(f + (i >> nlo)), fe_load(f + ((size_t)1 << nhi) + (i & (((size_t)1 << nlo) - 1))));
        else fi = fe_load(f + i);
        fe gi = fi;
        if (NV == 2) gi = fe_load(g + i);
#pragma unroll
        for (int k = 0; k < NR; k++) {
            const fe wi = fe_load(w + (size_t)k * row_stride + i);
            acc[NV * k] = fe_add(acc[NV * k], fe_mulx(wi, fi));
            if (NV == 2) acc[NV * k + 1] = fe_add(acc[NV * k + 1], fe_mulx(wi, gi));
        }
    }
    grid_finish_fe<NR * NV>(acc, red);
}

// ---------------------------------------------------------------- E1: univariate evaluation
// sum_i c[i] z^i.  Workgroup b owns the contiguous segment [b S, (b + 1) S), S = 256 cnt; lane t Horner-evaluates its stride-256
// subsequence c[b S + t], c[b S + t + 256], ... in z^256 (every load coalesced across the wave), scales by z^t -- one product with an
// entry of a 256-entry table a tiny kernel builds once per point -- and by z^(b S), which lane 0 computes for the whole workgroup while the
// others run their loops; the grid reduces.  cnt + 2 products per lane.  (Until round 5 the subsequences were strided over the whole grid
// and every lane raised z to its own global index: 8 select-multiplications for the lane bits + up to 10 for the block bits on top of the
// cnt = 8 of its loop -- most of the kernel's arithmetic was exponentiation.)
struct pow2_args {
    fe_arg p[28];  // z^(2^i)
};
__global__ __launch_bounds__(RED_THREADS) void zpow_table_kernel(pow2_args zp, fe* __restrict__ ztab) {  // ztab[t] = z^t, t < 256
    PK_LATENCY_PRIO();
    fe h = fe_one();
#pragma unroll 1
    for (int i = 0; i < 8; i++)
        if ((threadIdx.x >> i) & 1u) h = fe_mulx(h, from_arg(zp.p[i]));
    fe_store(ztab + threadIdx.x, h);
}
// NP polynomials of the same length at the same point in one launch (a batch commitment's OOD answers, mtUtilities.go:51-76)
template <int NP>
__global__ __launch_bounds__(RED_THREADS) void horner_kernel(const fe* __restrict__ c, const fe* __restrict__ c_second, size_t n, size_t cnt, pow2_args zp,
                                                             const fe* __restrict__ ztab, red_out red) {
    PK_LATENCY_PRIO();
    __shared__ unsigned s_zb[8];
    static_assert(RED_THREADS == 256, "the lane table has 256 entries");
    const size_t base = (size_t)blockIdx.x * cnt * RED_THREADS;
    if (threadIdx.x == 0) {  // z^(b S) for the workgroup: the set bits of b S select entries of the host's z^(2^i) table
        fe zb = fe_one();
        bool any = false;
        for (int i = 8; i < 28; i++)
            if ((base >> i) & 1u) {
                zb = any ? fe_mulx(zb, from_arg(zp.p[i])) : from_arg(zp.p[i]);
                any = true;
            }
#pragma unroll
        for (int k = 0; k < 8; k++) s_zb[k] = zb.v[k];
    }
    const fe z256 = from_arg(zp.p[8]);
    const size_t first = base + threadIdx.x;
    fe acc[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) acc[q] = fe_zero();
    size_t mine = 0;  // how many of this lane's cnt elements exist
    if (first < n) {
        mine = (n - first + RED_THREADS - 1) / RED_THREADS;
        if (mine > cnt) mine = cnt;
    }
    if (mine) {
        const fe zt = fe_load(ztab + threadIdx.x);
#pragma unroll
        for (int q = 0; q < NP; q++) {
            const fe* cq = q == 0 ? c : c_second;
            fe h = fe_load(cq + first + (mine - 1) * RED_THREADS);
            for (size_t j = mine - 1; j-- > 0;) h = fe_add(fe_mulx(h, z256), fe_load(cq + first + j * RED_THREADS));
            acc[q] = fe_mulx(h, zt);
        }
    }
    __syncthreads();
    if (mine && base) {
        fe zb;
#pragma unroll
        for (int k = 0; k < 8; k++) zb.v[k] = s_zb[k];
#pragma unroll
        for (int q = 0; q < NP; q++) acc[q] = fe_mulx(acc[q], zb);
    }
    grid_finish_fe<NP>(acc, red);
}

// ---------------------------------------------------------------- W1: coefficient fold
// out[t] = sum_j c[2^k t + j] * prod_b r_b^bit_b(j)   (MultivarPoly, utilities.go:15-22: r[0] <-> bit 0)
struct fold_args {
    fe_arg r[8];
};
__global__ __launch_bounds__(256) void fold_coeffs_kernel(const fe* __restrict__ c, size_t n_out, unsigned k, fold_args ra,
                                                          fe* __restrict__ out) {
    PK_LATENCY_PRIO();
    __shared__ uint4 wts[256 * 2];
    // weight j = prod_b r_b^{bit_b(j)}: thread j builds its own with at most k multiplications (no serial doubling pass)
    if (threadIdx.x < (1u << k)) {
        fe w = fe_one();
        for (unsigned b = 0; b < k; b++)
            if ((threadIdx.x >> b) & 1u) w = fe_mulx(w, from_arg(ra.r[b]));
        lds_put(wts, wts + 256, threadIdx.x, w);
    }
    __syncthreads();
    const int fw = 1 << k;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_out; t += stride) {
        fe acc = fe_load(c + t * fw);
        for (int j = 1; j < fw; j++) acc = fe_add(acc, fe_mulx(fe_load(c + t * fw + j), lds_get(wts, wts + 256, j)));
        fe_store(out + t, acc);
    }
}

// the WHIR fold (k = 4) with the 16 weights formed on the host (11 products) and passed by value: no per-workgroup weight
// phase.  LANES = 1: one output per lane.  LANES = 16: late rounds with few outputs -- the 16 products of an output go to
// 16 neighbouring lanes and are summed as limb sums (reduce.hpp), one multiplication deep instead of fifteen.
struct fold16_args {
    fe_arg w[16];
};
template <int LANES>
__global__ __launch_bounds__(256) void fold16_kernel(const fe* __restrict__ c, size_t n_out, fold16_args wa, fe* __restrict__ out) {
    PK_LATENCY_PRIO();
    __shared__ uint4 wts[16 * 2];
    if (threadIdx.x < 16) lds_put(wts, wts + 16, threadIdx.x, from_arg(wa.w[threadIdx.x]));
    __syncthreads();
    if (LANES == 1) {
        const size_t stride = (size_t)gridDim.x * blockDim.x;
        for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_out; t += stride) {
            fe acc = fe_load(c + t * 16);
#pragma unroll 1
            for (int j = 1; j < 16; j++) acc = fe_add(acc, fe_mulx(fe_load(c + t * 16 + j), lds_get(wts, wts + 16, j)));
            fe_store(out + t, acc);
        }
    } else {
        const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x, t = g >> 4;
        const unsigned j = threadIdx.x & 15;
        wide w = wide_zero();
        if (t < n_out) wide_add_fe(w, fe_mulx(fe_load(c + g), lds_get(wts, wts + 16, j)));  // c[16 t + j] * w_j (w_0 = 1)
#pragma unroll
        for (unsigned off = 8; off >= 1; off >>= 1)
#pragma unroll
            for (int i = 0; i < 8; i++) w.l[i] += shfl_down_u64(w.l[i], off);
        if (j == 0 && t < n_out) fe_store(out + t, wide_reduce(w));
    }
}

// out = a + beta * b (out may alias neither): the batching combination of two committed polynomials in one pass
__global__ __launch_bounds__(256) void lincomb_kernel(fe* __restrict__ out, const fe* __restrict__ a, const fe* __restrict__ b, size_t n,
                                                      fe_arg beta_arg) {
    PK_LATENCY_PRIO();
    const fe beta = from_arg(beta_arg);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        fe_store(out + i, fe_add(fe_load(a + i), fe_mulx(beta, fe_load(b + i))));
}
// y += beta * x ; y = a o b
__global__ __launch_bounds__(256) void axpy_kernel(fe* __restrict__ y, const fe* __restrict__ x, size_t n, fe_arg beta_arg) {
    PK_LATENCY_PRIO();
    const fe beta = from_arg(beta_arg);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        fe_store(y + i, fe_add(fe_load(y + i), fe_mulx(beta, fe_load(x + i))));
}

// two such combinations with the same beta in one launch (blockIdx.y picks one): the coefficient and the evaluation tables of a batch of two
__global__ __launch_bounds__(256) void lincomb_pair_kernel(fe* __restrict__ out0, const fe* __restrict__ a0, const fe* __restrict__ b0, size_t n0,
                                                           fe* __restrict__ out1, const fe* __restrict__ a1, const fe* __restrict__ b1, size_t n1,
                                                           fe_arg beta_arg) {
    PK_LATENCY_PRIO();
    const fe beta = from_arg(beta_arg);
    fe* out = blockIdx.y ? out1 : out0;
    const fe* a = blockIdx.y ? a1 : a0;
    const fe* b = blockIdx.y ? b1 : b0;
    const size_t n = blockIdx.y ? n1 : n0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        fe_store(out + i, fe_add(fe_load(a + i), fe_mulx(beta, fe_load(b + i))));
}
// y += g0 r0 + g1 r1 + g2 r2 with row k at rows + k * row_stride: one read and one write of y where three axpy launches make three,
// and one Montgomery reduction for the three products (fe29.hpp dot29; the rows are reduced values).  Every step gives the reduced
// representative, so y's bits are what the three launches leave.
__global__ __launch_bounds__(256) void axpy3_kernel(fe* __restrict__ y, const fe* __restrict__ rows, size_t row_stride, size_t n, fe3_arg ga) {
    PK_LATENCY_PRIO();
    const fe29 g0 = unpack29<5>(from_arg(ga.g[0])), g1 = unpack29<5>(from_arg(ga.g[1])), g2 = unpack29<5>(from_arg(ga.g[2]));
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        dot29 d;
        dot29_init(d);
        dot29_add(d, unpack29<0>(fe_load(rows + i)), g0);
        dot29_add(d, unpack29<0>(fe_load(rows + row_stride + i)), g1);
        dot29_add(d, unpack29<0>(fe_load(rows + 2 * row_stride + i)), g2);
        fe_store(y + i, fe_add(fe_load(y + i), dot29_result(d)));
    }
}

// <w,f> and (nv == 2) <w,g>: out[4 * v]
int dot(pk_ctx* ctx, int nv, const uint64_t* d_w, const uint64_t* d_f, const uint64_t* d_g, size_t n, uint64_t* out) {
    if (n == 0) return reduce_empty(ctx, nv, out);
    red_out red;
    unsigned blocks;
    int rc = reduction_begin(ctx, n, &red, &blocks);
    if (rc) return rc;
    {
        ProfScope prof(ctx, "dot");
        auto kernel = nv == 2 ? dot_kernel<2> : dot_kernel<1>;
        kernel<<<blocks, RED_THREADS, 0, ctx->stream>>>((const fe*)d_w, (const fe*)d_f, (const fe*)d_g, n, red);
    }
    PK_LAUNCH_CHECK(ctx);
    return collect_reduction(ctx, nv, out);
}

// What the launch of a sumcheck round, cubic or quadratic, does once its arguments are checked: the reduction (its sequence number goes
// to the caller), the gate and the challenge argument -- not folding: no challenge and no gate (fe_arg{}, gate_none()) -- and the grid:
// reduction_begin's with a lane per pair, enough workgroups for all pairs with `lanes_per_pair` lanes each in a small round.
struct round_launch {
    red_out red;
    unsigned blocks;
    gate_args gate;
    fe_arg farg;
};
int round_launch_begin(pk_ctx* ctx, size_t npairs, unsigned lanes_per_pair, const uint64_t* fold_or_null, unsigned gate_seq, unsigned* red_seq_out,
                       round_launch* L) {
    int rc = reduction_begin(ctx, npairs, &L->red, &L->blocks);
    if (rc) return rc;
    *red_seq_out = L->red.seq;
    L->gate = gate_seq ? gate_for(ctx, gate_seq) : gate_none();
    L->farg = fold_or_null ? to_arg(fold_or_null) : fe_arg{};
    const size_t pairs_per_wg = RED_THREADS / lanes_per_pair;
    if (lanes_per_pair > 1) L->blocks = (unsigned)((npairs + pairs_per_wg - 1) / pairs_per_wg);
    return PK_OK;
}

}  // namespace

namespace pk {

// launch only: round results go to the pinned page under sequence number *red_seq_out.  gate_seq != 0 (latency mode, folding rounds
// only): the folding challenge is not known yet -- the kernel waits for gate_publish(ctx, gate_seq, challenge) (reduce.hpp)
int sumcheck_cubic_launch(pk_ctx* ctx, uint64_t* d_a, uint64_t* d_b, uint64_t* d_c, CubicWeight kind, uint64_t* d_weight, size_t len,
                          const uint64_t* fold_or_null, unsigned gate_seq, unsigned* red_seq_out) {
    PK_REQUIRE(ctx, d_a && d_b && d_c && d_weight && red_seq_out, "null pointer");
    PK_REQUIRE(ctx, is_pow2(len) && len >= 2, "size must be a power of two >= 2");  // sumcheck.rs:22-23
    const bool fold = fold_or_null || gate_seq;
    PK_REQUIRE(ctx, !fold || len >= 4, "size must be >= 4 when folding");    // sumcheck.rs:27
    const size_t npairs = fold ? len / 4 : len / 2;
    // a lane per pair, or -- folding rounds of few pairs only: there is no small kernel that does not fold -- eight lanes per pair
    const bool small = fold && npairs <= SMALL_ROUND_PAIRS;
    round_launch L;
    int rc = round_launch_begin(ctx, npairs, small ? 8 : 1, fold_or_null, gate_seq, red_seq_out, &L);
    if (rc) return rc;
    auto launch = [&](auto kernel, auto* weight) {
        ProfScope prof(ctx, "sumcheck_cubic");
        kernel<<<L.blocks, RED_THREADS, 0, ctx->stream>>>((fe*)d_a, (fe*)d_b, (fe*)d_c, weight, len, L.farg, L.gate, L.red);
    };
    if (kind == CubicWeight::Level)
        launch(small ? sumcheck_cubic_spliteq_small_kernel : fold ? sumcheck_cubic_spliteq_kernel<true> : sumcheck_cubic_spliteq_kernel<false>, (const fe*)d_weight);
    else
        launch(small ? sumcheck_cubic_small_kernel : fold ? sumcheck_cubic_kernel<true> : sumcheck_cubic_kernel<false>, (fe*)d_weight);
    PK_LAUNCH_CHECK(ctx);
    return PK_OK;
}
// out[0..12) = Q(0), Q(-1), Q_inf of round i  ->  the round's f(0), f(-1), f_inf;  P = P_i, r_i = the round's coordinate of the eq point
void sumcheck_spliteq_correct(const uint64_t P[4], const uint64_t r_i[4], uint64_t out[12]) {
    fe p, r, q[3];
    memcpy(p.v, P, 32);
    memcpy(r.v, r_i, 32);
    memcpy(q, out, 96);
    const fe one = fe_one(), r2 = fe_dbl(r);
    q[0] = fe_mulx(fe_mulx(p, fe_sub(one, r)), q[0]);                          // P (1 - r)
    q[1] = fe_mulx(fe_mulx(p, fe_sub(fe_dbl(one), fe_add(r2, r))), q[1]);      // P (2 - 3r)
    q[2] = fe_mulx(fe_mulx(p, fe_sub(r2, one)), q[2]);                         // P (2r - 1)
    memcpy(out, q, 96);
}
// P_{i+1} = P_i eq(r_i, alpha_i)
void sumcheck_spliteq_advance(uint64_t P[4], const uint64_t r_i[4], const uint64_t alpha_i[4]) {
    fe p, r, a;
    memcpy(p.v, P, 32);
    memcpy(r.v, r_i, 32);
    memcpy(a.v, alpha_i, 32);
    const fe one = fe_one(), ra = fe_mulx(r, a);
    p = fe_mulx(p, fe_add(fe_sub(fe_sub(one, r), a), fe_dbl(ra)));  // (1-r)(1-a) + r a = 1 - r - a + 2 r a
    memcpy(P, p.v, 32);
}
// every level E_0 .. E_{n-1} of the point r[0, n) into d_out (2^n elements; the layout above)
int eq_suffix_tables(pk_ctx* ctx, const uint64_t* r, unsigned n, uint64_t* d_out) {
    PK_REQUIRE(ctx, r && d_out, "null pointer");
    PK_REQUIRE(ctx, n >= 1 && n <= 27, "1 .. 27 variables");
    point_args pt{};
    for (unsigned i = 0; i < n; i++) pt.x[i] = to_arg(r + 4 * i);
    fe* E = (fe*)d_out;
    ProfScope prof(ctx, "eq_suffix_tables");
    if (n <= EQ_SUFFIX_ONE_WG_VARS) {  // one workgroup builds everything
        eq_suffix_levels_kernel<<<1, 256, 0, ctx->stream>>>(pt, 0, n, E, 0, 0, nullptr);
    } else {  // levels L .. n-1 (the point r[L, n)) and the factor tables (the point r[0, L]) by one workgroup each, levels 0 .. L-1 grid-wide
        const unsigned L = n / 2;
        const size_t N = (size_t)1 << n, total = N - (N >> L);
        int rc = ensure_ws(ctx, (size_t)64 << L);
        if (rc) return rc;
        eq_suffix_levels_kernel<<<2, 256, 0, ctx->stream>>>(pt, L, n - L, E + total, 0, L + 1, (fe*)ctx->d_ws);
        eq_suffix_expand_kernel<<<grid_for(ctx, total, 256), 256, 0, ctx->stream>>>(E, (const fe*)ctx->d_ws, n, L);
    }
    PK_LAUNCH_CHECK(ctx);
    return PK_OK;
}
// nsums = 3: h(0), h(1), h(2); nsums = 2: h(0), h(2) -- the caller holds the claim h(0) + h(1)
int sumcheck_quadratic_launch(pk_ctx* ctx, const uint64_t* d_f, const uint64_t* d_w, size_t len, const uint64_t* fold_or_null, unsigned gate_seq,
                              uint64_t* d_f_out, uint64_t* d_w_out, int nsums, unsigned* red_seq_out) {
    PK_REQUIRE(ctx, d_f && d_w && red_seq_out && (nsums == 2 || nsums == 3), "null pointer");
    PK_REQUIRE(ctx, is_pow2(len), "size must be a power of two");
    const bool fold = fold_or_null || gate_seq;
    const size_t out_len = fold ? len / 2 : len;
    PK_REQUIRE(ctx, out_len >= 2, "at least one pair is needed after folding");
    PK_REQUIRE(ctx, !fold || (d_f_out && d_w_out && d_f_out != d_f && d_w_out != d_w), "folding is out-of-place");
    const size_t npairs = out_len / 2;
    // a lane per pair, or -- rounds of few pairs, folding or not -- four lanes per pair
    const bool small = npairs <= SMALL_ROUND_PAIRS;
    round_launch L;
    int rc = round_launch_begin(ctx, npairs, small ? 4 : 1, fold_or_null, gate_seq, red_seq_out, &L);
    if (rc) return rc;
    if (!fold) d_f_out = d_w_out = nullptr;  // not folding: no output arrays either
    using kernel_t = void (*)(const fe*, const fe*, size_t, fe_arg, gate_args, fe*, fe*, red_out);
    static const kernel_t kernels[2][2][2] = {  // [nsums - 2][small][fold]
        {{sumcheck_quadratic_kernel<false, 2>, sumcheck_quadratic_kernel<true, 2>},
         {sumcheck_quadratic_small_kernel<false, 2>, sumcheck_quadratic_small_kernel<true, 2>}},
        {{sumcheck_quadratic_kernel<false, 3>, sumcheck_quadratic_kernel<true, 3>},
         {sumcheck_quadratic_small_kernel<false, 3>, sumcheck_quadratic_small_kernel<true, 3>}}};
    {
        ProfScope prof(ctx, "sumcheck_quadratic");
        kernels[nsums - 2][small][fold]<<<L.blocks, RED_THREADS, 0, ctx->stream>>>((const fe*)d_f, (const fe*)d_w, out_len, L.farg, L.gate, (fe*)d_f_out,
                                                                                  (fe*)d_w_out, L.red);
    }
    PK_LAUNCH_CHECK(ctx);
    return PK_OK;
}
// the host's side of a gated launch and the wait for a launch's three results without draining the stream (prover.hip, latency mode)
int sumcheck_collect_spin(pk_ctx* ctx, int nsums, unsigned red_seq, uint64_t out[12]) { return collect_reduction_spin(ctx, nsums, red_seq, out); }
int sumcheck_collect(pk_ctx* ctx, int nsums, uint64_t out[12]) { return collect_reduction(ctx, nsums, out); }  // after a launch without a gate
// the three-sum message of a two-sum round: out = h(0), h(2)  ->  h(0), h(1) = claim - h(0), h(2)
void sumcheck_quadratic_from_claim(const uint64_t claim[4], uint64_t out[12]) {
    fe cl, h0;
    memcpy(cl.v, claim, 32);
    memcpy(h0.v, out, 32);
    const fe h1 = fe_sub(cl, h0);
    memcpy(out + 8, out + 4, 32);
    memcpy(out + 4, h1.v, 32);
}
unsigned sumcheck_gate_next(pk_ctx* ctx) { return gate_next(ctx); }
// 0 = no gated kernel of this context gave up on its challenge since the last call, else PK_ERR_HIP with the message set (reduce.hpp)
void sumcheck_gate_clear(pk_ctx* ctx) { (void)gate_timed_out(ctx); }  // forget a give-up word without touching the error message
int sumcheck_gate_check(pk_ctx* ctx) { return gate_timed_out(ctx) ? set_err(ctx, PK_ERR_HIP, "%s", PK_GATE_TIMEOUT_MSG) : PK_OK; }
void sumcheck_gate_publish(pk_ctx* ctx, unsigned gate_seq, const uint64_t challenge[4]) {
    fe c;
    memcpy(c.v, challenge, 32);
    gate_publish(ctx, gate_seq, c);
}

int lincomb2(pk_ctx* ctx, uint64_t* d_out, const uint64_t* d_a, const uint64_t* beta, const uint64_t* d_b, size_t n) {
    PK_REQUIRE(ctx, beta && (n == 0 || (d_out && d_a && d_b)), "null pointer");
    if (!n) return PK_OK;
    ProfScope prof(ctx, "lincomb");
    lincomb_kernel<<<grid_for(ctx, n, 256), 256, 0, ctx->stream>>>((fe*)d_out, (const fe*)d_a, (const fe*)d_b, n, to_arg(beta));
    PK_LAUNCH_CHECK(ctx);
    return PK_OK;
}
int lincomb2_pair(pk_ctx* ctx, uint64_t* d_out0, const uint64_t* d_a0, const uint64_t* d_b0, size_t n0, uint64_t* d_out1, const uint64_t* d_a1,
                  const uint64_t* d_b1, size_t n1, const uint64_t* beta) {
    PK_REQUIRE(ctx, beta && (n0 == 0 || (d_out0 && d_a0 && d_b0)) && (n1 == 0 || (d_out1 && d_a1 && d_b1)), "null pointer");
    if (!n0 && !n1) return PK_OK;
    ProfScope prof(ctx, "lincomb");
    lincomb_pair_kernel<<<dim3(grid_for(ctx, n0 > n1 ? n0 : n1, 256), 2), 256, 0, ctx->stream>>>(
        (fe*)d_out0, (const fe*)d_a0, (const fe*)d_b0, n0, (fe*)d_out1, (const fe*)d_a1, (const fe*)d_b1, n1, to_arg(beta));
    PK_LAUNCH_CHECK(ctx);
    return PK_OK;
}
int axpy3(pk_ctx* ctx, uint64_t* d_y, const uint64_t* g3, const uint64_t* d_rows, size_t row_stride, size_t n) {
    PK_REQUIRE(ctx, g3 && (n == 0 || (d_y && d_rows)), "null pointer");
    if (!n) return PK_OK;
    ProfScope prof(ctx, "lincomb");
    fe3_arg ga;
    for (int k = 0; k < 3; k++) ga.g[k] = to_arg(g3 + 4 * k);
    axpy3_kernel<<<grid_for(ctx, n, 256), 256, 0, ctx->stream>>>((fe*)d_y, (const fe*)d_rows, row_stride, n, ga);
    PK_LAUNCH_CHECK(ctx);
    return PK_OK;
}
int to_coeffs_generated(pk_ctx* ctx, unsigned m, const uint64_t* d_wit, size_t n_wit, const RngKey& key, uint32_t stream_mask, uint32_t stream_g,
                        uint64_t* d_f_evals, uint64_t* d_g_evals, uint64_t* d_f_coeffs, uint64_t* d_g_coeffs) {
    PK_REQUIRE(ctx, d_f_evals && d_g_evals && d_f_coeffs && d_g_coeffs && (n_wit == 0 || d_wit), "null pointer");
    PK_REQUIRE(ctx, m >= 1 && m <= 30 && n_wit <= ((size_t)1 << (m - 1)), "witness longer than half the table");
    const size_t half = (size_t)1 << (m - 1), N = 2 * half;
    const gen_table tf = {(const fe*)d_wit, n_wit, half, half, stream_mask, (fe*)d_f_evals, (fe*)d_f_coeffs};
    const gen_table tg = {nullptr, 0, 0, N, stream_g, (fe*)d_g_evals, (fe*)d_g_coeffs};
    ProfScope prof(ctx, "to_coeffs");
    const unsigned logt = wavelet_low_bits(m);
    PK_HIP(ctx, hipFuncSetAttribute((const void*)wavelet_low_generated_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 1 << 16));
    wavelet_low_generated_kernel<<<dim3((unsigned)(N >> logt), 2), 256, ((size_t)2 << logt) * 16, ctx->stream>>>(tf, tg, key, logt);
    int rc = wavelet_high_sweeps<true>(ctx, (fe*)d_f_coeffs, logt, m);
    return rc ? rc : wavelet_high_sweeps<true>(ctx, (fe*)d_g_coeffs, logt, m);
}
int fold_pairs2(pk_ctx* ctx, const uint64_t* d_v0, uint64_t* d_out0, const uint64_t* d_v1, uint64_t* d_out1, size_t len, const uint64_t* r,
                unsigned gate_seq) {
    PK_REQUIRE(ctx, d_v0 && d_out0 && d_v1 && d_out1 && (r || gate_seq), "null pointer");
    PK_REQUIRE(ctx, is_pow2(len) && len >= 2, "size must be a power of two >= 2");
    if (gate_seq) {
        int rc = reduction_scratch(ctx);
        if (rc) return rc;
    }
    ProfScope prof(ctx, "fold_pairs");
    fold_pairs_kernel<<<dim3(grid_for(ctx, len / 2, 256), 2), 256, 0, ctx->stream>>>((const fe*)d_v0, (fe*)d_out0, (const fe*)d_v1, (fe*)d_out1,
                                                                                     len / 2, r ? to_arg(r) : fe_arg{},
                                                                                     gate_seq ? gate_for(ctx, gate_seq) : gate_none());
    PK_LAUNCH_CHECK(ctx);
    return PK_OK;
}
int tables_to_host(pk_ctx* ctx, const uint64_t* const* d_src, const size_t* n, unsigned count, uint64_t* host_out) {
    PK_REQUIRE(ctx, d_src && n && host_out && count >= 1 && count <= 4, "one to four runs");
    table_runs R{};
    size_t total = 0;
    for (unsigned k = 0; k < count; k++) {
        PK_REQUIRE(ctx, d_src[k] || !n[k], "null pointer");
        R.src[k] = (const fe*)d_src[k];
        R.n[k] = n[k];
        total += n[k];
    }
    if (!total) return PK_OK;
    PK_REQUIRE(ctx, total <= ((size_t)4 << PK_HOST_TAIL_MAX_LOG2), "short tables only");
    fe* m_dst = nullptr;
    int rc = mail_alloc(ctx, 32 * total, (void**)&m_dst);
    if (rc) return rc;
    {
        ProfScope prof(ctx, "tables_to_host");
        tables_to_host_kernel<<<grid_for(ctx, total, 256), 256, 0, ctx->stream>>>(R, m_dst);
    }
    PK_LAUNCH_CHECK(ctx);
    rc = sync_stream(ctx);  // the mailbox rewinds: what it holds is taken out before anything else is allocated there
    if (rc) return rc;
    memcpy(host_out, m_dst, 32 * total);
    return PK_OK;
}

int eval_univariate_multi(pk_ctx* ctx, const uint64_t* const* d_polys, unsigned np, size_t n, const uint64_t z[4], uint64_t* out) {
    PK_REQUIRE(ctx, np == 1 || np == 2, "one or two polynomials");
    if (n == 0) return reduce_empty(ctx, (int)np, out);
    PK_REQUIRE(ctx, (n >> 28) == 0, "polynomial too long for the evaluation kernel (2^28 coefficients)");
    red_out red;
    unsigned blocks;
    int rc = reduction_begin(ctx, n, &red, &blocks);
    if (rc) return rc;
    // not reduction_blocks' grid: ~8 coefficients per lane, at most RED_MAX_BLOCKS (1024) workgroups, each over a contiguous segment
    // of 256 * cnt coefficients
    size_t want = (n / 8 + RED_THREADS - 1) / RED_THREADS;
    const size_t cap = want < 1 ? 1 : (want > RED_MAX_BLOCKS ? RED_MAX_BLOCKS : want);
    const size_t cnt = (n + cap * RED_THREADS - 1) / (cap * RED_THREADS);
    blocks = (unsigned)((n + cnt * RED_THREADS - 1) / (cnt * RED_THREADS));
    if (!ctx->d_ztab) PK_HIP(ctx, hipMalloc(&ctx->d_ztab, 256 * 32));
    // z^(2^i) on the host (27 squarings)
    pow2_args zp;
    {
        fe b;
        memcpy(b.v, z, 32);
        for (int i = 0; i < 28; i++) {
            memcpy(zp.p[i].v, b.v, 32);
            b = fe_mulx(b, b);
        }
    }
    {
        ProfScope prof(ctx, "eval_univariate");
        zpow_table_kernel<<<1, RED_THREADS, 0, ctx->stream>>>(zp, (fe*)ctx->d_ztab);
        auto kernel = np == 2 ? horner_kernel<2> : horner_kernel<1>;
        kernel<<<blocks, RED_THREADS, 0, ctx->stream>>>((const fe*)d_polys[0], (const fe*)(np == 2 ? d_polys[1] : nullptr), n, cnt, zp,
                                                        (const fe*)ctx->d_ztab, red);
    }
    PK_LAUNCH_CHECK(ctx);
    return collect_reduction(ctx, (int)np, out);
}
int dot_rows(pk_ctx* ctx, const uint64_t* d_w, size_t row_stride, unsigned nrows, const uint64_t* d_f, const uint64_t* d_g, size_t n, uint64_t* out,
             bool defer) {
    const int nv = d_g ? 2 : 1;
    PK_REQUIRE(ctx, nrows == 3 && (out || defer) && (n == 0 || (d_w && d_f)), "three weight rows");
    PK_REQUIRE(ctx, !defer || (n != 0 && !ctx->red_across), "a deferred dot product needs work and a lone context");
    if (n == 0) return reduce_empty(ctx, 3 * nv, out);
    red_out red;
    unsigned blocks;
    int rc = reduction_begin(ctx, n, &red, &blocks);
    if (rc) return rc;
    {
        ProfScope prof(ctx, "dot");
        auto kernel = nv == 2 ? dot_rows_kernel<3, 2> : dot_rows_kernel<3, 1>;
        kernel<<<blocks, RED_THREADS, 0, ctx->stream>>>((const fe*)d_w, row_stride, (const fe*)d_f, (const fe*)d_g, n, 0, 0, red);
    }
    PK_LAUNCH_CHECK(ctx);
    if (defer) return PK_OK;
    return collect_reduction(ctx, 3 * nv, out);
}

namespace {
// the half tables of q points over n_vars variables, scaled, into the context's workspace (pk_eq_accumulate's first launch): the points
// and scales go through the pinned mailbox, which the table kernel reads directly.  *d_tables: [pt][2^nhi hi | 2^nlo lo].
int eq_half_tables(pk_ctx* ctx, unsigned n_vars, const uint64_t* points, const uint64_t* scales, unsigned q, unsigned* nhi_out, unsigned* nlo_out,
                   const fe** d_tables) {
    const unsigned nlo = (n_vars + 1) / 2, nhi = n_vars - nlo;
    PK_REQUIRE(ctx, n_vars <= 30 && nlo <= 16, "too many variables");
    *nhi_out = nhi;
    *nlo_out = nlo;
    *d_tables = nullptr;
    if (!q) return PK_OK;
    const size_t per_pt = ((size_t)1 << nhi) + ((size_t)1 << nlo);
    int rc = ensure_ws(ctx, 32 * (size_t)q * per_pt + 64);
    if (rc) return rc;
    char* mail = nullptr;
    rc = mail_alloc(ctx, 32 * ((size_t)q * n_vars + q), (void**)&mail);
    if (rc) return rc;
    fe* d_points = (fe*)mail;
    fe* d_scales = d_points + (size_t)q * n_vars;
    if (n_vars) memcpy(d_points, points, 32 * (size_t)q * n_vars);
    memcpy(d_scales, scales, 32 * (size_t)q);
    eq_half_tables_kernel<<<dim3(q, 2), 256, 0, ctx->stream>>>(d_points, d_scales, n_vars, nhi, nlo, (fe*)ctx->d_ws);
    *d_tables = (const fe*)ctx->d_ws;
    return PK_OK;
}
}  // namespace

int opening_first_launch(pk_ctx* ctx, const opening_first& a, unsigned grid, unsigned* red_seq_out) {
    PK_REQUIRE(ctx, a.d_p && a.d_w && red_seq_out && (a.nsums == 2 || a.nsums == 3), "null pointer");
    PK_REQUIRE(ctx, is_pow2(a.n) && a.n >= 2, "size must be a power of two >= 2");
    PK_REQUIRE(ctx, a.q == 0 || (a.points && a.scales), "null pointer");
    const bool combine = a.d_e0 != nullptr;
    PK_REQUIRE(ctx, !combine || (a.d_e1 && a.beta), "null pointer");
    PK_REQUIRE(ctx, a.nrows == 0 || ((a.nrows == 1 || a.nrows == 3) && a.row_scales && (a.row_len == 0 || a.d_rows) && a.row_len <= a.n), "one row or three");
    PK_REQUIRE(ctx, combine == (a.nrows != 0) && (combine || a.nsums == 3), "either the opening's first launch (combination and rows) or a round's (neither, three sums)");
    unsigned nhi, nlo;
    const fe* d_tables;
    ProfScope prof(ctx, "opening_first");
    int rc = eq_half_tables(ctx, ilog2(a.n), a.points, a.scales, a.q, &nhi, &nlo, &d_tables);
    if (rc) return rc;
    const size_t npairs = a.n / 2;
    red_out red;
    unsigned blocks;
    rc = reduction_begin(ctx, npairs, &red, &blocks);
    if (rc) return rc;
    *red_seq_out = red.seq;
    // eq_accumulate_kernel's grid, a lane per pair, as far as the reduction's partial sums reach: the point loop is a chain of dependent
    // loads and products, which more pairs per lane only lengthen
    const size_t want = (npairs + RED_THREADS - 1) / RED_THREADS;
    blocks = (unsigned)(want < (size_t)RED_MAX_BLOCKS ? want : (size_t)RED_MAX_BLOCKS);
    if (grid && grid < blocks) blocks = grid;
    first_rows R{(const fe*)a.d_rows, a.row_stride, a.row_len, {}};
    for (unsigned k = 0; k < a.nrows; k++) R.g.g[k] = to_arg(a.row_scales + 4 * k);
    using kernel_t = void (*)(const fe*, const fe*, fe_arg, fe*, fe*, size_t, unsigned, unsigned, unsigned, const fe*, int, first_rows, red_out);
    kernel_t kernel = opening_first_kernel<false, 0, 3>;
    if (combine && a.nrows == 1) kernel = a.nsums == 2 ? opening_first_kernel<true, 1, 2> : opening_first_kernel<true, 1, 3>;
    if (combine && a.nrows == 3) kernel = a.nsums == 2 ? opening_first_kernel<true, 3, 2> : opening_first_kernel<true, 3, 3>;
    kernel<<<blocks, RED_THREADS, 0, ctx->stream>>>((const fe*)a.d_e0, (const fe*)a.d_e1, combine ? to_arg(a.beta) : fe_arg{}, (fe*)a.d_p, (fe*)a.d_w, a.n,
                                                    nhi, nlo, a.q, d_tables, a.overwrite, R, red);
    PK_LAUNCH_CHECK(ctx);
    return PK_OK;
}

int dot_rows_eq(pk_ctx* ctx, const uint64_t* d_w, size_t row_stride, unsigned nrows, const uint64_t* point, unsigned n_vars, size_t n, uint64_t* out) {
    PK_REQUIRE(ctx, (nrows == 1 || nrows == 3) && out && point && (n == 0 || d_w), "one weight row or three");
    PK_REQUIRE(ctx, n <= ((size_t)1 << n_vars), "rows longer than the table");
    if (n == 0) return reduce_empty(ctx, (int)nrows, out);
    static const uint64_t one[4] = {0xac96341c4ffffffbULL, 0x36fc76959f60cd29ULL, 0x666ea36f7879462eULL, 0x0e0a77c19a07df2fULL};
    unsigned nhi, nlo;
    const fe* d_tables;
    int rc = eq_half_tables(ctx, n_vars, point, one, 1, &nhi, &nlo, &d_tables);
    if (rc) return rc;
    red_out red;
    unsigned blocks;
    rc = reduction_begin(ctx, n, &red, &blocks);
    if (rc) return rc;
    {
        ProfScope prof(ctx, "dot");
        auto kernel = nrows == 3 ? dot_rows_kernel<3, 1, true> : dot_rows_kernel<1, 1, true>;
        kernel<<<blocks, RED_THREADS, 0, ctx->stream>>>((const fe*)d_w, row_stride, d_tables, nullptr, n, nhi, nlo, red);
    }
    PK_LAUNCH_CHECK(ctx);
    return collect_reduction(ctx, (int)nrows, out);
}

}  // namespace pk

extern "C" {

int pk_to_coeffs(pk_ctx* ctx, uint64_t* d_evals, unsigned n_vars) {
    PK_ENTER(ctx);
    return wavelet<true>(ctx, nullptr, d_evals, n_vars);
}
int pk_to_evals(pk_ctx* ctx, uint64_t* d_coeffs, unsigned n_vars) {
    PK_ENTER(ctx);
    return wavelet<false>(ctx, nullptr, d_coeffs, n_vars);
}
// out-of-place forms: d_dst receives the transform of d_src (which is left untouched)
int pk_to_coeffs_into(pk_ctx* ctx, const uint64_t* d_src, uint64_t* d_dst, unsigned n_vars) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, d_src && d_src != d_dst, "source must differ from destination");
    return wavelet<true>(ctx, d_src, d_dst, n_vars);
}
int pk_to_evals_into(pk_ctx* ctx, const uint64_t* d_src, uint64_t* d_dst, unsigned n_vars) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, d_src && d_src != d_dst, "source must differ from destination");
    return wavelet<false>(ctx, d_src, d_dst, n_vars);
}

int pk_eq_accumulate(pk_ctx* ctx, uint64_t* d_w, unsigned n_vars, const uint64_t* points, const uint64_t* scales, unsigned q,
                     int overwrite) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, d_w && (q == 0 || (points && scales)), "null pointer");
    PK_REQUIRE(ctx, n_vars <= 30, "too many variables");
    const size_t n = (size_t)1 << n_vars;
    if (q == 0) {
        if (overwrite) PK_HIP(ctx, hipMemsetAsync(d_w, 0, 32 * n, ctx->stream));
        return PK_OK;
    }
    // tables use the context workspace; stream order keeps them clear of earlier kernels (NTT scratch)
    unsigned nhi, nlo;
    const fe* d_tables;
    {
        ProfScope prof(ctx, "eq_accumulate");
        int rc = eq_half_tables(ctx, n_vars, points, scales, q, &nhi, &nlo, &d_tables);
        if (rc) return rc;
        eq_accumulate_kernel<<<grid_for(ctx, nlo ? (n + 1) / 2 : n, 256), 256, 0, ctx->stream>>>((fe*)d_w, n, nhi, nlo, q, d_tables, overwrite);
    }
    PK_LAUNCH_CHECK(ctx);
    // the caller's host arrays were copied into the mailbox above: they may be reused on return
    return PK_OK;
}

int pk_eq_table(pk_ctx* ctx, const uint64_t* r, unsigned m, uint64_t* d_out) {
    PK_ENTER(ctx);
    static const uint64_t one[4] = {0xac96341c4ffffffbULL, 0x36fc76959f60cd29ULL, 0x666ea36f7879462eULL, 0x0e0a77c19a07df2fULL};
    return pk_eq_accumulate(ctx, d_out, m, r, one, 1, 1);
}


int pk_sumcheck_cubic_round(pk_ctx* ctx, uint64_t* d_a, uint64_t* d_b, uint64_t* d_c, uint64_t* d_eq, size_t len,
                            const uint64_t* fold_or_null, uint64_t out[12]) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, out, "null pointer");
    unsigned seq = 0;
    int rc = sumcheck_cubic_launch(ctx, d_a, d_b, d_c, CubicWeight::EqArray, d_eq, len, fold_or_null, 0, &seq);
    if (rc) return rc;
    return collect_reduction(ctx, 3, out);
}

int pk_sumcheck_quadratic_round(pk_ctx* ctx, const uint64_t* d_f, const uint64_t* d_w, size_t len, const uint64_t* fold_or_null,
                                uint64_t* d_f_out, uint64_t* d_w_out, uint64_t out[12]) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, out, "null pointer");
    unsigned seq = 0;
    int rc = sumcheck_quadratic_launch(ctx, d_f, d_w, len, fold_or_null, 0, d_f_out, d_w_out, 3, &seq);
    if (rc) return rc;
    return collect_reduction(ctx, 3, out);
}

// test entry points (tools/probes/pk_selftest.h): the routes of Proof::zk_rounds and WhirProver::sumcheck_rounds, one round per call
int pk_selftest_eq_suffix_tables(pk_ctx* ctx, const uint64_t* r, unsigned n, uint64_t* d_out) {
    PK_ENTER(ctx);
    return eq_suffix_tables(ctx, r, n, d_out);
}
// round `round` of the n-variable cubic sumcheck on a, b, c as they stand after round - 1 rounds (2^(n - round + 1) entries; 2^n for round 0): folds by
// alphas[round - 1] if round > 0, then out = f(0), f(-1), f_inf as pk_sumcheck_cubic_round gives them for the eq table of r folded by the same alphas
int pk_selftest_sumcheck_cubic_spliteq(pk_ctx* ctx, uint64_t* d_a, uint64_t* d_b, uint64_t* d_c, const uint64_t* d_tables, unsigned n, unsigned round,
                                       const uint64_t* r, const uint64_t* alphas, uint64_t out[12]) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, out && r && d_tables && n >= 1 && n <= 27 && round < n && (round == 0 || alphas), "bad round");
    const size_t N = (size_t)1 << n, len = round ? N >> (round - 1) : N;
    unsigned seq = 0;
    uint64_t* level = const_cast<uint64_t*>(d_tables) + 4 * (N - (N >> round));  // read only
    int rc = sumcheck_cubic_launch(ctx, d_a, d_b, d_c, CubicWeight::Level, level, len, round ? alphas + 4 * (round - 1) : nullptr, 0, &seq);
    if (rc) return rc;
    rc = collect_reduction(ctx, 3, out);
    if (rc) return rc;
    uint64_t P[4];
    const fe one = fe_one();
    memcpy(P, one.v, 32);
    for (unsigned k = 0; k < round; k++) sumcheck_spliteq_advance(P, r + 4 * k, alphas + 4 * k);
    sumcheck_spliteq_correct(P, r + 4 * round, out);
    return PK_OK;
}
// pk_sumcheck_quadratic_round by the two-sum kernels: out = h(0), claim - h(0), h(2)
int pk_selftest_sumcheck_quadratic_claim(pk_ctx* ctx, const uint64_t* d_f, const uint64_t* d_w, size_t len, const uint64_t* fold_or_null,
                                         uint64_t* d_f_out, uint64_t* d_w_out, const uint64_t claim[4], uint64_t out[12]) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, out && claim, "null pointer");
    unsigned seq = 0;
    int rc = sumcheck_quadratic_launch(ctx, d_f, d_w, len, fold_or_null, 0, d_f_out, d_w_out, 2, &seq);
    if (rc) return rc;
    rc = collect_reduction(ctx, 2, out);
    if (rc) return rc;
    sumcheck_quadratic_from_claim(claim, out);
    return PK_OK;
}

int pk_fold_pairs(pk_ctx* ctx, const uint64_t* d_v, size_t len, const uint64_t* r, uint64_t* d_out) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, d_v && d_out && r && d_v != d_out, "null or aliased pointer");
    PK_REQUIRE(ctx, is_pow2(len) && len >= 2, "size must be a power of two >= 2");
    fold_pairs_kernel<<<grid_for(ctx, len / 2, 256), 256, 0, ctx->stream>>>((const fe*)d_v, (fe*)d_out, nullptr, nullptr, len / 2, to_arg(r), gate_none());
    PK_LAUNCH_CHECK(ctx);
    return PK_OK;
}

int pk_dot(pk_ctx* ctx, const uint64_t* d_w, const uint64_t* d_f, size_t n, uint64_t out[4]) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, out && (n == 0 || (d_w && d_f)), "null pointer");
    return dot(ctx, 1, d_w, d_f, nullptr, n, out);
}

int pk_dot2(pk_ctx* ctx, const uint64_t* d_w, const uint64_t* d_f, const uint64_t* d_g, size_t n, uint64_t out[8]) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, out && (n == 0 || (d_w && d_f && d_g)), "null pointer");
    return dot(ctx, 2, d_w, d_f, d_g, n, out);
}

int pk_eval_univariate(pk_ctx* ctx, const uint64_t* d_coeffs, size_t n, const uint64_t z[4], uint64_t out[4]) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, out && z && (n == 0 || d_coeffs), "null pointer");
    const uint64_t* polys[1] = {d_coeffs};
    return pk::eval_univariate_multi(ctx, polys, 1, n, z, out);
}

int pk_fold_coeffs(pk_ctx* ctx, const uint64_t* d_coeffs, unsigned n_vars, const uint64_t* r, unsigned k, uint64_t* d_out) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, d_coeffs && d_out && (k == 0 || r), "null pointer");
    PK_REQUIRE(ctx, k <= 8 && k <= n_vars, "fold factor out of range");
    fold_args ra{};
    for (unsigned b = 0; b < k; b++) ra.r[b] = to_arg(r + 4 * b);
    size_t n_out = (size_t)1 << (n_vars - k);
    ProfScope prof(ctx, "fold_coeffs");
    if (k == 4) {  // weight j = prod_b r_b^{bit_b(j)} by doubling, on the host
        fe wt[16];
        wt[0] = fe_one();
        for (unsigned b = 0; b < 4; b++) {
            fe rb;
            memcpy(rb.v, r + 4 * b, 32);
            for (unsigned j = 0; j < (1u << b); j++) wt[(1u << b) + j] = fe_mulx(wt[j], rb);
        }
        fold16_args wa;
        for (int j = 0; j < 16; j++) memcpy(wa.w[j].v, wt[j].v, 32);
        if (n_out <= 8192)
            fold16_kernel<16><<<(unsigned)((n_out * 16 + 255) / 256), 256, 0, ctx->stream>>>((const fe*)d_coeffs, n_out, wa, (fe*)d_out);
        else
            fold16_kernel<1><<<grid_for(ctx, n_out, 256), 256, 0, ctx->stream>>>((const fe*)d_coeffs, n_out, wa, (fe*)d_out);
        PK_LAUNCH_CHECK(ctx);
        return PK_OK;
    }
    fold_coeffs_kernel<<<grid_for(ctx, n_out, 256), 256, 0, ctx->stream>>>((const fe*)d_coeffs, n_out, k, ra, (fe*)d_out);
    PK_LAUNCH_CHECK(ctx);
    return PK_OK;
}

int pk_fe_axpy(pk_ctx* ctx, uint64_t* d_y, const uint64_t* beta, const uint64_t* d_x, size_t n) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, beta && (n == 0 || (d_y && d_x)), "null pointer");
    if (!n) return PK_OK;
    ProfScope prof(ctx, "lincomb");
    axpy_kernel<<<grid_for(ctx, n, 256), 256, 0, ctx->stream>>>((fe*)d_y, (const fe*)d_x, n, to_arg(beta));
    PK_LAUNCH_CHECK(ctx);
    return PK_OK;
}

}  // extern "C"
