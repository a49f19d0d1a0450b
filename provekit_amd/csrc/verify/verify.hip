// verify.hip -- the device path of libprovekit_verify.so: two kernels for gfx950 and the host code that feeds them.
//
// pkv_verify_many walks every proof twice with core.hpp's Walk.  Pass 1 (recorder) replays the Fiat-Shamir transcript, judges
// every relation that needs no opening and flattens the data-parallel work of ALL proofs into device arrays; the kernels run; pass
// 2 (replayer) is the host core again with the kernels' values in place of its own -- hence the same verdict and failing check.
//
// openings_kernel: one lane per opened leaf, across all proofs and rounds of the batch.  A lane folds its leaf (h = C(h, x_j),
//   width 16 or 32), walks sibling + path by the index bits, compares with the expected root, and on the way accumulates the
//   opening's fold value sum_j x_j * w_j (w = beta^b * prod r_t^bit_t(j): MultivarPoly of the beta-combined leaf).  The chain is
//   ~50 DEPENDENT compressions; a batch of 64 proofs is only ~12 k chains, fewer than the 16 k lanes that one wave per SIMD
//   would be on 256 CUs.  So there is no occupancy to win and nothing to hide latency with: the launch uses 64-lane workgroups
//   (one wave each) so that the ~190 waves spread over as many CUs as possible, and splitting leaf fold and path into two
//   launches would only add a launch and a round trip of the digests -- the chain stays as long.  Hashing runs in the scaled
//   domain of skyscraper29s.hpp (state = 32 x value): canonical inputs enter through to_scaled29, the digest leaves once through
//   from_scaled_canon, exactly as merkle_levels_kernel does.
// mat_eval_kernel: one lane per 4 matrix ENTRIES (not per row: the constant-one column and the grand-sum rows are ordinary
//   entries here).  A workgroup loads its 1024 entries once, then loops over the K proofs of the tile: term = v * eq_a_k[row] *
//   eq_y_k[col], wave-shuffle + LDS reduction, one partial per (proof, workgroup); sum_partials_kernel adds the partials.  The
//   matrix is read once per tile of up to 16 proofs; the eq tables come from pk_eq_table.
#include <hip/hip_runtime.h>

#include "../skyscraper29s.hpp"
#include "verifier.hpp"

using namespace pk;

namespace {

struct OpenDesc {  // offsets in field elements
    uint32_t leaf_off, width, node_off, n_nodes, w_off, pad;
    uint64_t index;
};

// nodes of an opening: sibling, path digests leaf -> root, then the expected root (n_nodes = depth + 2)
template <int VERSION>
__global__ __launch_bounds__(64) void openings_kernel(const fe* __restrict__ leaves, const fe* __restrict__ nodes, const fe* __restrict__ weights,
                                                      const OpenDesc* __restrict__ desc, size_t n, uint32_t* __restrict__ reached,
                                                      fe* __restrict__ folds) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const OpenDesc d = desc[i];
    const fe* lp = leaves + d.leaf_off;
    const fe* wp = weights + d.w_off;
    fe x = fe_reduce_any(fe_load(lp));  // the hash takes any 256-bit value mod p; so does the fold
    fe29 h = to_scaled29(x);
    fe acc = fe_mulx(x, fe_load(wp));  // canonical x Montgomery = canonical
    for (uint32_t j = 1; j < d.width; j++) {
        x = fe_reduce_any(fe_load(lp + j));
        h = compress29s<VERSION>(h, to_scaled29(x));
        acc = fe_add(acc, fe_mulx(x, fe_load(wp + j)));
    }
    const fe* np = nodes + d.node_off;
    uint64_t idx = d.index;
    for (uint32_t t = 0; t + 1 < d.n_nodes; t++) {
        const fe29 s = to_scaled29(fe_load(np + t));
        const bool right = idx & 1;  // this node is the right child: the sibling goes left
        fe29 l, r;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            l.v[k] = right ? s.v[k] : h.v[k];
            r.v[k] = right ? h.v[k] : s.v[k];
        }
        h = compress29s<VERSION>(l, r);
        idx >>= 1;
    }
    reached[i] = fe_eq(from_scaled_canon(h), fe_load(np + d.n_nodes - 1)) ? 1u : 0u;
    fe_store(folds + i, acc);
}

// sum of `v` over the workgroup's 256 lanes; valid in lane 0.  lds: 4 elements, not reused by the caller before its next barrier
__device__ __forceinline__ fe block_sum(fe v, fe* lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        fe o;
#pragma unroll
        for (int k = 0; k < 8; k++) o.v[k] = __shfl_down(v.v[k], off, 64);
        v = fe_add(v, o);
    }
    const unsigned wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) v = fe_add(fe_add(lds[0], lds[1]), fe_add(lds[2], lds[3]));
    return v;
}

constexpr int MAT_E = 4;  // entries per lane
__global__ __launch_bounds__(256) void mat_eval_kernel(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ cols,
                                                       const uint32_t* __restrict__ vals, size_t nnz, const fe* __restrict__ interner,
                                                       const fe* __restrict__ eq_a, size_t stride_a, const fe* __restrict__ eq_y, size_t stride_y,
                                                       unsigned K, fe* __restrict__ partial) {
    __shared__ fe lds[2][4];
    uint32_t row[MAT_E], col[MAT_E];
    fe v[MAT_E];
    const size_t base = (size_t)blockIdx.x * (256 * MAT_E);
#pragma unroll
    for (int t = 0; t < MAT_E; t++) {
        const size_t e = base + (size_t)t * 256 + threadIdx.x;
        const bool in = e < nnz;
        row[t] = in ? rows[e] : 0u;
        col[t] = in ? cols[e] : 0u;
        v[t] = in ? fe_load(interner + vals[e]) : fe_zero();
    }
    for (unsigned k = 0; k < K; k++) {
        const fe* ea = eq_a + (size_t)k * stride_a;
        const fe* ey = eq_y + (size_t)k * stride_y;
        fe acc = fe_zero();
#pragma unroll
        for (int t = 0; t < MAT_E; t++) acc = fe_add(acc, fe_mulx(fe_mulx(v[t], fe_load(ea + row[t])), fe_load(ey + col[t])));
        acc = block_sum(acc, lds[k & 1]);  // alternating buffers: one barrier per proof is enough
        if (threadIdx.x == 0) fe_store(partial + (size_t)k * gridDim.x + blockIdx.x, acc);
    }
}
// out[k * out_stride] = sum of partial[k][0..n): one workgroup per k
__global__ __launch_bounds__(256) void sum_partials_kernel(const fe* __restrict__ partial, size_t n, fe* __restrict__ out, unsigned out_stride) {
    __shared__ fe lds[4];
    const fe* p = partial + (size_t)blockIdx.x * n;
    fe acc = fe_zero();
    for (size_t i = threadIdx.x; i < n; i += 256) acc = fe_add(acc, fe_load(p + i));
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) fe_store(out + (size_t)blockIdx.x * out_stride, acc);
}

// ---- device state --------------------------------------------------------------------------------------------------------------
struct Buf {
    void* p = nullptr;
    size_t cap = 0;
};
struct DeviceState {
    hipStream_t stream = nullptr;
    uint32_t *rows[3] = {}, *cols[3] = {}, *vals[3] = {};
    size_t nnz[3] = {};
    fe* interner = nullptr;
    Buf leaves, nodes, weights, desc, reached, folds, eq_a, eq_y, partial, mout;
};
constexpr size_t MAT_TILE = 16;  // proofs per pass over the matrices (their eq tables are resident together)

int fail(pkv_verifier* v, int rc, const std::string& why) {
    v->err = why;
    return rc;
}
int fail_pk(pkv_verifier* v, int rc, const char* what) {
    const char* e = v->ctx ? pk_last_error(v->ctx) : "";
    return fail(v, rc, std::string(what) + ": " + (e ? e : ""));
}
int ensure(pk_ctx* ctx, Buf& b, size_t bytes) {
    if (b.cap >= bytes && b.p) return PK_OK;
    if (b.p) pk_free(ctx, b.p);
    b.p = nullptr;
    b.cap = 0;
    const size_t want = bytes + bytes / 4 + 256;
    int rc = pk_malloc(ctx, want, &b.p);
    if (!rc) b.cap = want;
    return rc;
}
void release_device(pkv_verifier* v) {
    DeviceState* d = static_cast<DeviceState*>(v->dev);
    if (d && v->ctx) {
        pk_ctx_sync(v->ctx);  // also selects the context's device on this thread
        if (d->stream) (void)hipStreamDestroy(d->stream);
        for (int k = 0; k < 3; k++) {
            pk_free(v->ctx, d->rows[k]);
            pk_free(v->ctx, d->cols[k]);
            pk_free(v->ctx, d->vals[k]);
        }
        pk_free(v->ctx, d->interner);
        for (Buf* b : {&d->leaves, &d->nodes, &d->weights, &d->desc, &d->reached, &d->folds, &d->eq_a, &d->eq_y, &d->partial, &d->mout}) pk_free(v->ctx, b->p);
    }
    delete d;
    v->dev = nullptr;
    v->ctx = nullptr;
    v->dev_release = nullptr;
}

// ---- the flattened openings of a batch -------------------------------------------------------------------------------------------
struct Flat {
    std::vector<fe> leaves, nodes, weights;
    std::vector<OpenDesc> desc;
    void add(const pkv::RoundOpenings& ro) {
        const uint32_t w_off = (uint32_t)weights.size();
        weights.insert(weights.end(), ro.weights.begin(), ro.weights.end());
        for (size_t q = 0; q < ro.k; q++) {
            OpenDesc d{};
            d.leaf_off = (uint32_t)leaves.size();
            d.width = ro.width;
            d.node_off = (uint32_t)nodes.size();
            d.n_nodes = ro.depth + 2;
            d.w_off = w_off;
            d.index = ro.indices[q];
            const size_t l0 = leaves.size();
            leaves.resize(l0 + ro.width);
            memcpy(leaves.data() + l0, ro.leaves[q], 32 * (size_t)ro.width);
            nodes.push_back(pkv::load_raw(ro.siblings[q]));
            for (unsigned t = ro.depth; t-- > 0;) nodes.push_back(pkv::load_raw(ro.paths[q * ro.depth + t]));
            nodes.push_back(ro.root);
            desc.push_back(d);
        }
    }
    bool fits() const { return leaves.size() < UINT32_MAX && nodes.size() < UINT32_MAX && weights.size() < UINT32_MAX; }
};

// runs the openings kernel over `flat`; reached / folds (canonical) come back to the host
int run_openings(pk_ctx* ctx, DeviceState& d, hipStream_t stream, int hash_version, const Flat& flat, std::vector<uint32_t>& reached, std::vector<fe>& folds,
                 std::string& why) {
    const size_t n = flat.desc.size();
    reached.assign(n, 0);
    folds.assign(n, fe_zero());
    if (!n) return PK_OK;
    int rc = PK_OK;
    auto up = [&](Buf& b, const void* src, size_t bytes) {
        if (rc) return;
        rc = ensure(ctx, b, bytes);
        if (!rc) rc = pk_memcpy_h2d(ctx, b.p, src, bytes);
    };
    up(d.leaves, flat.leaves.data(), 32 * flat.leaves.size());
    up(d.nodes, flat.nodes.data(), 32 * flat.nodes.size());
    up(d.weights, flat.weights.data(), 32 * flat.weights.size());
    up(d.desc, flat.desc.data(), sizeof(OpenDesc) * n);
    if (!rc) rc = ensure(ctx, d.reached, 4 * n);
    if (!rc) rc = ensure(ctx, d.folds, 32 * n);
    if (rc) {
        why = std::string("openings upload: ") + pk_last_error(ctx);
        return rc;
    }
    const unsigned grid = (unsigned)((n + 63) / 64);
    if (hash_version == 2)
        openings_kernel<2><<<grid, 64, 0, stream>>>((const fe*)d.leaves.p, (const fe*)d.nodes.p, (const fe*)d.weights.p, (const OpenDesc*)d.desc.p, n,
                                                    (uint32_t*)d.reached.p, (fe*)d.folds.p);
    else
        openings_kernel<1><<<grid, 64, 0, stream>>>((const fe*)d.leaves.p, (const fe*)d.nodes.p, (const fe*)d.weights.p, (const OpenDesc*)d.desc.p, n,
                                                    (uint32_t*)d.reached.p, (fe*)d.folds.p);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        why = std::string("openings kernel: ") + hipGetErrorString(e);
        return PK_ERR_HIP;
    }
    rc = pk_memcpy_d2h(ctx, reached.data(), d.reached.p, 4 * n);
    if (!rc) rc = pk_memcpy_d2h(ctx, folds.data(), d.folds.p, 32 * n);
    if (rc) why = std::string("openings download: ") + pk_last_error(ctx);
    return rc;
}

// out[3 k + matrix] for K (alpha, point) pairs, Montgomery
int run_matrix_evaluations(pkv_verifier* v, const fe* alphas, const fe* points, size_t K, fe* out) {
    DeviceState& d = *static_cast<DeviceState*>(v->dev);
    pk_ctx* ctx = v->ctx;
    const pkv::Statement& st = v->st;
    const unsigned m_0 = st.m_0, my = st.m - 1;
    const size_t sa = (size_t)1 << m_0, sy = (size_t)1 << my;
    for (size_t k0 = 0; k0 < K; k0 += MAT_TILE) {
        const size_t kt = std::min(MAT_TILE, K - k0);
        int rc = ensure(ctx, d.eq_a, 32 * sa * kt);
        if (!rc) rc = ensure(ctx, d.eq_y, 32 * sy * kt);
        if (!rc) rc = ensure(ctx, d.mout, 32 * 3 * kt);
        for (size_t k = 0; k < kt && !rc; k++) {
            rc = pk_eq_table(ctx, (const uint64_t*)(alphas + (k0 + k) * m_0), m_0, (uint64_t*)((fe*)d.eq_a.p + k * sa));
            if (!rc) rc = pk_eq_table(ctx, (const uint64_t*)(points + (k0 + k) * my), my, (uint64_t*)((fe*)d.eq_y.p + k * sy));
        }
        if (!rc) rc = pk_ctx_sync(ctx);
        if (rc) return fail_pk(v, rc, "eq tables");
        for (int mat = 0; mat < 3; mat++) {
            const size_t nnz = d.nnz[mat];
            const unsigned grid = (unsigned)std::max<size_t>(1, (nnz + 256 * MAT_E - 1) / (256 * MAT_E));
            rc = ensure(ctx, d.partial, 32 * (size_t)grid * kt);
            if (rc) return fail_pk(v, rc, "partial sums");
            mat_eval_kernel<<<grid, 256, 0, d.stream>>>(d.rows[mat], d.cols[mat], d.vals[mat], nnz, d.interner, (const fe*)d.eq_a.p, sa, (const fe*)d.eq_y.p,
                                                        sy, (unsigned)kt, (fe*)d.partial.p);
            sum_partials_kernel<<<(unsigned)kt, 256, 0, d.stream>>>((const fe*)d.partial.p, grid, (fe*)d.mout.p + mat, 3);
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(d.stream);  // d.partial is reused by the next matrix
            if (e != hipSuccess) return fail(v, PK_ERR_HIP, std::string("matrix evaluation kernel: ") + hipGetErrorString(e));
        }
        rc = pk_memcpy_d2h(ctx, out + 3 * k0, d.mout.p, 32 * 3 * kt);
        if (rc) return fail_pk(v, rc, "matrix evaluation download");
    }
    return PK_OK;
}

// ---- the two backends of the device path ---------------------------------------------------------------------------------------
struct Recorder : pkv::Backend {
    Flat& flat;
    size_t count = 0;
    std::vector<fe> alpha, point;
    bool wants_matrices = false;
    explicit Recorder(Flat& f) : flat(f) {}
    void openings(int, const pkv::RoundOpenings& ro, std::vector<uint8_t>& reached, std::vector<fe>& folds) override {
        tainted = true;
        flat.add(ro);
        count += ro.k;
        reached.assign(ro.k, 1);
        folds.assign(ro.k, fe_zero());
    }
    void matrix_evaluations(const pkv::Statement&, const std::vector<fe>& a, const std::vector<fe>& y, fe out[3]) override {
        tainted = true;
        alpha = a;
        point = y;
        wants_matrices = true;
        out[0] = out[1] = out[2] = fe_zero();
    }
};
struct Replayer : pkv::Backend {
    const uint32_t* reached_all;
    const fe* folds_all;
    size_t cursor, end;
    fe evals[3];
    void openings(int, const pkv::RoundOpenings& ro, std::vector<uint8_t>& reached, std::vector<fe>& folds) override {
        reached.assign(ro.k, 0);
        folds.assign(ro.k, fe_zero());
        for (size_t q = 0; q < ro.k && cursor < end; q++, cursor++) {
            reached[q] = reached_all[cursor] ? 1 : 0;
            folds[q] = h_from_canon(folds_all[cursor]);
        }
    }
    void matrix_evaluations(const pkv::Statement&, const std::vector<fe>&, const std::vector<fe>&, fe out[3]) override {
        for (int k = 0; k < 3; k++) out[k] = evals[k];
    }
};

}  // namespace

extern "C" {

int pkv_verifier_attach_device(pkv_verifier* v, pk_ctx* ctx) {
    if (!v) return PK_ERR_BAD_ARG;
    try {
        if (v->dev) release_device(v);
        if (!ctx) return PK_OK;
        int rc = pk_ctx_sync(ctx);  // selects the context's device on this thread
        if (rc) return fail(v, rc, std::string("context: ") + pk_last_error(ctx));
        DeviceState* d = new DeviceState();
        v->dev = d;
        v->ctx = ctx;
        v->dev_release = release_device;
        if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) {
            release_device(v);
            return fail(v, PK_ERR_HIP, "hipStreamCreate failed");
        }
        const pkv::Statement& st = v->st;
        if (st.has_r1cs) {
            auto up = [&](void** dst, const void* src, size_t bytes) {
                if (rc) return;
                rc = pk_malloc(ctx, bytes, dst);
                if (!rc && bytes) rc = pk_memcpy_h2d(ctx, *dst, src, bytes);
            };
            for (int k = 0; k < 3; k++) {
                d->nnz[k] = st.rows[k].size();
                up((void**)&d->rows[k], st.rows[k].data(), 4 * d->nnz[k]);
                up((void**)&d->cols[k], st.cols[k].data(), 4 * d->nnz[k]);
                up((void**)&d->vals[k], st.vals[k].data(), 4 * d->nnz[k]);
            }
            up((void**)&d->interner, st.interner.data(), 32 * st.interner.size());
            if (rc) {
                std::string why = std::string("R1CS upload: ") + pk_last_error(ctx);
                release_device(v);
                return fail(v, rc, why);
            }
        }
        return PK_OK;
    } catch (...) {
        return fail(v, PK_ERR_OOM, "out of memory");
    }
}

int pkv_verify_many(pkv_verifier* v, const uint8_t* const* proofs, const size_t* lens, size_t n, pkv_result* results) {
    if (!v) return PK_ERR_BAD_ARG;
    if (!v->dev || !v->ctx) return fail(v, PK_ERR_BAD_ARG, "no device attached (pkv_verifier_attach_device)");
    if (n && (!proofs || !lens || !results)) return fail(v, PK_ERR_BAD_ARG, "null pointer");
    for (size_t i = 0; i < n; i++)
        if (lens[i] && !proofs[i]) return fail(v, PK_ERR_BAD_ARG, "null proof");
    try {
        DeviceState& d = *static_cast<DeviceState*>(v->dev);
        static const uint8_t none = 0;
        struct Item {
            bool final = false;  // judged in pass 1: failed before any opening
            size_t first = 0, count = 0;
            bool wants_matrices = false;
            size_t matrix_slot = 0;
        };
        std::vector<Item> items(n);
        Flat flat;
        std::vector<fe> alphas, points;
        size_t n_matrix = 0;
        for (size_t i = 0; i < n; i++) {  // pass 1
            pkv::Verdict verdict;
            Recorder rec(flat);
            const size_t first = flat.desc.size();
            pkv::Walk walk(v->st, rec, lens[i] ? proofs[i] : &none, lens[i], verdict);
            walk.run();
            Item& it = items[i];
            it.first = first;
            it.count = rec.count;
            if (!rec.tainted) {  // nothing was deferred: this IS the host core's verdict
                it.final = true;
                pkv::to_result(verdict, &results[i]);
                continue;
            }
            if (rec.wants_matrices) {
                it.wants_matrices = true;
                it.matrix_slot = n_matrix++;
                alphas.insert(alphas.end(), rec.alpha.begin(), rec.alpha.end());
                points.insert(points.end(), rec.point.begin(), rec.point.end());
            }
        }
        if (!flat.fits()) return fail(v, PK_ERR_BAD_ARG, "batch too large: split it");
        std::vector<uint32_t> reached;
        std::vector<fe> folds, evals(3 * n_matrix);
        std::string why;
        int rc = pk_ctx_sync(v->ctx);  // selects the device
        if (!rc) rc = run_openings(v->ctx, d, d.stream, v->st.hash_version, flat, reached, folds, why);
        if (rc) return fail(v, rc, why);
        if (n_matrix) {
            rc = run_matrix_evaluations(v, alphas.data(), points.data(), n_matrix, evals.data());
            if (rc) return rc;
        }
        for (size_t i = 0; i < n; i++) {  // pass 2
            const Item& it = items[i];
            if (it.final) continue;
            pkv::Verdict verdict;
            Replayer rep;
            rep.reached_all = reached.data();
            rep.folds_all = folds.data();
            rep.cursor = it.first;
            rep.end = it.first + it.count;
            for (int k = 0; k < 3; k++) rep.evals[k] = it.wants_matrices ? evals[3 * it.matrix_slot + k] : fe_zero();
            pkv::Walk walk(v->st, rep, lens[i] ? proofs[i] : &none, lens[i], verdict);
            walk.run();
            pkv::to_result(verdict, &results[i]);
        }
        return PK_OK;
    } catch (...) {
        return fail(v, PK_ERR_OOM, "out of memory");
    }
}

int pkv_openings_check(pk_ctx* ctx, int hash_version, const uint64_t* leaves, size_t k, size_t width, const uint64_t* siblings, const uint64_t* paths,
                       size_t depth, const uint64_t* indices, const uint64_t* roots, const uint64_t* weights, uint8_t* reached, uint64_t* folds) {
    if (!ctx || (hash_version != 1 && hash_version != 2) || width < 1 || width > 64 || depth > 64) return PK_ERR_BAD_ARG;
    if (k && (!leaves || !siblings || (depth && !paths) || !indices || !roots || !reached)) return PK_ERR_BAD_ARG;
    if (k > (1u << 24)) return PK_ERR_BAD_ARG;
    try {
        Flat flat;
        flat.weights.assign(width, fe_zero());
        if (weights) memcpy(flat.weights.data(), weights, 32 * width);
        const fe* L = (const fe*)leaves;
        const fe* S = (const fe*)siblings;
        const fe* P = (const fe*)paths;
        const fe* R = (const fe*)roots;
        for (size_t q = 0; q < k; q++) {
            OpenDesc d{};
            d.leaf_off = (uint32_t)(q * width);
            d.width = (uint32_t)width;
            d.node_off = (uint32_t)flat.nodes.size();
            d.n_nodes = (uint32_t)depth + 2;
            d.index = indices[q];
            flat.nodes.push_back(S[q]);
            for (size_t t = depth; t-- > 0;) flat.nodes.push_back(P[q * depth + t]);
            flat.nodes.push_back(R[q]);
            flat.desc.push_back(d);
        }
        flat.leaves.assign(L, L + k * width);
        DeviceState d;
        std::vector<uint32_t> r;
        std::vector<fe> f;
        std::string why;
        int rc = pk_ctx_sync(ctx);
        if (!rc) rc = run_openings(ctx, d, nullptr, hash_version, flat, r, f, why);
        for (Buf* b : {&d.leaves, &d.nodes, &d.weights, &d.desc, &d.reached, &d.folds}) pk_free(ctx, b->p);
        if (rc) return rc;
        for (size_t q = 0; q < k; q++) reached[q] = (uint8_t)r[q];
        if (folds && k) memcpy(folds, f.data(), 32 * k);
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

int pkv_matrix_evaluations(pkv_verifier* v, const uint64_t* alphas, const uint64_t* points, size_t K, uint64_t* out) {
    if (!v) return PK_ERR_BAD_ARG;
    if (!v->dev || !v->ctx) return fail(v, PK_ERR_BAD_ARG, "no device attached (pkv_verifier_attach_device)");
    if (!v->st.has_r1cs) return fail(v, PK_ERR_BAD_ARG, "no R1CS attached");
    if (((size_t)1 << (v->st.m - 1)) < v->st.nw) return fail(v, PK_ERR_BAD_ARG, "witness does not fit 2^(m-1)");
    if (K && (!alphas || !points || !out)) return fail(v, PK_ERR_BAD_ARG, "null pointer");
    if (!K) return PK_OK;
    try {
        int rc = pk_ctx_sync(v->ctx);
        if (rc) return fail_pk(v, rc, "context");
        return run_matrix_evaluations(v, (const fe*)alphas, (const fe*)points, K, (fe*)out);
    } catch (...) {
        return fail(v, PK_ERR_OOM, "out of memory");
    }
}

}  // extern "C"
