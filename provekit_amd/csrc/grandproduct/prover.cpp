// prover.cpp -- the device half of libprovekit_grandproduct.so's C ABI: the two provers (one arena each, the launches of tree.hip,
// the prover side of the outer transcripts, the chain of pks proofs) and the tree by itself.  Host code; of other libraries it calls
// what provekit_hip.h and provekit_sumcheck.h declare.
#include "prover.hpp"

using pk::fail;
using pk::fe;

namespace {

// a prover of `stmt` with its arena, events and pks provers; the reason of a failure goes to pkg::g_error
int make_prover(pk_ctx* ctx, const pkg_statement& stmt, std::unique_ptr<pkg_prover>& p) {
    p.reset(new pkg_prover());  // its destructor gives back what a failure or a throw below leaves behind
    p->st = stmt;
    p->pattern = pkg::io_pattern(stmt);
    return pk::gkr::make_frame(*p, ctx, pkg::tree_bytes(stmt.n), p->tree, stmt.n, pkg::layer_statement, pkg::g_error);
}

// after the tree's launches: the phase's time, the top values and the product, on the host
int read_top(pkg_prover* p, const uint64_t* d_bottom) {
    const unsigned n = p->st.n;
    (void)hipEventRecord(p->ev[1], nullptr);
    if (hipMemcpy(p->product.v, p->tree + 4, 32, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(p->top, n == 1 ? d_bottom : p->tree + 8, 64, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(p, PK_ERR_HIP, "the top of the tree did not arrive");
    p->prof.tree_ms = pk::between(p->ev[0], p->ev[1]);
    return PK_OK;
}

// the tree of d_v into the arena
int build(pkg_prover* p, const uint64_t* d_v) {
    // the caller's work on the context is finished before anything here reads its tables; the library's own launches go to the null stream
    if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
    (void)hipEventRecord(p->ev[0], nullptr);
    if (int rc = pkg::tree_launch(nullptr, p->st.n, d_v, p->tree, p->layers, p->grid)) return fail(p, rc, "the tree kernels' launch failed");
    return read_top(p, d_v);
}
// the leaves of one side into d_leaf and their tree into the arena
int build_leaves(pkg_prover* p, const pkg::Leaves& lv, uint64_t* d_leaf) {
    if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
    (void)hipEventRecord(p->ev[0], nullptr);
    if (int rc = pkg::leaf_tree_launch(nullptr, p->st.n, lv, d_leaf, p->tree, p->layers, p->grid)) return fail(p, rc, "the leaf and tree kernels' launch failed");
    return read_top(p, d_leaf);
}

// What the prover adds to the chain's rule (pkg::Chain, statement.hpp): layer d's two tables
struct Proving : pkg::Chain {
    const pkg_prover* p;
    const uint64_t* d_v;
    Proving(const pkg_prover* prover, const uint64_t* bottom) : Chain(prover->st), p(prover), d_v(bottom) {}
    // L_d and R_d are the two halves of layer d + 1: of the caller's table at the bottom, of the arena above it
    int tables(unsigned d, const fe*, const uint64_t** out) const {
        const uint64_t* const L = d + 1 == s.n ? d_v : p->tree + ((size_t)8 << d);
        out[0] = L, out[1] = L + ((size_t)4 << d);
        return PK_OK;
    }
};

// The protocol on the tree as it stands (build / build_leaves of d_v): gkr/chain.hpp's outer transcript and n - 1 pks proofs, into
// proof_out (pkg::proof_bytes(p->st) bytes).  point: n elements, value: one; either may be NULL.
int chain(pkg_prover* p, const uint64_t* d_v, const uint64_t* bind, uint8_t* proof_out, uint64_t* point_out, uint64_t* value_out) {
    Proving rule(p, d_v);
    if (int rc = pk::gkr::prove_chain(p, rule, p->top, bind, proof_out, point_out)) return rc;
    if (value_out) pkg::put_fe(value_out, rule.claim);
    return PK_OK;
}

}  // namespace

extern "C" {

int pkg_prover_create(pk_ctx* ctx, const pkg_statement* stmt, pkg_prover** out) {
    return pk::create<pkg::Lib>(ctx, stmt, out, [&](std::unique_ptr<pkg_prover>& p) { return make_prover(ctx, *stmt, p); });
}

int pkg_prover_destroy(pkg_prover* p) { return pk::destroy(p); }

const char* pkg_last_error(const pkg_prover* p) { return p ? p->err.c_str() : "null prover"; }

// Host only; here and not next to the verifier because the sumcheck provers' share comes from their launch header.
int pkg_prover_arena_bytes(const pkg_statement* stmt, size_t* bytes) {
    return pk::size_out<pkg::Lib>(stmt, bytes, [](const pkg_statement& s) { return pkg::tree_bytes(s.n) + pkg::layers_arena_bytes(s.n); });
}

int pkg_tree(pk_ctx* ctx, unsigned n, const uint64_t* d_v, uint64_t* d_tree_out, uint64_t* product_out) {
    if (!ctx || !d_v || !d_tree_out || !product_out) return pkg::refuse("null pointer");
    if (n < 1 || n > PKG_MAX_VARS) return pkg::refuse("n must be 1..28");
    if (int rc = pk_ctx_sync(ctx)) return pkg::g_error = "pk_ctx_sync failed", rc;
    if (int rc = pkg::tree_launch(nullptr, n, d_v, d_tree_out, 0, 0)) return pkg::g_error = "the tree kernels' launch failed", rc;
    if (hipMemcpy(product_out, d_tree_out + 4, 32, hipMemcpyDeviceToHost) != hipSuccess) return pkg::g_error = "the product did not arrive", PK_ERR_HIP;
    return PK_OK;
}

int pkg_prove(pkg_prover* p, const uint64_t* d_v, const uint64_t* bind, uint8_t* proof_out, size_t cap, size_t* len, uint64_t* product_out, uint64_t* point_out,
              uint64_t* value_out) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkg_statement& st = p->st;
    if (!d_v || !len || (!proof_out && cap)) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    if (int rc = pk::proof_room_and_bind(p, pkg::proof_bytes(st), cap, len, bind, st.n_bind)) return rc;
    try {
        if (int rc = build(p, d_v)) return rc;
        if (int rc = chain(p, d_v, bind, proof_out, point_out, value_out)) return rc;
        if (product_out) pkg::put_fe(product_out, p->product);
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

int pkg_multiset_prover_create(pk_ctx* ctx, const pkg_multiset_statement* stmt, pkg_multiset_prover** out) {
    return pk::create<pkg::Lib>(ctx, stmt, out, [&](std::unique_ptr<pkg_multiset_prover>& p) {
        p.reset(new pkg_multiset_prover());
        p->ctx = ctx;
        p->st = *stmt;
        p->pattern = pkg::io_pattern(*stmt);
        void* base = nullptr;
        if (int rc = pk_malloc(ctx, pkg::tree_bytes(stmt->n), &base)) return pkg::g_error = "pk_malloc of the leaf table failed", rc;
        p->leaf = (uint64_t*)base;
        std::unique_ptr<pkg_prover> inner;
        if (int rc = make_prover(ctx, pkg::side_statement(*stmt), inner)) return rc;
        p->inner = inner.release();
        return PK_OK;
    });
}

int pkg_multiset_prover_destroy(pkg_multiset_prover* p) { return pk::destroy(p); }

const char* pkg_multiset_last_error(const pkg_multiset_prover* p) { return p ? p->err.c_str() : "null prover"; }

int pkg_multiset_prove(pkg_multiset_prover* p, const uint64_t* const* d_a, const uint64_t* const* d_b, const uint64_t* bind, uint8_t* proof_out, size_t cap,
                       size_t* len, pkg_multiset_claims* claims_out) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkg_multiset_statement& st = p->st;
    if (!d_a || !d_b || !len || (!proof_out && cap)) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    const size_t half = pkg::proof_bytes(pkg::side_statement(st));
    if (int rc = pk::proof_room(p, 2 * half, cap, len)) return rc;
    for (unsigned j = 0; j < st.w; j++)
        if (!d_a[j] || !d_b[j]) return fail(p, PK_ERR_BAD_ARG, "null column");
    if (int rc = pk::bind_ok(p, bind, st.n_bind)) return rc;
    try {
        pk::Transcript tr(p->pattern);
        for (unsigned i = 0; i < st.n_bind; i++) tr.add_scalar(pk::h_load(bind + 4 * i));
        const fe gamma = tr.challenge_scalar(), beta = st.w > 1 ? tr.challenge_scalar() : pk::fe_one();
        fe seeds[2];
        tr.challenge_scalars(seeds, 2);
        if (!tr.finished()) return fail(p, PK_ERR_IO_PATTERN, "the transcript left its pattern: " + tr.violation());

        pkg::Leaves side[2]{};
        for (int which = 0; which < 2; which++) {
            side[which].w = st.w;
            for (unsigned j = 0; j < st.w; j++) side[which].col[j] = (which ? d_b : d_a)[j];
            pkg::put_fe(side[which].gamma, gamma);
            pkg::put_fe(side[which].beta, beta);
        }
        pkg_prover* const g = p->inner;
        auto inner_failed = [&](int rc) { return fail(p, rc, g->err); };
        // the two products first, B's then A's, so that A's leaves and tree stand when its proof begins; nothing is written before
        if (int rc = build_leaves(g, side[1], p->leaf)) return inner_failed(rc);
        const fe product_b = g->product;
        if (int rc = build_leaves(g, side[0], p->leaf)) return inner_failed(rc);
        if (!pk::fe_eq(g->product, product_b))
            return fail(p, PK_ERR_UNSATISFIED, "the two sides are not equal as multisets: their products at (gamma, beta) differ");
        fe z[2][PKG_MAX_VARS], c[2];
        if (int rc = chain(g, p->leaf, (const uint64_t*)seeds[0].v, proof_out, (uint64_t*)z[0], (uint64_t*)c[0].v)) return inner_failed(rc);
        if (int rc = build_leaves(g, side[1], p->leaf)) return inner_failed(rc);
        if (int rc = chain(g, p->leaf, (const uint64_t*)seeds[1].v, proof_out + half, (uint64_t*)z[1], (uint64_t*)c[1].v)) return inner_failed(rc);
        if (claims_out) {
            memset(claims_out, 0, sizeof *claims_out);
            pkg::put_fe(claims_out->gamma, gamma);
            pkg::put_fe(claims_out->beta, beta);
            memcpy(claims_out->z_a, z[0], 32 * (size_t)st.n);
            memcpy(claims_out->z_b, z[1], 32 * (size_t)st.n);
            pkg::put_fe(claims_out->comb_a, pk::h_sub(gamma, c[0]));
            pkg::put_fe(claims_out->comb_b, pk::h_sub(gamma, c[1]));
        }
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

}  // extern "C"
