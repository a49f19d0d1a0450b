// prover.cpp -- the device half of libprovekit_fracsum.so's C ABI: the two provers (their arenas, the launches of tree.hip, the
// prover side of the outer transcripts, the chain of pks proofs) and the trees by themselves.  Host code; of other libraries it calls
// what provekit_hip.h and provekit_sumcheck.h declare.
#include "prover.hpp"

using pk::fail;
using pk::fe;

namespace {

// a prover of `stmt` with its arena, events and pks provers; the reason of a failure goes to pkf::g_error
int make_prover(pk_ctx* ctx, const pkf_statement& stmt, std::unique_ptr<pkf_prover>& p) {
    p.reset(new pkf_prover());  // its destructor gives back what a failure or a throw below leaves behind
    p->st = stmt;
    p->pattern = pkf::io_pattern(stmt);
    auto layer_statement = [&](unsigned d) { return pkf::layer_statement(stmt, d); };
    if (int rc = pk::gkr::make_frame(*p, ctx, pkf::arena_bytes(stmt.n), p->arena, stmt.n, layer_statement, pkf::g_error)) return rc;
    p->ptree = p->arena, p->qtree = p->ptree + 4 * pkf::tree_fes(stmt.n), p->u = p->qtree + 4 * pkf::tree_fes(stmt.n);
    return PK_OK;
}

// after the trees' launches: the phase's time, the top values and the fraction, on the host.  (d_p, d_q): the leaves, d_p NULL: unit
int read_top(pkf_prover* p, const uint64_t* d_p, const uint64_t* d_q) {
    const unsigned n = p->st.n;
    (void)hipEventRecord(p->ev[1], nullptr);
    const uint64_t* const from_p = n == 1 ? d_p : p->ptree + 8;
    p->top[0] = p->top[1] = pk::fe_one();
    if ((from_p && hipMemcpy(p->top, from_p, 64, hipMemcpyDeviceToHost) != hipSuccess) ||
        hipMemcpy(p->top + 2, n == 1 ? d_q : p->qtree + 8, 64, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(p, PK_ERR_HIP, "the top of the trees did not arrive");
    pkf::fraction_of(p->top, p->P, p->Q);
    p->prof.tree_ms = pk::between(p->ev[0], p->ev[1]);
    return PK_OK;
}

// the trees of (d_p, d_q) into the arena
int build(pkf_prover* p, const uint64_t* d_p, const uint64_t* d_q) {
    // the caller's work on the context is finished before anything here reads its tables; the library's own launches go to the null stream
    if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
    (void)hipEventRecord(p->ev[0], nullptr);
    if (int rc = pkf::tree_launch(nullptr, p->st.n, d_p, d_q, p->ptree, p->qtree, p->layers, p->grid)) return fail(p, rc, "the tree kernels' launch failed");
    return read_top(p, d_p, d_q);
}
// the leaves alpha - d_table of one side of a lookup into d_leaf and their trees (numerators d_m, NULL: unit) into the arena
int build_lookup(pkf_prover* p, const uint64_t* d_table, const uint64_t* d_m, const fe& alpha, uint64_t* d_leaf) {
    if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
    (void)hipEventRecord(p->ev[0], nullptr);
    if (int rc = pkf::lookup_leaf_launch(nullptr, p->st.n, d_table, d_m, (const uint64_t*)alpha.v, d_leaf, p->ptree, p->qtree, p->layers, p->grid))
        return fail(p, rc, "the leaf and tree kernels' launch failed");
    return read_top(p, d_m, d_leaf);
}

using pk::is_zero;

// What the prover adds to the chain's rule (pkf::Chain, statement.hpp): layer d's combined table u_d, made on the way, its three or
// four tables, and the combine pass's time
struct Proving : pkf::Chain {
    pkf_prover* p;
    const uint64_t *d_p, *d_q;
    Proving(pkf_prover* prover, const uint64_t* bottom_p, const uint64_t* bottom_q) : Chain(prover->st), p(prover), d_p(bottom_p), d_q(bottom_q) {}
    int tables(unsigned d, const fe* ch, const uint64_t** out) const {
        // the children are the two halves of layer d + 1: of the caller's tables at the bottom, of the arena above it
        const bool bottom = d + 1 == s.n, unit_leaves = pkf::unit_layer(s, d);
        const size_t half = (size_t)4 << d;
        const uint64_t* const pL = bottom ? d_p : p->ptree + 2 * half;
        const uint64_t* const qL = bottom ? d_q : p->qtree + 2 * half;
        // u_d goes to the null stream, where the sumcheck library's own launches follow it: no synchronise between the two
        (void)hipEventRecord(p->ev[2], nullptr);
        if (int rc = pkf::combine_launch(nullptr, (size_t)1 << d, unit_leaves ? nullptr : pL + half, qL + half, (const uint64_t*)ch[0].v, p->u, p->grid))
            return fail(p, rc, "layer " + std::to_string(d) + "'s combine launch failed");
        (void)hipEventRecord(p->ev[3], nullptr);
        if (!unit_leaves) *out++ = pL;
        out[0] = qL, out[1] = qL + half, out[2] = p->u;
        return PK_OK;
    }
    void step(unsigned d, const fe* finals, const fe* ch, const fe& rho) {
        p->prof.combine_ms[d] = pk::between(p->ev[2], p->ev[3]);  // pks_prove is blocking: both events have completed
        Chain::step(d, finals, ch, rho);
    }
};

// The protocol on the trees as they stand (build / build_lookup of the leaves (d_p, d_q)): gkr/chain.hpp's outer transcript and n - 1
// pks proofs, into proof_out (pkf::proof_bytes(p->st) bytes).  point: n elements, the values: one each; any may be NULL.
int chain(pkf_prover* p, const uint64_t* d_p, const uint64_t* d_q, const uint64_t* bind, uint8_t* proof_out, uint64_t* point_out, uint64_t* value_p_out,
          uint64_t* value_q_out) {
    Proving rule(p, d_p, d_q);
    if (int rc = pk::gkr::prove_chain(p, rule, p->top, bind, proof_out, point_out)) return rc;
    if (value_p_out && rule.claim.has_p) pkf::put_fe(value_p_out, rule.claim.cp);
    if (value_q_out) pkf::put_fe(value_q_out, rule.claim.cq);
    return PK_OK;
}

}  // namespace

extern "C" {

int pkf_prover_create(pk_ctx* ctx, const pkf_statement* stmt, pkf_prover** out) {
    return pk::create<pkf::Lib>(ctx, stmt, out, [&](std::unique_ptr<pkf_prover>& p) { return make_prover(ctx, *stmt, p); });
}

int pkf_prover_destroy(pkf_prover* p) { return pk::destroy(p); }

const char* pkf_last_error(const pkf_prover* p) { return p ? p->err.c_str() : "null prover"; }

// Host only; here and not next to the verifier because the sumcheck provers' share comes from their launch header.
int pkf_prover_arena_bytes(const pkf_statement* stmt, size_t* bytes) {
    return pk::size_out<pkf::Lib>(stmt, bytes, [](const pkf_statement& s) { return pkf::arena_bytes(s.n) + pkf::layers_arena_bytes(s); });
}

int pkf_lookup_prover_arena_bytes(const pkf_lookup_statement* stmt, size_t* bytes) {
    return pk::size_out<pkf::Lib>(stmt, bytes, [](const pkf_lookup_statement& s) {
        const pkf_statement F = pkf::side_f(s), T = pkf::side_t(s);
        return pkf::arena_bytes(F.n) + pkf::layers_arena_bytes(F) + pkf::arena_bytes(T.n) + pkf::layers_arena_bytes(T) + 32 * (pkf::tree_fes(F.n) + pkf::tree_fes(T.n));
    });
}

int pkf_tree(pk_ctx* ctx, unsigned n, const uint64_t* d_p_or_null, const uint64_t* d_q, uint64_t* d_ptree_out, uint64_t* d_qtree_out, uint64_t* fraction_out) {
    if (!ctx || !d_q || !d_ptree_out || !d_qtree_out || !fraction_out) return pkf::refuse("null pointer");
    if (n < 1 || n > PKF_MAX_VARS) return pkf::refuse("n must be 1..28");
    if (int rc = pk_ctx_sync(ctx)) return pkf::g_error = "pk_ctx_sync failed", rc;
    if (int rc = pkf::tree_launch(nullptr, n, d_p_or_null, d_q, d_ptree_out, d_qtree_out, 0, 0)) return pkf::g_error = "the tree kernels' launch failed", rc;
    if (hipMemcpy(fraction_out, d_ptree_out + 4, 32, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(fraction_out + 4, d_qtree_out + 4, 32, hipMemcpyDeviceToHost) != hipSuccess)
        return pkf::g_error = "the fraction did not arrive", PK_ERR_HIP;
    return PK_OK;
}

int pkf_prove(pkf_prover* p, const uint64_t* d_p_or_null, const uint64_t* d_q, const uint64_t* bind, uint8_t* proof_out, size_t cap, size_t* len,
              uint64_t* fraction_out, uint64_t* point_out, uint64_t* value_p_out, uint64_t* value_q_out) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkf_statement& st = p->st;
    if (!d_q || !len || (!proof_out && cap)) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    if (!d_p_or_null != (st.unit == 1)) return fail(p, PK_ERR_BAD_ARG, "the numerator table is NULL exactly when the statement's unit is 1");
    if (int rc = pk::proof_room_and_bind(p, pkf::proof_bytes(st), cap, len, bind, st.n_bind)) return rc;
    try {
        if (int rc = build(p, d_p_or_null, d_q)) return rc;
        if (is_zero(p->Q)) return fail(p, PK_ERR_UNSATISFIED, "a denominator is zero: Q = 0 and the sum of fractions is not defined");
        if (int rc = chain(p, d_p_or_null, d_q, bind, proof_out, point_out, value_p_out, value_q_out)) return rc;
        if (fraction_out) pkf::put_fe(fraction_out, p->P), pkf::put_fe(fraction_out + 4, p->Q);
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

int pkf_lookup_prover_create(pk_ctx* ctx, const pkf_lookup_statement* stmt, pkf_lookup_prover** out) {
    return pk::create<pkf::Lib>(ctx, stmt, out, [&](std::unique_ptr<pkf_lookup_prover>& p) {
        p.reset(new pkf_lookup_prover());
        p->ctx = ctx;
        p->st = *stmt;
        p->pattern = pkf::io_pattern(*stmt);
        const pkf_statement sides[2] = {pkf::side_f(*stmt), pkf::side_t(*stmt)};
        for (int which = 0; which < 2; which++) {
            void* base = nullptr;
            if (int rc = pk_malloc(ctx, 32 * pkf::tree_fes(sides[which].n), &base)) return pkf::g_error = "pk_malloc of a leaf table failed", rc;
            p->leaf[which] = (uint64_t*)base;
            std::unique_ptr<pkf_prover> inner;
            if (int rc = make_prover(ctx, sides[which], inner)) return rc;
            p->side[which] = inner.release();
        }
        return PK_OK;
    });
}

int pkf_lookup_prover_destroy(pkf_lookup_prover* p) { return pk::destroy(p); }

const char* pkf_lookup_last_error(const pkf_lookup_prover* p) { return p ? p->err.c_str() : "null prover"; }

int pkf_lookup_prove(pkf_lookup_prover* p, const uint64_t* d_f, const uint64_t* d_t, const uint64_t* d_m, const uint64_t* bind, uint8_t* proof_out, size_t cap,
                     size_t* len, pkf_lookup_claims* claims_out) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkf_lookup_statement& st = p->st;
    if (!d_f || !d_t || !d_m || !len || (!proof_out && cap)) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    pkf_prover *const F = p->side[PKF_SIDE_F], *const T = p->side[PKF_SIDE_T];
    const size_t len_f = pkf::proof_bytes(F->st);
    if (int rc = pk::proof_room_and_bind(p, len_f + pkf::proof_bytes(T->st), cap, len, bind, st.n_bind)) return rc;
    try {
        pk::Transcript tr(p->pattern);
        for (unsigned i = 0; i < st.n_bind; i++) tr.add_scalar(pk::h_load(bind + 4 * i));
        const fe alpha = tr.challenge_scalar();
        fe seeds[2];
        tr.challenge_scalars(seeds, 2);
        if (!tr.finished()) return fail(p, PK_ERR_IO_PATTERN, "the transcript left its pattern: " + tr.violation());

        // both sides' leaves, trees and roots first: each side has its own arena, so both stand; nothing is written before
        if (int rc = build_lookup(F, d_f, nullptr, alpha, p->leaf[PKF_SIDE_F])) return fail(p, rc, F->err);
        if (int rc = build_lookup(T, d_t, d_m, alpha, p->leaf[PKF_SIDE_T])) return fail(p, rc, T->err);
        if (is_zero(F->Q)) return fail(p, PK_ERR_UNSATISFIED, "a denominator is zero: alpha is an entry of f");
        if (is_zero(T->Q)) return fail(p, PK_ERR_UNSATISFIED, "a denominator is zero: alpha is an entry of t");
        if (!pkf::same_fraction(F->P, F->Q, T->P, T->Q))
            return fail(p, PK_ERR_UNSATISFIED, "the two sides' fractions differ: f is not inside t under m, or m is not f's multiplicities");
        fe z[2][PKF_MAX_VARS], cq[2], cp;
        if (int rc = chain(F, nullptr, p->leaf[PKF_SIDE_F], (const uint64_t*)seeds[0].v, proof_out, (uint64_t*)z[0], nullptr, (uint64_t*)cq[0].v)) return fail(p, rc, F->err);
        if (int rc = chain(T, d_m, p->leaf[PKF_SIDE_T], (const uint64_t*)seeds[1].v, proof_out + len_f, (uint64_t*)z[1], (uint64_t*)cp.v, (uint64_t*)cq[1].v))
            return fail(p, rc, T->err);
        if (claims_out) {
            memset(claims_out, 0, sizeof *claims_out);
            pkf::put_fe(claims_out->alpha, alpha);
            memcpy(claims_out->z_f, z[0], 32 * (size_t)st.n);
            memcpy(claims_out->z_t, z[1], 32 * (size_t)st.k);
            pkf::put_fe(claims_out->f_value, pk::h_sub(alpha, cq[0]));
            pkf::put_fe(claims_out->t_value, pk::h_sub(alpha, cq[1]));
            pkf::put_fe(claims_out->m_value, cp);
        }
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

}  // extern "C"
