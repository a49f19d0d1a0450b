// prover.cpp -- the device half of libprovekit_fracsum.so's C ABI: the two provers (their arenas, the launches of tree.hip, the
// prover side of the outer transcripts, the chain of pks proofs) and the trees by themselves.  Host code; of other libraries it calls
// what provekit_hip.h and provekit_sumcheck.h declare.
#include "prover.hpp"

using pk::fail;
using pk::fe;
using pk::host_ms_since;

namespace {

// a prover of `stmt` with its arena, events and pks provers; the reason of a failure goes to pkf::g_error
int make_prover(pk_ctx* ctx, const pkf_statement& stmt, std::unique_ptr<pkf_prover>& out) {
    auto stop = [](int rc, const std::string& reason) { return pkf::g_error = reason, rc; };
    std::unique_ptr<pkf_prover> p(new pkf_prover());  // its destructor gives back what a return or a throw below leaves behind
    p->ctx = ctx;
    p->st = stmt;
    p->pattern = pkf::io_pattern(stmt);
    void* base = nullptr;
    if (int rc = pk_malloc(ctx, pkf::arena_bytes(stmt.n), &base)) return stop(rc, "pk_malloc of the arena failed");
    p->arena = (uint64_t*)base;
    p->ptree = p->arena, p->qtree = p->ptree + 4 * pkf::tree_fes(stmt.n), p->u = p->qtree + 4 * pkf::tree_fes(stmt.n);
    for (hipEvent_t& e : p->ev)
        if (hipEventCreate(&e) != hipSuccess) return stop(PK_ERR_HIP, "hipEventCreate failed");
    for (unsigned d = 1; d < stmt.n; d++) {
        const pks_statement ps = pkf::layer_statement(stmt, d);
        if (int rc = pks_prover_create(ctx, &ps, &p->layer[d])) return stop(rc, std::string("pks_prover_create failed: ") + pks_create_error());
    }
    out = std::move(p);
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

bool is_zero(const fe& x) { return pk::fe_eq(x, pk::fe_zero()); }

// The protocol on the trees as they stand (build / build_lookup of the leaves (d_p, d_q)): the outer transcript and the n - 1 pks
// proofs, into proof_out (pkf::proof_bytes(p->st) bytes).  point: n elements, the values: one each; any may be NULL.
int chain(pkf_prover* p, const uint64_t* d_p, const uint64_t* d_q, const uint64_t* bind, uint8_t* proof_out, uint64_t* point_out, uint64_t* value_p_out,
          uint64_t* value_q_out) {
    const pkf_statement& st = p->st;
    const unsigned n = st.n;
    pk::Transcript tr(p->pattern);
    for (unsigned i = 0; i < st.n_bind; i++) tr.add_scalar(pk::h_load(bind + 4 * i));
    tr.add_scalars(p->top, 4);
    for (int i = 0; i < 4; i++) {
        const fe canon = pk::h_to_canon(p->top[i]);
        memcpy(proof_out + 32 * i, canon.v, 32);
    }
    fe rho = tr.challenge_scalar();
    fe z[PKF_MAX_VARS], r[PKF_MAX_VARS], finals[4];
    pkf::Claims claim;
    claim.from_top(p->top, rho);
    claim.has_p = !(st.unit && n == 1);
    z[0] = rho;
    for (unsigned d = 1; d < n; d++) {
        const fe lambda = tr.challenge_scalar(), seed = tr.challenge_scalar();
        // the children are the two halves of layer d + 1: of the caller's tables at the bottom, of the arena above it
        const bool bottom = d + 1 == n, unit_leaves = pkf::unit_layer(st, d);
        const size_t half = (size_t)4 << d;
        const uint64_t* const pL = bottom ? d_p : p->ptree + 2 * half;
        const uint64_t* const qL = bottom ? d_q : p->qtree + 2 * half;
        // u_d goes to the null stream, where the sumcheck library's own launches follow it: no synchronise between the two
        (void)hipEventRecord(p->ev[2], nullptr);
        if (int rc = pkf::combine_launch(nullptr, (size_t)1 << d, unit_leaves ? nullptr : pL + half, qL + half, (const uint64_t*)lambda.v, p->u, p->grid))
            return fail(p, rc, "layer " + std::to_string(d) + "'s combine launch failed");
        (void)hipEventRecord(p->ev[3], nullptr);
        const uint64_t* const with_p[4] = {pL, qL, qL + half, p->u};
        const uint64_t* const without_p[3] = {qL, qL + half, p->u};
        const unsigned m = pkf::layer_tables(st, d);
        size_t part = 0;
        const auto t0 = std::chrono::steady_clock::now();
        if (int rc = pks_prove(p->layer[d], unit_leaves ? without_p : with_p, (const uint64_t*)z, (const uint64_t*)seed.v, proof_out + pkf::layer_at(st, d),
                               pkf::layer_bytes(st, d), &part, (uint64_t*)r, (uint64_t*)finals))
            return fail(p, rc, "layer " + std::to_string(d) + "'s sumcheck failed: " + pks_last_error(p->layer[d]));
        p->prof.layer_ms[d] = host_ms_since(t0);
        p->prof.combine_ms[d] = pk::between(p->ev[2], p->ev[3]);  // pks_prove is blocking: both events have completed
        tr.add_scalars(finals, m);
        rho = tr.challenge_scalar();
        claim.step(unit_leaves, finals, lambda, rho);
        for (unsigned i = 0; i < d; i++) z[i + 1] = r[i];
        z[0] = rho;
    }
    if (!tr.finished()) return fail(p, PK_ERR_IO_PATTERN, "the transcript left its pattern: " + tr.violation());
    if (point_out) memcpy(point_out, z, 32 * (size_t)n);
    if (value_p_out && claim.has_p) pkf::put_fe(value_p_out, claim.cp);
    if (value_q_out) pkf::put_fe(value_q_out, claim.cq);
    return PK_OK;
}

}  // namespace

extern "C" {

int pkf_prover_create(pk_ctx* ctx, const pkf_statement* stmt, pkf_prover** out) {
    if (out) *out = nullptr;
    std::string why;
    if (!ctx || !out) return pkf::refuse("null pointer");
    if (!pkf::statement_ok(stmt, why)) return pkf::refuse(why);
    try {
        std::unique_ptr<pkf_prover> p;
        if (int rc = make_prover(ctx, *stmt, p)) return rc;
        *out = p.release();
        pkf::g_error.clear();
        return PK_OK;
    } catch (...) {
        return pk::out_of_host_memory(pkf::g_error);
    }
}

int pkf_prover_destroy(pkf_prover* p) {
    if (!p) return PK_OK;
    const int rc = p->give_back();
    delete p;
    return rc;
}

const char* pkf_last_error(const pkf_prover* p) { return p ? p->err.c_str() : "null prover"; }

// Host only; here and not next to the verifier because the sumcheck provers' share comes from their launch header.
int pkf_prover_arena_bytes(const pkf_statement* stmt, size_t* bytes) {
    std::string why;
    if (!bytes) return pkf::refuse("null pointer");
    if (!pkf::statement_ok(stmt, why)) return pkf::refuse(why);
    *bytes = pkf::arena_bytes(stmt->n) + pkf::layers_arena_bytes(*stmt);
    return PK_OK;
}

int pkf_lookup_prover_arena_bytes(const pkf_lookup_statement* stmt, size_t* bytes) {
    std::string why;
    if (!bytes) return pkf::refuse("null pointer");
    if (!pkf::statement_ok(stmt, why)) return pkf::refuse(why);
    const pkf_statement F = pkf::side_f(*stmt), T = pkf::side_t(*stmt);
    *bytes = pkf::arena_bytes(F.n) + pkf::layers_arena_bytes(F) + pkf::arena_bytes(T.n) + pkf::layers_arena_bytes(T) + 32 * (pkf::tree_fes(F.n) + pkf::tree_fes(T.n));
    return PK_OK;
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
    const size_t need = pkf::proof_bytes(st);
    *len = need;
    if (cap < need) return fail(p, PK_ERR_BAD_ARG, "the proof buffer holds " + std::to_string(cap) + " bytes, the proof has " + std::to_string(need));
    if (st.n_bind && !bind) return fail(p, PK_ERR_BAD_ARG, "the statement binds elements: pass them");
    std::string why;
    if (!pkf::elements_below_p(bind, st.n_bind, "bind", why)) return fail(p, PK_ERR_BAD_ARG, why);
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
    if (out) *out = nullptr;
    std::string why;
    if (!ctx || !out) return pkf::refuse("null pointer");
    if (!pkf::statement_ok(stmt, why)) return pkf::refuse(why);
    try {
        std::unique_ptr<pkf_lookup_prover> p(new pkf_lookup_prover());
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
        *out = p.release();
        pkf::g_error.clear();
        return PK_OK;
    } catch (...) {
        return pk::out_of_host_memory(pkf::g_error);
    }
}

int pkf_lookup_prover_destroy(pkf_lookup_prover* p) {
    if (!p) return PK_OK;
    const int rc = p->give_back();
    delete p;
    return rc;
}

const char* pkf_lookup_last_error(const pkf_lookup_prover* p) { return p ? p->err.c_str() : "null prover"; }

int pkf_lookup_prove(pkf_lookup_prover* p, const uint64_t* d_f, const uint64_t* d_t, const uint64_t* d_m, const uint64_t* bind, uint8_t* proof_out, size_t cap,
                     size_t* len, pkf_lookup_claims* claims_out) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkf_lookup_statement& st = p->st;
    if (!d_f || !d_t || !d_m || !len || (!proof_out && cap)) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    pkf_prover *const F = p->side[PKF_SIDE_F], *const T = p->side[PKF_SIDE_T];
    const size_t len_f = pkf::proof_bytes(F->st), need = len_f + pkf::proof_bytes(T->st);
    *len = need;
    if (cap < need) return fail(p, PK_ERR_BAD_ARG, "the proof buffer holds " + std::to_string(cap) + " bytes, the proof has " + std::to_string(need));
    if (st.n_bind && !bind) return fail(p, PK_ERR_BAD_ARG, "the statement binds elements: pass them");
    std::string why;
    if (!pkf::elements_below_p(bind, st.n_bind, "bind", why)) return fail(p, PK_ERR_BAD_ARG, why);
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
