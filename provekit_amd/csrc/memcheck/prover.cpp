// prover.cpp -- the device half of libprovekit_memcheck.so's C ABI: the prover (its arena, the launches of mem.hip, the prover side of
// the outer transcript, the three inner proofs, the balance), the trace builder and the leaves by themselves.  Host code; of other
// libraries it calls what provekit_hip.h and provekit_fracsum.h declare.
#include "prover.hpp"

using pk::fail;
using pk::fe;
using pk::host_ms_since;

namespace {

using pk::is_zero;

const char* const SIDE_NAMES[3] = {"OPS", "MEM", "TIME"};

// the statement's three inner arenas, summed; a refusal of a statement this library made is passed on with its reason
int inner_arena_bytes(const pkm_statement& s, size_t* out) {
    size_t total = 0, part = 0;
    for (int side = PKM_SIDE_OPS; side <= PKM_SIDE_MEM; side++) {
        const pkf_statement sum = pkm::side_sum(s, side);
        if (int rc = pkf_prover_arena_bytes(&sum, &part)) return pkm::g_error = std::string("pkf_prover_arena_bytes failed: ") + pkf_create_error(), rc;
        total += part;
    }
    const pkf_lookup_statement time = pkm::side_time(s);
    if (int rc = pkf_lookup_prover_arena_bytes(&time, &part)) return pkm::g_error = std::string("pkf_lookup_prover_arena_bytes failed: ") + pkf_create_error(), rc;
    *out = total + part;
    return PK_OK;
}

bool take_columns(const pkm_columns* cols, bool with_m, pkm::LeafColumns& out) {
    out = pkm::LeafColumns{cols->a, cols->wv, cols->rv, cols->rt, cols->init, cols->fin, cols->ft};
    return cols->a && cols->wv && cols->rv && cols->rt && cols->init && cols->fin && cols->ft && (!with_m || cols->m);
}

}  // namespace

extern "C" {

int pkm_prover_arena_bytes(const pkm_statement* stmt, size_t* bytes) {
    std::string why;
    if (!bytes) return pkm::refuse("null pointer");
    if (!pkm::statement_ok(stmt, why)) return pkm::refuse(why);
    size_t inner = 0;
    if (int rc = inner_arena_bytes(*stmt, &inner)) return rc;
    const size_t tmp = pkm::sort_tmp_bytes(stmt->n, stmt->k);
    if (!tmp) return pkm::g_error = "the sort's temporary storage could not be sized", PK_ERR_HIP;
    *bytes = pkm::layout(*stmt, tmp).total + inner;
    return PK_OK;
}

int pkm_prover_create(pk_ctx* ctx, const pkm_statement* stmt, pkm_prover** out) {
    auto stop = [](int rc, const std::string& reason) { return pkm::g_error = reason, rc; };
    return pk::create<pkm::Lib>(ctx, stmt, out, [&](std::unique_ptr<pkm_prover>& p) {
        p.reset(new pkm_prover());  // its destructor gives back what a return or a throw below leaves behind
        p->ctx = ctx;
        p->st = *stmt;
        p->pattern = pkm::io_pattern(*stmt);
        if (int rc = pk_ctx_sync(ctx)) return stop(rc, "pk_ctx_sync failed");  // also selects the context's device
        const size_t tmp = pkm::sort_tmp_bytes(stmt->n, stmt->k);
        if (!tmp) return stop(PK_ERR_HIP, "the sort's temporary storage could not be sized");
        p->at = pkm::layout(*stmt, tmp);
        void* base = nullptr;
        if (int rc = pk_malloc(ctx, p->at.total, &base)) return stop(rc, "pk_malloc of the arena failed");
        p->arena = (uint8_t*)base;
        for (hipEvent_t& e : p->ev)
            if (hipEventCreate(&e) != hipSuccess) return stop(PK_ERR_HIP, "hipEventCreate failed");
        for (int side = PKM_SIDE_OPS; side <= PKM_SIDE_MEM; side++) {
            const pkf_statement sum = pkm::side_sum(*stmt, side);
            if (int rc = pkf_prover_create(ctx, &sum, &p->sum[side])) return stop(rc, std::string("pkf_prover_create failed: ") + pkf_create_error());
            if (int rc = pkf_proof_bytes(&sum, &p->side_bytes[side])) return stop(rc, std::string("pkf_proof_bytes failed: ") + pkf_create_error());
            if (int rc = pkm::sign_launch(nullptr, sum.n - 1, p->sign(side), 0)) return stop(rc, "the sign table's launch failed");
        }
        const pkf_lookup_statement time = pkm::side_time(*stmt);
        if (int rc = pkf_lookup_prover_create(ctx, &time, &p->time)) return stop(rc, std::string("pkf_lookup_prover_create failed: ") + pkf_create_error());
        if (int rc = pkf_lookup_proof_bytes(&time, &p->side_bytes[PKM_SIDE_TIME])) return stop(rc, std::string("pkf_lookup_proof_bytes failed: ") + pkf_create_error());
        if (int rc = pkm::iota_launch(nullptr, stmt->n, p->t(), 0)) return stop(rc, "the time table's launch failed");
        if (hipStreamSynchronize(nullptr) != hipSuccess) return stop(PK_ERR_HIP, "the constant tables' kernels failed");
        p->staging.resize(p->side_bytes[0] + p->side_bytes[1] + p->side_bytes[2]);
        return PK_OK;
    });
}

int pkm_prover_destroy(pkm_prover* p) { return pk::destroy(p); }

const char* pkm_last_error(const pkm_prover* p) { return p ? p->err.c_str() : "null prover"; }

int pkm_trace(pkm_prover* p, const uint32_t* d_addr, const uint64_t* d_wv, const uint64_t* d_init, uint64_t* d_a, uint64_t* d_rv, uint64_t* d_rt, uint64_t* d_fin,
              uint64_t* d_ft, uint64_t* d_m, uint64_t* first_bad) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkm_statement& st = p->st;
    if (first_bad) *first_bad = UINT64_MAX;
    if (!d_addr || !d_wv || !d_init || !d_a || !d_rv || !d_rt || !d_fin || !d_ft || !d_m) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    try {
        // the caller's work on the context is finished before anything here reads its tables; the library's own launches go to the null stream
        if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
        const pkm::TraceTables tables{d_addr, d_wv, d_init, d_a, d_rv, d_rt, d_m, d_fin, d_ft};
        if (int rc = pkm::trace_launch(nullptr, st.n, st.k, tables, p->scratch(), p->grid, p->ev)) return fail(p, rc, "the trace builder's launches failed");
        unsigned long long bad = 0;
        if (hipMemcpy(&bad, p->scratch().bad, 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(p, PK_ERR_HIP, "the trace builder's kernels failed");
        p->prof.key_ms = pk::between(p->ev[0], p->ev[1]), p->prof.sort_ms = pk::between(p->ev[1], p->ev[2]);
        p->prof.resolve_ms = pk::between(p->ev[2], p->ev[3]), p->prof.count_ms = pk::between(p->ev[3], p->ev[4]);
        if (bad != ~0ull) {
            if (first_bad) *first_bad = bad;
            return fail(p, PK_ERR_BAD_ARG, "operation " + std::to_string(bad) + ": its address is outside the memory of 2^" + std::to_string(st.k) + " cells");
        }
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

int pkm_leaves(pk_ctx* ctx, unsigned n, unsigned k, const pkm_columns* cols, const uint64_t* gamma, const uint64_t* beta, uint64_t* d_ops_out, uint64_t* d_mem_out,
               uint64_t* d_f_out_or_null) {
    if (!ctx || !cols || !gamma || !beta || !d_ops_out || !d_mem_out) return pkm::refuse("null pointer");
    if (n < 1 || n > PKM_MAX_VARS) return pkm::refuse("n must be 1..27");
    if (k < 1 || k > PKM_MAX_VARS) return pkm::refuse("k must be 1..27");
    std::string why;
    if (!pkm::elements_below_p(gamma, 1, "gamma", why) || !pkm::elements_below_p(beta, 1, "beta", why)) return pkm::refuse(why);
    pkm::LeafColumns c{};
    if (!take_columns(cols, false, c)) return pkm::refuse("a column is NULL");
    if (int rc = pk_ctx_sync(ctx)) return pkm::g_error = "pk_ctx_sync failed", rc;
    if (int rc = pkm::ops_leaf_launch(nullptr, n, c, gamma, beta, d_ops_out, d_f_out_or_null, 0)) return pkm::g_error = "the operations' leaf launch failed", rc;
    if (int rc = pkm::cells_leaf_launch(nullptr, k, c, gamma, beta, d_mem_out, 0)) return pkm::g_error = "the cells' leaf launch failed", rc;
    if (hipStreamSynchronize(nullptr) != hipSuccess) return pkm::g_error = "the leaf kernels failed", PK_ERR_HIP;
    return PK_OK;
}

int pkm_prove(pkm_prover* p, const pkm_columns* cols, const uint64_t* bind, uint8_t* proof_out, size_t cap, size_t* len, pkm_claims* claims_out) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkm_statement& st = p->st;
    if (!cols || !len || (!proof_out && cap)) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    const size_t at[3] = {0, p->side_bytes[0], p->side_bytes[0] + p->side_bytes[1]}, need = at[2] + p->side_bytes[2];
    if (int rc = pk::proof_room_and_bind(p, need, cap, len, bind, st.n_bind)) return rc;
    try {
        pkm::LeafColumns c{};
        if (!take_columns(cols, true, c)) return fail(p, PK_ERR_BAD_ARG, "a column is NULL");
        pk::Transcript tr(p->pattern);
        for (unsigned i = 0; i < st.n_bind; i++) tr.add_scalar(pk::h_load(bind + 4 * i));
        pkm::Challenges ch;
        ch.gamma = tr.challenge_scalar();
        ch.beta = tr.challenge_scalar();
        tr.challenge_scalars(ch.seeds, 3);
        if (!tr.finished()) return fail(p, PK_ERR_IO_PATTERN, "the transcript left its pattern: " + tr.violation());

        // both stacked tables and f first: each has its own part of the arena
        if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
        (void)hipEventRecord(p->ev[0], nullptr);
        if (int rc = pkm::ops_leaf_launch(nullptr, st.n, c, (const uint64_t*)ch.gamma.v, (const uint64_t*)ch.beta.v, p->q(PKM_SIDE_OPS), p->f(), p->grid))
            return fail(p, rc, "side OPS's leaf launch failed");
        if (int rc = pkm::cells_leaf_launch(nullptr, st.k, c, (const uint64_t*)ch.gamma.v, (const uint64_t*)ch.beta.v, p->q(PKM_SIDE_MEM), p->grid))
            return fail(p, rc, "side MEM's leaf launch failed");
        (void)hipEventRecord(p->ev[1], nullptr);

        // the two stacked sums into the staging: pkf's own launches follow the leaves on the null stream.  Nothing of proof_out is written yet
        fe frac[2][2], z[2][PKF_MAX_VARS], cq[2], cp[2];
        for (int side = PKM_SIDE_OPS; side <= PKM_SIDE_MEM; side++) {
            size_t part = 0;
            const auto t0 = std::chrono::steady_clock::now();
            const int rc = pkf_prove(p->sum[side], p->sign(side), p->q(side), (const uint64_t*)ch.seeds[side].v, p->staging.data() + at[side], p->side_bytes[side], &part,
                                     (uint64_t*)frac[side], (uint64_t*)z[side], (uint64_t*)cp[side].v, (uint64_t*)cq[side].v);
            p->prof.side_ms[side] = host_ms_since(t0);
            if (rc == PK_ERR_UNSATISFIED)
                return fail(p, rc, std::string("a denominator is zero: gamma is a compressed triple of side ") + SIDE_NAMES[side]);
            if (rc) return fail(p, rc, std::string("side ") + SIDE_NAMES[side] + "'s fractional sum failed: " + pkf_last_error(p->sum[side]));
        }
        p->prof.leaf_ms = pk::between(p->ev[0], p->ev[1]);  // pkf_prove is blocking: both events have completed
        if (is_zero(frac[0][1]) || is_zero(frac[1][1])) return fail(p, PK_ERR_UNSATISFIED, "a denominator is zero: gamma is a compressed triple");
        if (!pkm::balanced(frac[0][0], frac[0][1], frac[1][0], frac[1][1]))
            return fail(p, PK_ERR_UNSATISFIED, "the multisets differ: the triples written (init and every write) are not the triples read (every read and fin)");
        // the time side: f = i - rt in t = (0 .. 2^n - 1) under m
        pkf_lookup_claims time;
        {
            size_t part = 0;
            const auto t0 = std::chrono::steady_clock::now();
            const int rc = pkf_lookup_prove(p->time, p->f(), p->t(), cols->m, (const uint64_t*)ch.seeds[PKM_SIDE_TIME].v, p->staging.data() + at[PKM_SIDE_TIME],
                                            p->side_bytes[PKM_SIDE_TIME], &part, &time);
            p->prof.side_ms[PKM_SIDE_TIME] = host_ms_since(t0);
            if (rc == PK_ERR_UNSATISFIED) {
                const std::string inner = pkf_lookup_last_error(p->time);
                if (inner.find("denominator") != std::string::npos) return fail(p, rc, "a denominator is zero on the time side: " + inner);
                return fail(p, rc, "a read is not older than its operation, or m is wrong: the time check's lookup of i - rt_i in 0 .. 2^n - 1 fails");
            }
            if (rc) return fail(p, rc, std::string("side TIME's lookup failed: ") + pkf_lookup_last_error(p->time));
        }
        memcpy(proof_out, p->staging.data(), need);
        if (claims_out) pkm::fill_claims(st, ch, z[0], cq[0], z[1], cq[1], time, claims_out);
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

}  // extern "C"
