// prover.cpp -- the device half of libprovekit_rangecheck.so's C ABI: the prover (its arena, the launches of range.hip, the prover side
// of the outer transcript, the one inner lookup proof with its refusals translated) and the fused decomposition.  Host code; of other
// libraries it calls what provekit_hip.h and provekit_tuplelookup.h declare.
#include "prover.hpp"

#include <cstdio>

using pk::fail;
using pk::fe;
using pk::host_ms_since;

namespace {

// what group g of the plan looks up, in words
std::string group_name(const pkr_prover* p, unsigned g) {
    const pkr::Plan& P = p->plan;
    if (g < P.L) return "limb " + std::to_string(g) + " (a limb must be below 2^" + std::to_string(p->st.k) + ")";
    if (g < P.G)
        return "the top-check group (2^" + std::to_string(P.shift_of[g]) + " times limb " + std::to_string(P.L - 1) + ": the top limb must be below 2^" +
               std::to_string(P.r) + ")";
    return "the spare group (limb 0 again)";
}

// pkt_prove's refusal with its group translated: pkt names a row outside t as "stacked index <i> (group <g>, row <x>)"
std::string translated(const pkr_prover* p, const char* inner) {
    const std::string why = inner ? inner : "";
    const size_t at = why.find("(group ");
    unsigned g = 0;
    unsigned long long x = 0;
    if (at != std::string::npos && sscanf(why.c_str() + at, "(group %u, row %llu)", &g, &x) == 2 && g < p->plan.c)
        return "entry " + std::to_string(x) + " of " + group_name(p, g) + " is not in 0 .. 2^" + std::to_string(p->st.k) + " - 1: " + why;
    return why;
}

}  // namespace

extern "C" {

int pkr_prover_arena_bytes(const pkr_statement* stmt, size_t* bytes) {
    std::string why;
    if (!bytes) return pkr::refuse("null pointer");
    if (!pkr::statement_ok(stmt, why)) return pkr::refuse(why);
    const pkt_statement look = pkr::lookup_of(*stmt);
    size_t inner = 0;
    if (int rc = pkt_prover_arena_bytes(&look, &inner)) return pkr::g_error = std::string("pkt_prover_arena_bytes failed: ") + pkt_create_error(), rc;
    *bytes = pkr::layout(*stmt).total + inner;
    return PK_OK;
}

int pkr_prover_create(pk_ctx* ctx, const pkr_statement* stmt, pkr_prover** out) {
    auto stop = [](int rc, const std::string& reason) { return pkr::g_error = reason, rc; };
    return pk::create<pkr::Lib>(ctx, stmt, out, [&](std::unique_ptr<pkr_prover>& p) {
        p.reset(new pkr_prover());  // its destructor gives back what a return or a throw below leaves behind
        p->ctx = ctx;
        p->st = *stmt;
        p->plan = pkr::plan_of(stmt->bits, stmt->k);
        p->pattern = pkr::io_pattern(*stmt);
        if (int rc = pk_ctx_sync(ctx)) return stop(rc, "pk_ctx_sync failed");  // also selects the context's device
        p->at = pkr::layout(*stmt);
        void* base = nullptr;
        if (int rc = pk_malloc(ctx, p->at.total, &base)) return stop(rc, "pk_malloc of the arena failed");
        p->arena = (uint8_t*)base;
        for (hipEvent_t& e : p->ev)
            if (hipEventCreate(&e) != hipSuccess) return stop(PK_ERR_HIP, "hipEventCreate failed");
        const pkt_statement look = pkr::lookup_of(*stmt);
        if (int rc = pkt_prover_create(ctx, &look, &p->look)) return stop(rc, std::string("pkt_prover_create failed: ") + pkt_create_error());
        if (int rc = pkt_proof_bytes(&look, &p->proof_bytes)) return stop(rc, std::string("pkt_proof_bytes failed: ") + pkt_create_error());
        if (int rc = pkr::index_launch(nullptr, stmt->k, p->iota(), 0)) return stop(rc, "the index table's launch failed");
        if (hipStreamSynchronize(nullptr) != hipSuccess) return stop(PK_ERR_HIP, "the index table's kernel failed");
        p->staging.resize(p->proof_bytes);
        return PK_OK;
    });
}

int pkr_prover_destroy(pkr_prover* p) { return pk::destroy(p); }

const char* pkr_last_error(const pkr_prover* p) { return p ? p->err.c_str() : "null prover"; }

int pkr_decompose(pkr_prover* p, const uint64_t* d_f, uint64_t* const* d_limbs_out, uint64_t* d_m_out, uint64_t* first_bad) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkr_statement& st = p->st;
    if (first_bad) *first_bad = UINT64_MAX;
    if (!d_f || !d_limbs_out || !d_m_out) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    try {
        uint64_t* limbs[PKR_MAX_GROUPS] = {};
        for (unsigned i = 0; i < p->plan.L; i++)
            if (!(limbs[i] = d_limbs_out[i])) return fail(p, PK_ERR_BAD_ARG, "a limb column is NULL");
        // the caller's work on the context is finished before anything here reads its column; the library's own launches go to the null stream
        if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
        (void)hipEventRecord(p->ev[0], nullptr);
        if (int rc = pkr::decompose_launch(nullptr, st.n, st.bits, st.k, d_f, limbs, p->counts(), p->bad(), d_m_out, p->grid))
            return fail(p, rc, "the decomposition's launch failed");
        (void)hipEventRecord(p->ev[1], nullptr);
        unsigned long long bad = 0;
        if (hipMemcpy(&bad, p->bad(), 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(p, PK_ERR_HIP, "the decomposition failed");
        p->prof.decompose_ms = pk::between(p->ev[0], p->ev[1]);
        if (bad != ~0ull) {
            if (first_bad) *first_bad = bad;
            return fail(p, PK_ERR_UNSATISFIED, "entry " + std::to_string(bad) + " is not below 2^" + std::to_string(st.bits));
        }
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

int pkr_prove(pkr_prover* p, const uint64_t* const* d_limbs, const uint64_t* d_m, const uint64_t* bind, uint8_t* proof_out, size_t cap, size_t* len,
              pkr_claims* claims_out) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkr_statement& st = p->st;
    const pkr::Plan& P = p->plan;
    if (!d_limbs || !d_m || !len || (!proof_out && cap)) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    if (int rc = pk::proof_room_and_bind(p, p->proof_bytes, cap, len, bind, st.n_bind)) return rc;
    try {
        for (unsigned i = 0; i < P.L; i++)
            if (!d_limbs[i]) return fail(p, PK_ERR_BAD_ARG, "a limb column is NULL");
        pk::Transcript tr(p->pattern);
        for (unsigned i = 0; i < st.n_bind; i++) tr.add_scalar(pk::h_load(bind + 4 * i));
        const fe seed = tr.challenge_scalar();
        if (!tr.finished()) return fail(p, PK_ERR_IO_PATTERN, "the transcript left its pattern: " + tr.violation());

        // the groups of the plan: a limb column, or the top limb scaled into the arena
        if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
        const uint64_t* groups[PKR_MAX_GROUPS] = {};
        p->prof.scale_ms = 0;
        for (unsigned g = 0; g < P.c; g++) {
            groups[g] = d_limbs[P.limb_of[g]];
            if (!P.shift_of[g]) continue;
            (void)hipEventRecord(p->ev[0], nullptr);
            if (int rc = pkr::scale_launch(nullptr, st.n, P.shift_of[g], d_limbs[P.limb_of[g]], p->scaled(), p->grid)) return fail(p, rc, "the scale kernel's launch failed");
            (void)hipEventRecord(p->ev[1], nullptr);
            groups[g] = p->scaled();  // pkt's own launches follow the scale pass on the null stream
        }
        const uint64_t* table[1] = {p->iota()};
        pkt_claims look;
        size_t part = 0;
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = pkt_prove(p->look, groups, table, d_m, (const uint64_t*)seed.v, p->staging.data(), p->proof_bytes, &part, &look);
        p->prof.lookup_ms = host_ms_since(t0);
        if (P.r < st.k && hipStreamSynchronize(nullptr) == hipSuccess) p->prof.scale_ms = pk::between(p->ev[0], p->ev[1]);
        if (rc == PK_ERR_UNSATISFIED) return fail(p, rc, translated(p, pkt_last_error(p->look)));
        if (rc) return fail(p, rc, std::string("the lookup failed: ") + pkt_last_error(p->look));
        memcpy(proof_out, p->staging.data(), p->proof_bytes);
        if (claims_out) pkr::fill_claims(st, look, claims_out);
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

}  // extern "C"
