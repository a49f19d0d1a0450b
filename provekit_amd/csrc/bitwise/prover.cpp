// prover.cpp -- the device half of libprovekit_bitwise.so's C ABI: the prover (its arena, the launches of bitwise.hip, the prover side of
// the outer transcript, the one inner lookup proof with its refusals translated) and the fused decomposition.  Host code; of other
// libraries it calls what provekit_hip.h and provekit_tuplelookup.h declare.
#include "prover.hpp"

#include <cstdio>

using pk::fail;
using pk::fe;
using pk::host_ms_since;

namespace {

// what group g of the plan looks up, in words
std::string group_name(const pkb_prover* p, unsigned g) {
    const std::string row = "digit " + std::to_string(p->plan.digit_of[g]) + " (the row (a_i, b_i, c_i) must be a row of the " + pkb::op_name(p->st.op) + " table of " +
                            std::to_string(p->st.d) + "-bit digits)";
    return g < p->st.L ? row : "the spare group, " + row;
}

// pkt_prove's refusal with its group translated: pkt names a row outside t as "stacked index <i> (group <g>, row <x>)"
std::string translated(const pkb_prover* p, const char* inner) {
    const std::string why = inner ? inner : "";
    const size_t at = why.find("(group ");
    unsigned g = 0;
    unsigned long long x = 0;
    if (at != std::string::npos && sscanf(why.c_str() + at, "(group %u, row %llu)", &g, &x) == 2 && g < p->plan.c)
        return "entry " + std::to_string(x) + " of " + group_name(p, g) + " is not in the table: " + why;
    return why;
}

}  // namespace

extern "C" {

int pkb_prover_arena_bytes(const pkb_statement* stmt, size_t* bytes) {
    std::string why;
    if (!bytes) return pkb::refuse("null pointer");
    if (!pkb::statement_ok(stmt, why)) return pkb::refuse(why);
    const pkt_statement look = pkb::lookup_of(*stmt);
    size_t inner = 0;
    if (int rc = pkt_prover_arena_bytes(&look, &inner)) return pkb::g_error = std::string("pkt_prover_arena_bytes failed: ") + pkt_create_error(), rc;
    *bytes = pkb::layout(*stmt).total + inner;
    return PK_OK;
}

int pkb_prover_create(pk_ctx* ctx, const pkb_statement* stmt, pkb_prover** out) {
    auto stop = [](int rc, const std::string& reason) { return pkb::g_error = reason, rc; };
    return pk::create<pkb::Lib>(ctx, stmt, out, [&](std::unique_ptr<pkb_prover>& p) {
        p.reset(new pkb_prover());  // its destructor gives back what a return or a throw below leaves behind
        p->ctx = ctx;
        p->st = *stmt;
        p->plan = pkb::plan_of(stmt->L);
        p->pattern = pkb::io_pattern(*stmt);
        if (int rc = pk_ctx_sync(ctx)) return stop(rc, "pk_ctx_sync failed");  // also selects the context's device
        p->at = pkb::layout(*stmt);
        void* base = nullptr;
        if (int rc = pk_malloc(ctx, p->at.total, &base)) return stop(rc, "pk_malloc of the arena failed");
        p->arena = (uint8_t*)base;
        for (hipEvent_t& e : p->ev)
            if (hipEventCreate(&e) != hipSuccess) return stop(PK_ERR_HIP, "hipEventCreate failed");
        const pkt_statement look = pkb::lookup_of(*stmt);
        if (int rc = pkt_prover_create(ctx, &look, &p->look)) return stop(rc, std::string("pkt_prover_create failed: ") + pkt_create_error());
        if (int rc = pkt_proof_bytes(&look, &p->proof_bytes)) return stop(rc, std::string("pkt_proof_bytes failed: ") + pkt_create_error());
        uint64_t* const cols[3] = {p->table(0), p->table(1), p->table(2)};
        if (int rc = pkb::table_launch(nullptr, stmt->op, stmt->d, cols, 0)) return stop(rc, "the table's launch failed");
        if (hipStreamSynchronize(nullptr) != hipSuccess) return stop(PK_ERR_HIP, "the table's kernel failed");
        p->staging.resize(p->proof_bytes);
        return PK_OK;
    });
}

int pkb_prover_destroy(pkb_prover* p) { return pk::destroy(p); }

const char* pkb_last_error(const pkb_prover* p) { return p ? p->err.c_str() : "null prover"; }

int pkb_decompose(pkb_prover* p, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, int c_given, uint64_t* const* d_digits_out, uint64_t* d_m_out,
                  uint64_t* first_bad) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkb_statement& st = p->st;
    if (first_bad) *first_bad = UINT64_MAX;
    if (!d_a || !d_b || !d_c || !d_digits_out || !d_m_out) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    if (c_given != 0 && c_given != 1) return fail(p, PK_ERR_BAD_ARG, "c_given must be 0 or 1");
    try {
        for (unsigned i = 0; i < 3 * st.L; i++)
            if (!d_digits_out[i]) return fail(p, PK_ERR_BAD_ARG, "a digit column is NULL");
        // the caller's work on the context is finished before anything here reads its columns; the library's own launches go to the null stream
        if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
        (void)hipEventRecord(p->ev[0], nullptr);
        if (int rc = pkb::decompose_launch(nullptr, st.n, st.op, st.d, st.L, d_a, d_b, d_c, c_given != 0, d_digits_out, p->counts(), p->bad(), d_m_out, p->grid))
            return fail(p, rc, "the decomposition's launch failed");
        (void)hipEventRecord(p->ev[1], nullptr);
        unsigned long long bad = 0;
        if (hipMemcpy(&bad, p->bad(), 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(p, PK_ERR_HIP, "the decomposition failed");
        p->prof.decompose_ms = pk::between(p->ev[0], p->ev[1]);
        if (bad != pkb::NO_BAD) {
            const unsigned long long x = bad >> 2;
            const unsigned which = (unsigned)(bad & 3);
            if (first_bad) *first_bad = x;
            const std::string bits = std::to_string(st.L * st.d);
            return fail(p, PK_ERR_UNSATISFIED,
                        "entry " + std::to_string(x) + ": " +
                            (which == pkb::BAD_A   ? "a is not below 2^" + bits
                             : which == pkb::BAD_B ? "b is not below 2^" + bits
                                                   : std::string("c is not a ") + pkb::op_name(st.op) + " b"));
        }
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

int pkb_prove(pkb_prover* p, const uint64_t* const* d_digits, const uint64_t* d_m, const uint64_t* bind, uint8_t* proof_out, size_t cap, size_t* len,
              pkb_claims* claims_out) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkb_statement& st = p->st;
    const pkb::Plan& P = p->plan;
    if (!d_digits || !d_m || !len || (!proof_out && cap)) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    if (int rc = pk::proof_room_and_bind(p, p->proof_bytes, cap, len, bind, st.n_bind)) return rc;
    try {
        for (unsigned i = 0; i < 3 * st.L; i++)
            if (!d_digits[i]) return fail(p, PK_ERR_BAD_ARG, "a digit column is NULL");
        pk::Transcript tr(p->pattern);
        for (unsigned i = 0; i < st.n_bind; i++) tr.add_scalar(pk::h_load(bind + 4 * i));
        const fe seed = tr.challenge_scalar();
        if (!tr.finished()) return fail(p, PK_ERR_IO_PATTERN, "the transcript left its pattern: " + tr.violation());

        // the groups of the plan: group g's three columns are digit digit_of[g] of a, b and c
        const uint64_t* groups[PKB_MAX_DIGITS * 3] = {};
        for (unsigned g = 0; g < P.c; g++)
            for (unsigned j = 0; j < 3; j++) groups[3 * g + j] = d_digits[j * st.L + P.digit_of[g]];
        const uint64_t* table[3] = {p->table(0), p->table(1), p->table(2)};
        pkt_claims look;
        size_t part = 0;
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = pkt_prove(p->look, groups, table, d_m, (const uint64_t*)seed.v, p->staging.data(), p->proof_bytes, &part, &look);
        p->prof.lookup_ms = host_ms_since(t0);
        if (rc == PK_ERR_UNSATISFIED) return fail(p, rc, translated(p, pkt_last_error(p->look)));
        if (rc) return fail(p, rc, std::string("the lookup failed: ") + pkt_last_error(p->look));
        memcpy(proof_out, p->staging.data(), p->proof_bytes);
        if (claims_out) pkb::fill_claims(st, look, claims_out);
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

}  // extern "C"
