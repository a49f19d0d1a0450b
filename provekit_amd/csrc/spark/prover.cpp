// prover.cpp -- the device half of libprovekit_spark.so's C ABI: the prover (its arena, the launches of spark.hip, the prover side of
// the outer transcript, the three inner proofs), the preprocessing of a matrix and the per-query gather.  Host code; of other libraries
// it calls what provekit_hip.h, provekit_sumcheck.h and provekit_tuplelookup.h declare.
#include "prover.hpp"

using pk::fail;
using pk::fe;
using pk::host_ms_since;

namespace {

const char* const SIDE_NAMES[3] = {"VAL", "ROW", "COL"};

// rx and ry present and below p, with the prover's failure or PK_OK
int point_ok(pkx_prover* p, const uint64_t* rx, const uint64_t* ry) {
    if (!rx || !ry) return fail(p, PK_ERR_BAD_ARG, "the point (rx, ry) is the statement: pass it");
    std::string why;
    if (!pkx::elements_below_p(rx, p->st.s, "rx", why) || !pkx::elements_below_p(ry, p->st.t, "ry", why)) return fail(p, PK_ERR_BAD_ARG, why);
    return PK_OK;
}

// eq(rx, .) and eq(ry, .) into the arena, finished: pk_eq_table works on the context, the library's own launches on the null stream
int eq_tables(pkx_prover* p, const uint64_t* rx, const uint64_t* ry) {
    if (int rc = pk_eq_table(p->ctx, rx, p->st.s, p->eq(0))) return fail(p, rc, "pk_eq_table of rx failed");
    if (int rc = pk_eq_table(p->ctx, ry, p->st.t, p->eq(1))) return fail(p, rc, "pk_eq_table of ry failed");
    if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
    return PK_OK;
}

// the cell of the first bad entry after a validating pass; PK_OK: none
int bad_entry(pkx_prover* p, uint64_t* first_bad) {
    unsigned long long bad = 0;
    if (hipMemcpy(&bad, p->bad(), 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(p, PK_ERR_HIP, "the kernels failed");
    if (bad == ~0ull) return PK_OK;
    if (first_bad) *first_bad = bad;
    return fail(p, PK_ERR_BAD_ARG, "entry " + std::to_string(bad) + ": its row is outside the 2^" + std::to_string(p->st.s) + " rows or its column outside the 2^" +
                                       std::to_string(p->st.t) + " columns");
}

}  // namespace

extern "C" {

int pkx_prover_arena_bytes(const pkx_statement* stmt, size_t* bytes) {
    std::string why;
    if (!bytes) return pkx::refuse("null pointer");
    if (!pkx::statement_ok(stmt, why)) return pkx::refuse(why);
    size_t total = pkx::layout(*stmt).total + pkx::val_arena_bytes(*stmt);
    for (int side = PKX_SIDE_ROW; side <= PKX_SIDE_COL; side++) {
        const pkt_statement look = pkx::side_lookup(*stmt, side);
        size_t inner = 0;
        if (int rc = pkt_prover_arena_bytes(&look, &inner)) return pkx::g_error = std::string("pkt_prover_arena_bytes failed: ") + pkt_create_error(), rc;
        total += inner;
    }
    *bytes = total;
    return PK_OK;
}

int pkx_prover_create(pk_ctx* ctx, const pkx_statement* stmt, pkx_prover** out) {
    auto stop = [](int rc, const std::string& reason) { return pkx::g_error = reason, rc; };
    return pk::create<pkx::Lib>(ctx, stmt, out, [&](std::unique_ptr<pkx_prover>& p) {
        p.reset(new pkx_prover());  // its destructor gives back what a return or a throw below leaves behind
        p->ctx = ctx;
        p->st = *stmt;
        p->pattern = pkx::io_pattern(*stmt);
        if (int rc = pk_ctx_sync(ctx)) return stop(rc, "pk_ctx_sync failed");  // also selects the context's device
        p->at = pkx::layout(*stmt);
        void* base = nullptr;
        if (int rc = pk_malloc(ctx, p->at.total, &base)) return stop(rc, "pk_malloc of the arena failed");
        p->arena = (uint8_t*)base;
        for (hipEvent_t& e : p->ev)
            if (hipEventCreate(&e) != hipSuccess) return stop(PK_ERR_HIP, "hipEventCreate failed");
        const pks_statement val = pkx::side_val(*stmt);
        if (int rc = pks_prover_create(ctx, &val, &p->val)) return stop(rc, std::string("pks_prover_create failed: ") + pks_create_error());
        if (int rc = pks_proof_bytes(&val, &p->side_bytes[PKX_SIDE_VAL])) return stop(rc, std::string("pks_proof_bytes failed: ") + pks_create_error());
        for (int side = PKX_SIDE_ROW; side <= PKX_SIDE_COL; side++) {
            const pkt_statement look = pkx::side_lookup(*stmt, side);
            if (int rc = pkt_prover_create(ctx, &look, &p->look[side - PKX_SIDE_ROW])) return stop(rc, std::string("pkt_prover_create failed: ") + pkt_create_error());
            if (int rc = pkt_proof_bytes(&look, &p->side_bytes[side])) return stop(rc, std::string("pkt_proof_bytes failed: ") + pkt_create_error());
        }
        if (int rc = pkx::iota_launch(nullptr, stmt->s > stmt->t ? stmt->s : stmt->t, p->iota(), 0)) return stop(rc, "the index column's launch failed");
        if (hipStreamSynchronize(nullptr) != hipSuccess) return stop(PK_ERR_HIP, "the index column's kernel failed");
        p->staging.resize(p->side_bytes[0] + p->side_bytes[1] + p->side_bytes[2]);
        return PK_OK;
    });
}

int pkx_prover_destroy(pkx_prover* p) { return pk::destroy(p); }

const char* pkx_last_error(const pkx_prover* p) { return p ? p->err.c_str() : "null prover"; }

int pkx_matrix(pkx_prover* p, const uint32_t* d_row_idx, const uint32_t* d_col_idx, uint64_t* d_row_out, uint64_t* d_col_out, uint64_t* d_m_row_out,
               uint64_t* d_m_col_out, uint64_t* first_bad) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkx_statement& st = p->st;
    if (first_bad) *first_bad = UINT64_MAX;
    if (!d_row_idx || !d_col_idx || !d_row_out || !d_col_out || !d_m_row_out || !d_m_col_out) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    try {
        // the caller's work on the context is finished before anything here reads its tables; the library's own launches go to the null stream
        if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
        (void)hipEventRecord(p->ev[0], nullptr);
        if (int rc = pkx::count_launch(nullptr, st.n, st.s, st.t, d_row_idx, d_col_idx, p->counts(0), p->counts(1), p->bad(), p->grid))
            return fail(p, rc, "the count kernels' launch failed");
        (void)hipEventRecord(p->ev[1], nullptr);
        // the counting pass validated every entry and wrote the arena only: with a bad entry nothing of the caller's is written
        if (int rc = bad_entry(p, first_bad)) return rc;
        if (int rc = pkx::columns_launch(nullptr, st.n, st.s, st.t, d_row_idx, d_col_idx, p->counts(0), p->counts(1), d_row_out, d_col_out, d_m_row_out, d_m_col_out,
                                         p->grid))
            return fail(p, rc, "the column kernels' launch failed");
        (void)hipEventRecord(p->ev[2], nullptr);
        if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(p, PK_ERR_HIP, "the column kernels failed");
        p->prof.count_ms = pk::between(p->ev[0], p->ev[1]), p->prof.columns_ms = pk::between(p->ev[1], p->ev[2]);
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

int pkx_begin(pkx_prover* p, const uint32_t* d_row_idx, const uint32_t* d_col_idx, const uint64_t* rx, const uint64_t* ry, uint64_t* d_e_row_out,
              uint64_t* d_e_col_out, uint64_t* first_bad) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkx_statement& st = p->st;
    if (first_bad) *first_bad = UINT64_MAX;
    if (!d_row_idx || !d_col_idx || !d_e_row_out || !d_e_col_out) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    if (int rc = point_ok(p, rx, ry)) return rc;
    try {
        if (int rc = eq_tables(p, rx, ry)) return rc;
        (void)hipEventRecord(p->ev[0], nullptr);
        if (int rc = pkx::gather_launch(nullptr, st.n, st.s, st.t, d_row_idx, d_col_idx, p->eq(0), p->eq(1), d_e_row_out, d_e_col_out, p->bad(), p->grid))
            return fail(p, rc, "the gather kernel's launch failed");
        (void)hipEventRecord(p->ev[1], nullptr);
        if (int rc = bad_entry(p, first_bad)) return rc;  // the copy follows the gather on the null stream
        p->prof.gather_ms = pk::between(p->ev[0], p->ev[1]);
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

int pkx_prove(pkx_prover* p, const uint64_t* const* cols, const uint64_t* rx, const uint64_t* ry, const uint64_t* bind, uint8_t* proof_out, size_t cap, size_t* len,
              uint64_t* value_out, pkx_claims* claims_out) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkx_statement& st = p->st;
    if (!cols || !len || (!proof_out && cap)) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    const size_t at[3] = {0, p->side_bytes[0], p->side_bytes[0] + p->side_bytes[1]}, need = at[2] + p->side_bytes[2];
    if (int rc = pk::proof_room_and_bind(p, need, cap, len, bind, st.n_bind)) return rc;
    if (int rc = point_ok(p, rx, ry)) return rc;
    try {
        for (int c = 0; c < PKX_COLUMNS; c++)
            if (!cols[c]) return fail(p, PK_ERR_BAD_ARG, "a column is NULL");
        pk::Transcript tr(p->pattern);
        for (unsigned i = 0; i < st.n_bind; i++) tr.add_scalar(pk::h_load(bind + 4 * i));
        for (unsigned i = 0; i < st.s; i++) tr.add_scalar(pk::h_load(rx + 4 * i));
        for (unsigned i = 0; i < st.t; i++) tr.add_scalar(pk::h_load(ry + 4 * i));
        fe seeds[3];
        tr.challenge_scalars(seeds, 3);
        if (!tr.finished()) return fail(p, PK_ERR_IO_PATTERN, "the transcript left its pattern: " + tr.violation());

        // the tables of the two lookups, rebuilt from the point: nothing of pkx_begin is kept
        auto t0 = std::chrono::steady_clock::now();
        if (int rc = eq_tables(p, rx, ry)) return rc;
        p->prof.eq_ms = host_ms_since(t0);

        // side VAL into the staging.  Nothing of proof_out is written yet
        fe z_val[PKX_MAX_VARS], finals[3];
        {
            const uint64_t* tables[3] = {cols[PKX_COL_VAL], cols[PKX_COL_E_ROW], cols[PKX_COL_E_COL]};
            size_t part = 0;
            t0 = std::chrono::steady_clock::now();
            const int rc = pks_prove(p->val, tables, nullptr, (const uint64_t*)seeds[PKX_SIDE_VAL].v, p->staging.data(), p->side_bytes[PKX_SIDE_VAL], &part,
                                     (uint64_t*)z_val, (uint64_t*)finals);
            p->prof.side_ms[PKX_SIDE_VAL] = host_ms_since(t0);
            if (rc) return fail(p, rc, std::string("side VAL's sumcheck failed: ") + pks_last_error(p->val));
        }
        // the two lookups: (index, e) in (I, eq(point, .)) under m
        pkt_claims look[2];
        for (int side = PKX_SIDE_ROW; side <= PKX_SIDE_COL; side++) {
            const bool row = side == PKX_SIDE_ROW;
            const uint64_t* f[2] = {cols[row ? PKX_COL_ROW : PKX_COL_COL], cols[row ? PKX_COL_E_ROW : PKX_COL_E_COL]};
            const uint64_t* table[2] = {p->iota(), p->eq(side - PKX_SIDE_ROW)};
            size_t part = 0;
            t0 = std::chrono::steady_clock::now();
            pkt_prover* inner = p->look[side - PKX_SIDE_ROW];
            const int rc = pkt_prove(inner, f, table, cols[row ? PKX_COL_M_ROW : PKX_COL_M_COL], (const uint64_t*)seeds[side].v, p->staging.data() + at[side],
                                     p->side_bytes[side], &part, &look[side - PKX_SIDE_ROW]);
            p->prof.side_ms[side] = host_ms_since(t0);
            if (rc == PK_ERR_UNSATISFIED)
                return fail(p, rc, std::string("side ") + SIDE_NAMES[side] + (row ? ": (row, e_row) is not a read of eq(rx, .) under m_row: " : ": (col, e_col) is not a read of eq(ry, .) under m_col: ") +
                                       pkt_last_error(inner));
            if (rc) return fail(p, rc, std::string("side ") + SIDE_NAMES[side] + "'s lookup failed: " + pkt_last_error(inner));
        }
        memcpy(proof_out, p->staging.data(), need);
        fe wire;
        memcpy(wire.v, p->staging.data(), 32);
        const fe value = pk::h_from_canon(wire);
        if (value_out) pk::put_fe(value_out, value);
        if (claims_out) pkx::fill_claims(st, value, z_val, finals, look, claims_out);
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

}  // extern "C"
