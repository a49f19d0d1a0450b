// verify_host.cpp -- the host half of libprovekit_spark.so's C ABI: the statement's rules, the outer IO pattern, the verifier with its
// table check, the claims' combinations and the stacked flattening of an R1CS.  No device code and no HIP call; of other libraries it
// calls pks_verify, pkt_verify, the lengths, pkf_check_name and the creation errors.  This file and its headers are also what the
// sanitizer build (make asan, spark/asan_main.cpp) compiles, next to the three host verifiers below it.
#include <vector>

#include "layout.hpp"

namespace pkx {
thread_local std::string g_error;
}

namespace {

using pk::fe;
using pk::verdict;

// the three parts' lengths; an inner refusal of a statement this library made is passed on with its reason
int side_bytes(const pkx_statement& st, size_t out[3]) {
    const pks_statement val = pkx::side_val(st);
    if (int rc = pks_proof_bytes(&val, &out[PKX_SIDE_VAL])) return pkx::g_error = pks_create_error(), rc;
    for (int side = PKX_SIDE_ROW; side <= PKX_SIDE_COL; side++) {
        const pkt_statement look = pkx::side_lookup(st, side);
        if (int rc = pkt_proof_bytes(&look, &out[side])) return pkx::g_error = pkt_create_error(), rc;
    }
    return PK_OK;
}

// The outer transcript absorbs bind, rx and ry and squeezes the three seeds.  false: the verdict (offset 0: nothing of the proof was
// read) is in *result
bool outer(const pkv::Statement& ps, const pkx_statement& st, const uint64_t* bind, const uint64_t* rx, const uint64_t* ry, fe* r_row, fe* r_col, fe seeds[3],
           pkv_result* result) {
    std::vector<uint8_t> bytes;
    pk::put_canonical(bytes, bind, st.n_bind), pk::put_canonical(bytes, rx, st.s), pk::put_canonical(bytes, ry, st.t);
    pkv::Verdict v;
    pkv::Arthur A(ps, bytes.data(), bytes.size(), v);
    std::vector<fe> scratch(st.n_bind);
    bool walked = !st.n_bind || A.next_scalars(st.n_bind, scratch.data());
    walked = walked && A.next_scalars(st.s, r_row) && A.next_scalars(st.t, r_col) && A.challenge_scalars(3, seeds);
    walked = walked && (A.done() || A.fail(PKV_CHECK_IO_PATTERN, "declared operations left after the outer transcript"));
    if (walked) return true;
    v.offset = 0;
    pkv::to_result(v, result);
    return false;
}

}  // namespace

extern "C" {

int pkx_abi_version(void) { return 1; }

const char* pkx_check_name(int check) { return check == PKX_CHECK_TABLE ? "TABLE" : pkf_check_name(check); }

const char* pkx_create_error(void) { return pkx::g_error.c_str(); }

unsigned pkx_count_lds_max(void) { return pkx::COUNT_LDS_MAX; }

int pkx_io_pattern(const pkx_statement* stmt, uint8_t* buf, size_t cap, size_t* len) { return pk::pattern_out<pkx::Lib>(stmt, buf, cap, len); }

int pkx_proof_bytes(const pkx_statement* stmt, size_t* len) {
    std::string why;
    if (!len) return pkx::refuse("null pointer");
    if (!pkx::statement_ok(stmt, why)) return pkx::refuse(why);
    size_t part[3];
    if (int rc = side_bytes(*stmt, part)) return rc;
    *len = part[0] + part[1] + part[2];
    return PK_OK;
}

int pkx_verify(const pkx_statement* stmt, const uint8_t* io_pattern_or_null, size_t io_pattern_len, const uint64_t* rx, const uint64_t* ry, const uint64_t* bind,
               const uint64_t* expected_value_or_null, const uint8_t* proof, size_t len, pkx_claims* claims_out, int* side_out, unsigned* layer_out, pkv_result* result) {
    std::string why;
    if (!result || (!proof && len)) return pkx::refuse("null pointer");
    if (!pkx::statement_ok(stmt, why)) return pkx::refuse(why);
    const pkx_statement& st = *stmt;
    if (!rx || !ry) return pkx::refuse("the point (rx, ry) is the statement: pass it");
    if (st.n_bind && !bind) return pkx::refuse("the statement binds elements: pass them");
    if (!pkx::elements_below_p(bind, st.n_bind, "bind", why) || !pkx::elements_below_p(rx, st.s, "rx", why) || !pkx::elements_below_p(ry, st.t, "ry", why) ||
        !pkx::elements_below_p(expected_value_or_null, expected_value_or_null ? 1 : 0, "expected_value", why))
        return pkx::refuse(why);
    try {
        pkv::Statement ps;
        if (int rc = pk::parse_pattern(ps, io_pattern_or_null, io_pattern_len, pkx::io_pattern(st), pkx::g_error)) return rc;
        size_t part[3];
        if (int rc = side_bytes(st, part)) return rc;
        const size_t at[3] = {0, part[0], part[0] + part[1]}, total = at[2] + part[2];
        // where a verdict points: the side and the layer it is about
        auto about = [&](int side, unsigned layer) {
            if (side_out) *side_out = side;
            if (layer_out) *layer_out = layer;
        };
        about(PKX_SIDE_VAL, 0);
        // framing first: all three parts have a fixed length, so a proof of another length is judged before any part is read
        if (len < total) return verdict(result, PKV_CHECK_TRANSCRIPT_SHORT, len, "the proof is shorter than its three parts"), PK_OK;
        if (len > total) return verdict(result, PKV_CHECK_TRAILING_BYTES, total, "bytes left after the proof"), PK_OK;
        fe point[2][PKX_MAX_VARS], seeds[3];
        if (!outer(ps, st, bind, rx, ry, point[0], point[1], seeds, result)) return PK_OK;

        const pks_statement val = pkx::side_val(st);
        fe z_val[PKX_MAX_VARS], finals[3];
        if (int rc = pks_verify(&val, nullptr, 0, nullptr, (const uint64_t*)seeds[PKX_SIDE_VAL].v, expected_value_or_null, proof, part[PKX_SIDE_VAL], (uint64_t*)z_val,
                                (uint64_t*)finals, result))
            return pkx::g_error = pks_create_error(), rc;
        if (!result->accepted) return PK_OK;
        fe wire;  // canonical on the wire, and below p: the walk accepted it
        memcpy(wire.v, proof, 32);
        const fe value = pk::h_from_canon(wire);

        pkt_claims look[2];
        for (int side = PKX_SIDE_ROW; side <= PKX_SIDE_COL; side++) {
            const pkt_statement ls = pkx::side_lookup(st, side);
            pkt_claims& seen = look[side - PKX_SIDE_ROW];
            unsigned layer = 0;
            if (int rc = pkt_verify(&ls, nullptr, 0, (const uint64_t*)seeds[side].v, proof + at[side], part[side], &seen, nullptr, &layer, result))
                return pkx::g_error = pkt_create_error(), rc;
            result->offset += at[side];
            about(side, layer);
            if (!result->accepted) return PK_OK;
            about(side, 0);
            fe y[PKX_MAX_VARS];
            for (unsigned i = 0; i < ls.k; i++) y[i] = pk::h_load(seen.z_t[i]);
            if (!pk::fe_eq(pk::h_load(seen.t_value), pkx::table_at(point[side - PKX_SIDE_ROW], pk::h_load(seen.beta), y, ls.k)))
                return verdict(result, PKX_CHECK_TABLE, at[side] + part[side],
                               side == PKX_SIDE_ROW ? "side ROW's table claim is not I(y) + beta eq(rx, y): its table is not (0 .. 2^s - 1, eq(rx, .))"
                                                    : "side COL's table claim is not I(y) + beta eq(ry, y): its table is not (0 .. 2^t - 1, eq(ry, .))"),
                       PK_OK;
        }
        verdict(result, PKV_CHECK_NONE, total, "");
        about(PKX_SIDE_VAL, 0);
        if (claims_out) pkx::fill_claims(st, value, z_val, finals, look, claims_out);
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

int pkx_check_claims(const pkx_statement* stmt, const pkx_claims* claims, const uint64_t* val_evals, const uint64_t* row_evals, const uint64_t* m_row_eval,
                     const uint64_t* col_evals, const uint64_t* m_col_eval, int* which_out) {
    std::string why;
    if (!claims || !val_evals || !row_evals || !m_row_eval || !col_evals || !m_col_eval || !which_out) return pkx::refuse("null pointer");
    if (!pkx::statement_ok(stmt, why)) return pkx::refuse(why);
    if (!pkx::elements_below_p(val_evals, 3, "val_evals", why) || !pkx::elements_below_p(row_evals, 2, "row_evals", why) ||
        !pkx::elements_below_p(m_row_eval, 1, "m_row_eval", why) || !pkx::elements_below_p(col_evals, 2, "col_evals", why) ||
        !pkx::elements_below_p(m_col_eval, 1, "m_col_eval", why) || !pkx::elements_below_p(&claims->value[0], sizeof *claims / 32, "claims", why))
        return pkx::refuse(why);
    const uint64_t* f_evals[2] = {row_evals, col_evals};
    const uint64_t* m_evals[2] = {m_row_eval, m_col_eval};
    *which_out = PKX_CLAIM_NONE;
    for (int j = 2; j >= 0; j--)
        if (!pk::fe_eq(pk::h_load(val_evals + 4 * j), pk::h_load(claims->val_values[j]))) *which_out = PKX_CLAIM_VAL + j;
    if (*which_out != PKX_CLAIM_NONE) return PK_OK;
    for (int side = 0; side < 2; side++) {
        fe sum = pk::fe_zero();
        for (unsigned j = 0; j < 2; j++) sum = pk::h_add(sum, pk::h_mul(pk::h_load(claims->f_coeff[side][j]), pk::h_load(f_evals[side] + 4 * j)));
        if (!pk::fe_eq(sum, pk::h_load(claims->f_value[side]))) return *which_out = side ? PKX_CLAIM_COL : PKX_CLAIM_ROW, PK_OK;
        if (!pk::fe_eq(pk::h_load(m_evals[side]), pk::h_load(claims->m_value[side]))) return *which_out = side ? PKX_CLAIM_M_COL : PKX_CLAIM_M_ROW, PK_OK;
    }
    return PK_OK;
}

int pkx_entries_from_r1cs(size_t num_constraints, size_t num_witnesses, const pk_sparse_matrix mats[3], const uint64_t* interner, size_t n_interned, unsigned n,
                          unsigned s, unsigned t, uint32_t* row_idx_out, uint32_t* col_idx_out, uint64_t* val_out) {
    if (!mats || !interner || !row_idx_out || !col_idx_out || !val_out) return pkx::refuse("null pointer");
    const pkx_statement query{n, s + 2, t, 0};
    std::string why;
    if (s + 2 < s || !pkx::statement_ok(&query, why)) return pkx::refuse("the stacked statement (n, s + 2, t): " + (why.empty() ? std::string("s must be 1..26") : why));
    if (s < 1) return pkx::refuse("s must be 1..26");
    const size_t entries = (size_t)1 << n, rows = (size_t)1 << s, cols = (size_t)1 << t;
    if (num_constraints > rows) return pkx::refuse("2^s is below the number of constraints");
    if (num_witnesses > cols) return pkx::refuse("2^t is below the number of witnesses");
    size_t nnz = 0;
    for (int g = 0; g < 3; g++) {
        if (mats[g].nnz > entries - nnz) return pkx::refuse("2^n is below the three matrices' non-zeros");
        if (mats[g].nnz && (!mats[g].col_indices || !mats[g].values)) return pkx::refuse("null pointer in matrix " + std::to_string(g));
        if (num_constraints && !mats[g].new_row_indices) return pkx::refuse("null pointer in matrix " + std::to_string(g));
        nnz += mats[g].nnz;
    }
    // everything is checked before anything is written
    for (int g = 0; g < 3; g++) {
        const pk_sparse_matrix& m = mats[g];
        for (size_t r = 0; r < num_constraints; r++) {
            const size_t from = m.new_row_indices[r], to = r + 1 < num_constraints ? m.new_row_indices[r + 1] : m.nnz;
            if (from > to || to > m.nnz) return pkx::refuse("matrix " + std::to_string(g) + ", row " + std::to_string(r) + ": its offset decreases or exceeds nnz");
        }
        if (num_constraints && m.new_row_indices[0] != 0) return pkx::refuse("matrix " + std::to_string(g) + ": its first row does not start at 0");
        for (size_t k = 0; k < m.nnz; k++) {
            if (m.col_indices[k] >= num_witnesses) return pkx::refuse("matrix " + std::to_string(g) + ", entry " + std::to_string(k) + ": its column is outside the witnesses");
            if (m.values[k] >= n_interned) return pkx::refuse("matrix " + std::to_string(g) + ", entry " + std::to_string(k) + ": its value index is outside the interner");
        }
    }
    if (!pkx::elements_below_p(interner, n_interned, "interner", why)) return pkx::refuse(why);
    size_t k = 0;
    for (int g = 0; g < 3; g++) {
        const pk_sparse_matrix& m = mats[g];
        for (size_t r = 0; r < num_constraints; r++) {
            const size_t to = r + 1 < num_constraints ? m.new_row_indices[r + 1] : m.nnz;
            for (size_t e = m.new_row_indices[r]; e < to; e++, k++) {
                row_idx_out[k] = (uint32_t)((size_t)g * rows + r);
                col_idx_out[k] = m.col_indices[e];
                memcpy(val_out + 4 * k, interner + 4 * (size_t)m.values[e], 32);
            }
        }
    }
    for (; k < entries; k++) {
        row_idx_out[k] = 0, col_idx_out[k] = 0;
        memset(val_out + 4 * k, 0, 32);
    }
    return PK_OK;
}

}  // extern "C"
