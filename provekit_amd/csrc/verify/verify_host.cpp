// verify_host.cpp -- the host half of libprovekit_verify.so's C ABI: the statement and the host core.  No device code and no HIP
// call: this file and core.hpp are also what the sanitizer build (make asan) compiles, without the product library.
#include "verifier.hpp"

namespace {
thread_local std::string g_create_error;
const char* const kCheckNames[PKV_CHECK_COUNT] = {
    "NONE",          "TRANSCRIPT_SHORT", "NON_CANONICAL", "IO_PATTERN", "HINT_FORMAT", "OPENING_COUNT",   "MERKLE",         "ZK_SUMCHECK", "WHIR_SUMCHECK",
    "POW",           "STIR_INDICES",     "FINAL_POLY",    "WHIR_FINAL", "BLINDING_WEIGHT", "TRAILING_BYTES", "SPARTAN", "WITNESS_FIT", "MATRIX_EVAL"};
int create_fail(int rc, const std::string& why) {
    g_create_error = why;
    return rc;
}
}  // namespace

extern "C" {

int pkv_abi_version(void) { return 1; }

const char* pkv_check_name(int check) { return check >= 0 && check < PKV_CHECK_COUNT ? kCheckNames[check] : "UNKNOWN"; }

const char* pkv_create_error(void) { return g_create_error.c_str(); }

int pkv_verifier_create(unsigned m, unsigned m_0, const pk_whir_config* whir_witness, const pk_whir_config* whir_for_hiding_spartan,
                        const uint8_t* io_pattern, size_t io_pattern_len, int hash_version, pkv_verifier** out) {
    if (out) *out = nullptr;
    if (!out || !whir_witness || !whir_for_hiding_spartan) return create_fail(PK_ERR_BAD_ARG, "null pointer");
    try {
        pkv_verifier* v = new pkv_verifier();
        pkv::Statement& st = v->st;
        st.m = m;
        st.m_0 = m_0;
        st.w = *whir_witness;
        st.b = *whir_for_hiding_spartan;
        st.hash_version = hash_version;
        std::string why;
        if (!pkv::statement_ok(st, why)) {
            delete v;
            return create_fail(PK_ERR_BAD_ARG, why);
        }
        if (io_pattern && io_pattern_len) {
            st.pattern.assign(reinterpret_cast<const char*>(io_pattern), io_pattern_len);
        } else {
#ifdef PKV_HOST_ONLY
            delete v;
            return create_fail(PK_ERR_BAD_ARG, "this build has no IO pattern of its own: pass the bytes");
#else
            size_t n = 0;
            int rc = pk_whir_r1cs_io_pattern(m_0, &st.w, &st.b, nullptr, 0, &n);
            if (!rc) {
                st.pattern.resize(n);
                rc = pk_whir_r1cs_io_pattern(m_0, &st.w, &st.b, reinterpret_cast<uint8_t*>(&st.pattern[0]), n, &n);
            }
            if (rc) {
                delete v;
                return create_fail(rc, "pk_whir_r1cs_io_pattern refuses this scheme shape");
            }
#endif
        }
        if (!pk::io_pattern_parse(st.pattern, st.ops, why)) {
            delete v;
            return create_fail(PK_ERR_IO_PATTERN, why);
        }
        *out = v;
        g_create_error.clear();
        return PK_OK;
    } catch (...) {
        return create_fail(PK_ERR_OOM, "out of memory");
    }
}

int pkv_verifier_destroy(pkv_verifier* v) {
    if (!v) return PK_OK;
    if (v->dev_release) v->dev_release(v);
    delete v;
    return PK_OK;
}

const char* pkv_last_error(const pkv_verifier* v) { return v ? v->err.c_str() : "null verifier"; }

int pkv_verifier_set_r1cs(pkv_verifier* v, size_t num_constraints, size_t num_witnesses, const pk_sparse_matrix mats[3], const uint64_t* interner,
                          size_t n_interned) {
    if (!v) return PK_ERR_BAD_ARG;
    auto bad = [&](const char* why) {
        v->err = why;
        return PK_ERR_BAD_ARG;
    };
    if (!mats || (n_interned && !interner)) return bad("null pointer");
    if (v->dev) return bad("attach the R1CS before the device");
    if (num_constraints > ((size_t)1 << v->st.m_0)) return bad("more constraints than 2^m_0");
    if (num_witnesses > ((size_t)1 << 28)) return bad("too many witnesses");
    try {
        pkv::Statement& st = v->st;
        std::vector<uint32_t> rows[3], cols[3], vals[3];
        for (int k = 0; k < 3; k++) {
            const pk_sparse_matrix& M = mats[k];
            if (M.nnz > UINT32_MAX) return bad("too many entries");
            if ((num_constraints && !M.new_row_indices) || (M.nnz && (!M.col_indices || !M.values))) return bad("null pointer");
            rows[k].resize(M.nnz);
            cols[k].assign(M.col_indices, M.col_indices + M.nnz);
            vals[k].assign(M.values, M.values + M.nnz);
            for (size_t r = 0; r < num_constraints; r++) {
                const size_t lo = M.new_row_indices[r], hi = r + 1 < num_constraints ? M.new_row_indices[r + 1] : M.nnz;
                if (lo > hi || hi > M.nnz || (r == 0 && lo != 0)) return bad("new_row_indices must be non-decreasing offsets into the entries, starting at 0");
                for (size_t e = lo; e < hi; e++) rows[k][e] = (uint32_t)r;
            }
            if (!num_constraints && M.nnz) return bad("entries without rows");
            for (size_t e = 0; e < M.nnz; e++)
                if (cols[k][e] >= num_witnesses || vals[k][e] >= n_interned) return bad("column or value index out of range");
        }
        st.interner.resize(n_interned);
        if (n_interned) memcpy(st.interner.data(), interner, 32 * n_interned);
        for (int k = 0; k < 3; k++) {
            st.rows[k].swap(rows[k]);
            st.cols[k].swap(cols[k]);
            st.vals[k].swap(vals[k]);
        }
        st.nc = num_constraints;
        st.nw = num_witnesses;
        st.has_r1cs = true;
        return PK_OK;
    } catch (...) {
        v->err = "out of memory";
        return PK_ERR_OOM;
    }
}

int pkv_verify(pkv_verifier* v, const uint8_t* proof, size_t len, pkv_result* result) {
    if (!v) return PK_ERR_BAD_ARG;
    if (!result || (len && !proof)) {
        v->err = "null pointer";
        return PK_ERR_BAD_ARG;
    }
    try {
        static const uint8_t none = 0;
        pkv::verify_host(v->st, len ? proof : &none, len, result);
        return PK_OK;
    } catch (...) {
        v->err = "out of memory";
        return PK_ERR_OOM;
    }
}

}  // extern "C"
