// provekit_spark.hpp -- provekit::Spark: the C++ face of libprovekit_spark.so (include/provekit_spark.h), next to
// provekit_memcheck.hpp's MemCheck.  Turn a sparse matrix's entry list into its committed columns on the device, gather a query's
// columns, prove M~(rx, ry) = v and verify on the host.  An accepted proof is accepted PROVIDED the nine values of SparkClaims:
// WhirPcs::open / WhirPcs::verify give the columns' evaluations, Spark::check_claims forms the combinations.  A rejected proof is a
// verdict, not an exception; only a failed call throws provekit::Error.
#pragma once
#include "provekit_hip.hpp"
#include "provekit_spark.h"

namespace provekit {

struct SparkClaims {
    pkx_claims raw;  // what check_claims reads
    FieldElement value;
    std::vector<FieldElement> z_val, z_row, z_col, y_row, y_col;  // the five points, variable 0 first
    static SparkClaims from(const pkx_statement& st, const pkx_claims& c) {
        auto fe = [](const uint64_t* p) { return FieldElement{p[0], p[1], p[2], p[3]}; };
        SparkClaims o;
        o.raw = c;
        o.value = fe(c.value);
        for (unsigned i = 0; i < st.n; i++) o.z_val.push_back(fe(c.z_val[i])), o.z_row.push_back(fe(c.z_f[0][i])), o.z_col.push_back(fe(c.z_f[1][i]));
        for (unsigned i = 0; i < st.s; i++) o.y_row.push_back(fe(c.z_m[0][i]));
        for (unsigned i = 0; i < st.t; i++) o.y_col.push_back(fe(c.z_m[1][i]));
        return o;
    }
};

struct SparkProof {
    std::vector<uint8_t> proof;
    FieldElement value;  // v = M~(rx, ry)
    SparkClaims claims;
};

struct SparkVerdict {
    bool accepted;
    int check;  // PKV_CHECK_*, PKS_CHECK_*, PKF_CHECK_* or PKX_CHECK_*
    int side;   // PKX_SIDE_*
    unsigned layer;
    uint64_t offset;
    std::string message;
    SparkClaims claims;  // when accepted
    const char* check_name() const { return pkx_check_name(check); }
    explicit operator bool() const { return accepted; }
};

// the seven device columns of a query
struct SparkColumns {
    const DeviceVec *row, *col, *val, *m_row, *m_col, *e_row, *e_col;
};

// an R1CS's three matrices as one stacked entry list of 2^n entries: the statement of its query is (n, s + 2, t)
struct SparkEntries {
    std::vector<uint32_t> row_idx, col_idx;
    std::vector<FieldElement> val;
};

class Spark {
   public:
    Spark(const Context& ctx, unsigned n, unsigned s, unsigned t, unsigned n_bind = 0) : st_{n, s, t, n_bind} {
        if (int rc = pkx_prover_create(ctx.get(), &st_, &p_)) throw Error(rc, pkx_create_error());
    }
    ~Spark() { pkx_prover_destroy(p_); }
    Spark(const Spark&) = delete;
    Spark& operator=(const Spark&) = delete;
    const pkx_statement& statement() const { return st_; }

    // 2^n indices as a device column for `matrix` and `begin`
    static DeviceVec indices(const Context& ctx, const std::vector<uint32_t>& idx) {
        DeviceVec d(ctx, (idx.size() * 4 + 31) / 32);
        if (!idx.empty()) ctx.check(pk_memcpy_h2d(ctx.get(), d.data(), idx.data(), 4 * idx.size()));
        return d;
    }

    // host only; interner: Montgomery
    static SparkEntries entries_from_r1cs(size_t num_constraints, size_t num_witnesses, const pk_sparse_matrix mats[3], const std::vector<FieldElement>& interner, unsigned n,
                                          unsigned s, unsigned t) {
        if (n > PKX_MAX_VARS) throw Error(PK_ERR_BAD_ARG, "n must be 1..28");
        SparkEntries e;
        e.row_idx.resize((size_t)1 << n), e.col_idx.resize((size_t)1 << n), e.val.resize((size_t)1 << n);
        if (int rc = pkx_entries_from_r1cs(num_constraints, num_witnesses, mats, interner.empty() ? nullptr : interner[0].data(), interner.size(), n, s, t,
                                           e.row_idx.data(), e.col_idx.data(), e.val[0].data()))
            throw Error(rc, pkx_create_error());
        return e;
    }

    // once per matrix: row, col (2^n elements), m_row (2^s), m_col (2^t).  An index outside the matrix throws with code PK_ERR_BAD_ARG;
    // *first_bad: the smallest such entry; nothing is written then
    void matrix(const DeviceVec& row_idx, const DeviceVec& col_idx, DeviceVec& row, DeviceVec& col, DeviceVec& m_row, DeviceVec& m_col, uint64_t* first_bad = nullptr) const {
        const size_t N = (size_t)1 << st_.n;
        if (row_idx.size() * 32 < 4 * N || col_idx.size() * 32 < 4 * N || row.size() != N || col.size() != N || m_row.size() != (size_t)1 << st_.s ||
            m_col.size() != (size_t)1 << st_.t)
            throw Error(PK_ERR_BAD_ARG, "the entry columns have 2^n elements, m_row 2^s, m_col 2^t");
        if (int rc = pkx_matrix(p_, reinterpret_cast<const uint32_t*>(row_idx.data()), reinterpret_cast<const uint32_t*>(col_idx.data()), row.data(), col.data(),
                                m_row.data(), m_col.data(), first_bad))
            throw Error(rc, pkx_last_error(p_));
    }

    // per query: e_row[k] = eq(rx, row_idx[k]), e_col[k] = eq(ry, col_idx[k])
    void begin(const DeviceVec& row_idx, const DeviceVec& col_idx, const std::vector<FieldElement>& rx, const std::vector<FieldElement>& ry, DeviceVec& e_row,
               DeviceVec& e_col, uint64_t* first_bad = nullptr) const {
        const size_t N = (size_t)1 << st_.n;
        if (rx.size() != st_.s || ry.size() != st_.t) throw Error(PK_ERR_BAD_ARG, "rx has s coordinates, ry has t");
        if (row_idx.size() * 32 < 4 * N || col_idx.size() * 32 < 4 * N || e_row.size() != N || e_col.size() != N)
            throw Error(PK_ERR_BAD_ARG, "the entry columns have 2^n elements");
        if (int rc = pkx_begin(p_, reinterpret_cast<const uint32_t*>(row_idx.data()), reinterpret_cast<const uint32_t*>(col_idx.data()), rx[0].data(), ry[0].data(),
                               e_row.data(), e_col.data(), first_bad))
            throw Error(rc, pkx_last_error(p_));
    }

    // columns that are not a read of the eq tables throw with code PK_ERR_UNSATISFIED and a reason that names the side; the prover stays usable
    SparkProof prove(const SparkColumns& cols, const std::vector<FieldElement>& rx, const std::vector<FieldElement>& ry, const std::vector<FieldElement>& bind = {}) const {
        if (bind.size() != st_.n_bind) throw Error(PK_ERR_BAD_ARG, "bind has the statement's count");
        if (rx.size() != st_.s || ry.size() != st_.t) throw Error(PK_ERR_BAD_ARG, "rx has s coordinates, ry has t");
        const size_t N = (size_t)1 << st_.n;
        for (const DeviceVec* v : {cols.row, cols.col, cols.val, cols.e_row, cols.e_col})
            if (!v || v->size() != N) throw Error(PK_ERR_BAD_ARG, "an entry column has 2^n elements");
        if (!cols.m_row || cols.m_row->size() != (size_t)1 << st_.s || !cols.m_col || cols.m_col->size() != (size_t)1 << st_.t)
            throw Error(PK_ERR_BAD_ARG, "m_row has 2^s elements, m_col 2^t");
        const uint64_t* raw[PKX_COLUMNS] = {cols.row->data(), cols.col->data(), cols.val->data(), cols.m_row->data(), cols.m_col->data(), cols.e_row->data(), cols.e_col->data()};
        size_t len = 0;
        pkx_proof_bytes(&st_, &len);
        SparkProof out;
        out.proof.resize(len);
        pkx_claims c;
        if (int rc = pkx_prove(p_, raw, rx[0].data(), ry[0].data(), bind.empty() ? nullptr : bind[0].data(), out.proof.data(), out.proof.size(), &len, out.value.data(), &c))
            throw Error(rc, pkx_last_error(p_));
        out.claims = SparkClaims::from(st_, c);
        return out;
    }

    // host only; expected_value NULL: any v is taken
    static SparkVerdict verify(const pkx_statement& st, const std::vector<uint8_t>& proof, const std::vector<FieldElement>& rx, const std::vector<FieldElement>& ry,
                               const std::vector<FieldElement>& bind = {}, const FieldElement* expected_value = nullptr) {
        if (bind.size() != st.n_bind) throw Error(PK_ERR_BAD_ARG, "bind must have the statement's count");
        if (rx.size() != st.s || ry.size() != st.t) throw Error(PK_ERR_BAD_ARG, "rx has s coordinates, ry has t");
        pkx_claims c;
        pkv_result r;
        int side = 0;
        unsigned layer = 0;
        const int rc = pkx_verify(&st, nullptr, 0, rx.empty() ? nullptr : rx[0].data(), ry.empty() ? nullptr : ry[0].data(), bind.empty() ? nullptr : bind[0].data(),
                                  expected_value ? expected_value->data() : nullptr, proof.data(), proof.size(), &c, &side, &layer, &r);
        if (rc) throw Error(rc, pkx_create_error());
        SparkVerdict v{r.accepted != 0, r.check, side, layer, r.offset, r.message, {}};
        if (v.accepted) v.claims = SparkClaims::from(st, c);
        return v;
    }

    // host only: val_evals = (val, e_row, e_col)(z_val), row_evals = (row, e_row)(z_row), m_row_eval = m_row(y_row), col_evals = (col,
    // e_col)(z_col), m_col_eval = m_col(y_col) -> PKX_CLAIM_NONE when all hold, else the first that does not
    static int check_claims(const pkx_statement& st, const SparkClaims& claims, const std::vector<FieldElement>& val_evals, const std::vector<FieldElement>& row_evals,
                            const FieldElement& m_row_eval, const std::vector<FieldElement>& col_evals, const FieldElement& m_col_eval) {
        if (val_evals.size() != 3 || row_evals.size() != 2 || col_evals.size() != 2) throw Error(PK_ERR_BAD_ARG, "val_evals has 3 elements, row_evals and col_evals 2");
        int which = -1;
        if (int rc = pkx_check_claims(&st, &claims.raw, val_evals[0].data(), row_evals[0].data(), m_row_eval.data(), col_evals[0].data(), m_col_eval.data(), &which))
            throw Error(rc, pkx_create_error());
        return which;
    }

   private:
    pkx_statement st_;
    pkx_prover* p_ = nullptr;
};

}  // namespace provekit
