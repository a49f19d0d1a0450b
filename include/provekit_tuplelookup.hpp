// provekit_tuplelookup.hpp -- provekit::TupleLookup: the C++ face of libprovekit_tuplelookup.so (include/provekit_tuplelookup.h), next
// to provekit_fracsum.hpp's GkrLookup.  Prove that every row of c groups of w device columns is a row of a table of w columns with
// given multiplicities -- ROM reads (addr, value), binop tables (a, b, a op b), several columns against one range table in one proof;
// verify on the host.  An accepted proof is accepted PROVIDED the three values of TupleLookupClaims: WhirPcs::open / WhirPcs::verify
// give the columns' evaluations, TupleLookup::check_claims forms the combinations.  A rejected proof is a verdict, not an exception;
// only a failed call throws provekit::Error.
#pragma once
#include "provekit_hip.hpp"
#include "provekit_tuplelookup.h"

namespace provekit {

struct TupleLookupClaims {
    pkt_claims raw;                                // what check_claims reads
    FieldElement alpha, beta;
    std::vector<FieldElement> z_lo, z_t;           // the points, variable 0 first: every f[g][j] is opened at z_lo, every t[j] and m at z_t
    FieldElement f_value, t_value, m_value;        // what the three combinations must be
    static TupleLookupClaims from(const pkt_statement& st, const pkt_claims& c) {
        auto fe = [](const uint64_t* p) { return FieldElement{p[0], p[1], p[2], p[3]}; };
        TupleLookupClaims o;
        o.raw = c;
        o.alpha = fe(c.alpha), o.beta = fe(c.beta), o.f_value = fe(c.f_value), o.t_value = fe(c.t_value), o.m_value = fe(c.m_value);
        for (unsigned i = 0; i < st.n; i++) o.z_lo.push_back(fe(c.z_lo[i]));
        for (unsigned i = 0; i < st.k; i++) o.z_t.push_back(fe(c.z_t[i]));
        return o;
    }
};

struct TupleLookupProof {
    std::vector<uint8_t> proof;
    TupleLookupClaims claims;
};

struct TupleLookupVerdict {
    bool accepted;
    int check;  // PKV_CHECK_*, PKS_CHECK_* or PKF_CHECK_*
    int side;   // PKT_SIDE_*
    unsigned layer;
    uint64_t offset;
    std::string message;
    TupleLookupClaims claims;  // when accepted
    const char* check_name() const { return pkt_check_name(check); }
    explicit operator bool() const { return accepted; }
};

class TupleLookup {
   public:
    using Columns = std::vector<const DeviceVec*>;  // one row's columns, j = 0 .. w - 1

    TupleLookup(const Context& ctx, unsigned n, unsigned k, unsigned w, unsigned c = 1, unsigned n_bind = 0) : st_{n, k, w, c, n_bind} {
        if (int rc = pkt_prover_create(ctx.get(), &st_, &p_)) throw Error(rc, pkt_create_error());
    }
    ~TupleLookup() { pkt_prover_destroy(p_); }
    TupleLookup(const TupleLookup&) = delete;
    TupleLookup& operator=(const TupleLookup&) = delete;
    const pkt_statement& statement() const { return st_; }

    // 2^n row numbers of t as a device column for `multiplicities`
    static DeviceVec indices(const Context& ctx, const std::vector<uint32_t>& idx) {
        DeviceVec d(ctx, (idx.size() * 4 + 31) / 32);
        if (!idx.empty()) ctx.check(pk_memcpy_h2d(ctx.get(), d.data(), idx.data(), 4 * idx.size()));
        return d;
    }

    // m[y] = how many rows of all groups are row y of t, into m (2^k elements); idx[g]: `indices` of group g's row numbers.  A row whose
    // index is outside t or that is not the row it names throws with code PK_ERR_UNSATISFIED; *first_bad: its stacked index
    void multiplicities(const std::vector<Columns>& f, const Columns& t, const std::vector<const DeviceVec*>& idx, DeviceVec& m, uint64_t* first_bad = nullptr) const {
        if (idx.size() != st_.c || m.size() != (size_t)1 << st_.k) throw Error(PK_ERR_BAD_ARG, "idx has c columns, m 2^k elements");
        const std::vector<const uint64_t*> pf = pointers(f, st_.c, st_.n), pt = pointers({t}, 1, st_.k);
        std::vector<const uint32_t*> pi;
        for (const DeviceVec* v : idx) pi.push_back(reinterpret_cast<const uint32_t*>(v->data()));
        if (int rc = pkt_multiplicities(p_, pf.data(), pt.data(), pi.data(), m.data(), first_bad)) throw Error(rc, pkt_last_error(p_));
    }

    // a row outside the table, a wrong m or an alpha that is a compressed row throws with code PK_ERR_UNSATISFIED and a reason that names
    // the case; the prover stays usable
    TupleLookupProof prove(const std::vector<Columns>& f, const Columns& t, const DeviceVec& m, const std::vector<FieldElement>& bind = {}) const {
        if (m.size() != (size_t)1 << st_.k || bind.size() != st_.n_bind) throw Error(PK_ERR_BAD_ARG, "m has 2^k elements, bind the statement's count");
        const std::vector<const uint64_t*> pf = pointers(f, st_.c, st_.n), pt = pointers({t}, 1, st_.k);
        size_t len = 0;
        pkt_proof_bytes(&st_, &len);
        TupleLookupProof out;
        out.proof.resize(len);
        pkt_claims c;
        if (int rc = pkt_prove(p_, pf.data(), pt.data(), m.data(), bind.empty() ? nullptr : bind[0].data(), out.proof.data(), out.proof.size(), &len, &c))
            throw Error(rc, pkt_last_error(p_));
        out.claims = TupleLookupClaims::from(st_, c);
        return out;
    }

    // host only
    static TupleLookupVerdict verify(const pkt_statement& st, const std::vector<uint8_t>& proof, const std::vector<FieldElement>& bind = {}) {
        if (bind.size() != st.n_bind) throw Error(PK_ERR_BAD_ARG, "bind must have the statement's count");
        pkt_claims c;
        pkv_result r;
        int side = 0;
        unsigned layer = 0;
        const int rc = pkt_verify(&st, nullptr, 0, bind.empty() ? nullptr : bind[0].data(), proof.data(), proof.size(), &c, &side, &layer, &r);
        if (rc) throw Error(rc, pkt_create_error());
        TupleLookupVerdict v{r.accepted != 0, r.check, side, layer, r.offset, r.message, {}};
        if (v.accepted) v.claims = TupleLookupClaims::from(st, c);
        return v;
    }

    // host only: f_evals[g * w + j] = f[g][j](z_lo), t_evals[j] = t[j](z_t), m_eval = m(z_t) -> PKT_CLAIM_NONE when the three claims hold,
    // else the first that does not
    static int check_claims(const pkt_statement& st, const TupleLookupClaims& claims, const std::vector<FieldElement>& f_evals, const std::vector<FieldElement>& t_evals,
                            const FieldElement& m_eval) {
        if (f_evals.size() != (size_t)st.c * st.w || t_evals.size() != st.w) throw Error(PK_ERR_BAD_ARG, "f_evals has c * w elements, t_evals w");
        int which = -1;
        if (int rc = pkt_check_claims(&st, &claims.raw, f_evals[0].data(), t_evals[0].data(), m_eval.data(), &which)) throw Error(rc, pkt_create_error());
        return which;
    }

   private:
    // the device pointers of `count` groups of w columns of 2^vars elements each
    std::vector<const uint64_t*> pointers(const std::vector<Columns>& groups, unsigned count, unsigned vars) const {
        if (groups.size() != count) throw Error(PK_ERR_BAD_ARG, "f has the statement's c groups");
        std::vector<const uint64_t*> out;
        for (const Columns& cols : groups) {
            if (cols.size() != st_.w) throw Error(PK_ERR_BAD_ARG, "a row has the statement's w columns");
            for (const DeviceVec* col : cols) {
                if (!col || col->size() != (size_t)1 << vars) throw Error(PK_ERR_BAD_ARG, "a column of f has 2^n elements, one of t 2^k");
                out.push_back(col->data());
            }
        }
        return out;
    }

    pkt_statement st_;
    pkt_prover* p_ = nullptr;
};

}  // namespace provekit
