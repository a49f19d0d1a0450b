// provekit_rangecheck.hpp -- provekit::RangeCheck: the C++ face of libprovekit_rangecheck.so (include/provekit_rangecheck.h), next to
// provekit_tuplelookup.hpp's TupleLookup.  Prove that every entry of a device column is below 2^bits, bits up to 64, by limbs of k bits
// looked up in the identity table; `decompose` builds the limb columns and the multiplicities on the device; verify on the host.  An
// accepted proof is accepted PROVIDED the three claims of RangeClaims: WhirPcs::open / WhirPcs::verify give the evaluations of f and the
// limbs at z_lo and of m at z_t, RangeCheck::check_claims forms the combinations.  A rejected proof is a verdict, not an exception; only
// a failed call throws provekit::Error.
#pragma once
#include "provekit_hip.hpp"
#include "provekit_rangecheck.h"

namespace provekit {

struct RangeClaims {
    pkr_claims raw;                       // what check_claims reads
    std::vector<FieldElement> z_lo, z_t;  // the points, variable 0 first: f and every limb are opened at z_lo, m at z_t
    FieldElement limbs_value, m_value;
    static RangeClaims from(const pkr_statement& st, const pkr_claims& c) {
        auto fe = [](const uint64_t* p) { return FieldElement{p[0], p[1], p[2], p[3]}; };
        RangeClaims o;
        o.raw = c;
        o.limbs_value = fe(c.limbs_value), o.m_value = fe(c.m_value);
        for (unsigned i = 0; i < st.n; i++) o.z_lo.push_back(fe(c.z_lo[i]));
        for (unsigned i = 0; i < st.k; i++) o.z_t.push_back(fe(c.z_t[i]));
        return o;
    }
};

struct RangeProof {
    std::vector<uint8_t> proof;
    RangeClaims claims;
};

struct RangeVerdict {
    bool accepted;
    int check;  // PKV_CHECK_*, PKS_CHECK_*, PKF_CHECK_* or PKR_CHECK_TABLE
    int side;   // PKT_SIDE_*
    unsigned layer;
    uint64_t offset;
    std::string message;
    RangeClaims claims;  // when accepted
    const char* check_name() const { return pkr_check_name(check); }
    explicit operator bool() const { return accepted; }
};

class RangeCheck {
   public:
    // the plan of a statement; a statement the library does not take throws with its reason
    static pkr_limb_plan plan(const pkr_statement& st) {
        pkr_limb_plan p;
        if (int rc = pkr_plan(&st, &p)) throw Error(rc, pkr_create_error());
        return p;
    }

    RangeCheck(const Context& ctx, unsigned n, unsigned bits, unsigned k, unsigned n_bind = 0) : st_{n, bits, k, n_bind} {
        if (int rc = pkr_prover_create(ctx.get(), &st_, &p_)) throw Error(rc, pkr_create_error());
        plan_ = plan(st_);
    }
    ~RangeCheck() { pkr_prover_destroy(p_); }
    RangeCheck(const RangeCheck&) = delete;
    RangeCheck& operator=(const RangeCheck&) = delete;
    const pkr_statement& statement() const { return st_; }
    unsigned limbs() const { return plan_.limbs; }

    // f (2^n elements) -> the L limb columns (2^n elements each) and m (2^k elements).  An entry >= 2^bits throws with code
    // PK_ERR_UNSATISFIED; *first_bad: the smallest such entry
    void decompose(const DeviceVec& f, const std::vector<DeviceVec*>& limbs_out, DeviceVec& m, uint64_t* first_bad = nullptr) const {
        if (f.size() != (size_t)1 << st_.n || limbs_out.size() != plan_.limbs || m.size() != (size_t)1 << st_.k)
            throw Error(PK_ERR_BAD_ARG, "f has 2^n elements, there are L limb columns, m has 2^k elements");
        std::vector<uint64_t*> out;
        for (DeviceVec* v : limbs_out) {
            if (!v || v->size() != f.size()) throw Error(PK_ERR_BAD_ARG, "a limb column has 2^n elements");
            out.push_back(v->data());
        }
        if (int rc = pkr_decompose(p_, f.data(), out.data(), m.data(), first_bad)) throw Error(rc, pkr_last_error(p_));
    }

    // a limb outside 0 .. 2^k - 1, a top limb outside 0 .. 2^r - 1 or a wrong m throws with code PK_ERR_UNSATISFIED and a reason that names
    // the group and the entry; the prover stays usable
    RangeProof prove(const std::vector<const DeviceVec*>& limbs, const DeviceVec& m, const std::vector<FieldElement>& bind = {}) const {
        if (limbs.size() != plan_.limbs || m.size() != (size_t)1 << st_.k || bind.size() != st_.n_bind)
            throw Error(PK_ERR_BAD_ARG, "there are L limb columns, m has 2^k elements, bind the statement's count");
        std::vector<const uint64_t*> in;
        for (const DeviceVec* v : limbs) {
            if (!v || v->size() != (size_t)1 << st_.n) throw Error(PK_ERR_BAD_ARG, "a limb column has 2^n elements");
            in.push_back(v->data());
        }
        size_t len = 0;
        pkr_proof_bytes(&st_, &len);
        RangeProof out;
        out.proof.resize(len);
        pkr_claims c;
        if (int rc = pkr_prove(p_, in.data(), m.data(), bind.empty() ? nullptr : bind[0].data(), out.proof.data(), out.proof.size(), &len, &c))
            throw Error(rc, pkr_last_error(p_));
        out.claims = RangeClaims::from(st_, c);
        return out;
    }

    // host only
    static RangeVerdict verify(const pkr_statement& st, const std::vector<uint8_t>& proof, const std::vector<FieldElement>& bind = {}) {
        if (bind.size() != st.n_bind) throw Error(PK_ERR_BAD_ARG, "bind must have the statement's count");
        pkr_claims c;
        pkv_result r;
        int side = 0;
        unsigned layer = 0;
        const int rc = pkr_verify(&st, nullptr, 0, bind.empty() ? nullptr : bind[0].data(), proof.data(), proof.size(), &c, &side, &layer, &r);
        if (rc) throw Error(rc, pkr_create_error());
        RangeVerdict v{r.accepted != 0, r.check, side, layer, r.offset, r.message, {}};
        if (v.accepted) v.claims = RangeClaims::from(st, c);
        return v;
    }

    // host only: f_eval = f(z_lo), limb_evals[i] = limb_i(z_lo), m_eval = m(z_t) -> PKR_CLAIM_NONE when the three claims hold, else the
    // first that does not
    static int check_claims(const pkr_statement& st, const RangeClaims& claims, const FieldElement& f_eval, const std::vector<FieldElement>& limb_evals,
                            const FieldElement& m_eval) {
        if (limb_evals.size() != plan(st).limbs) throw Error(PK_ERR_BAD_ARG, "limb_evals has L elements");
        int which = -1;
        if (int rc = pkr_check_claims(&st, &claims.raw, f_eval.data(), limb_evals[0].data(), m_eval.data(), &which)) throw Error(rc, pkr_create_error());
        return which;
    }

   private:
    pkr_statement st_;
    pkr_limb_plan plan_{};
    pkr_prover* p_ = nullptr;
};

}  // namespace provekit
