// provekit_lookup.hpp -- provekit::Lookup: the C++ face of libprovekit_lookup.so (include/provekit_lookup.h), next to
// provekit_sumcheck.hpp's ProductSumcheck.  Prove that every entry of a device column f occurs in a device table t (LogUp); verify on
// the host.  An accepted proof is accepted PROVIDED the seven evaluation claims of LookupClaims hold: WhirPcs::open / WhirPcs::verify
// establish them for committed tables.  A rejected proof is a verdict, not an exception; only a failed call throws provekit::Error.
#pragma once
#include "provekit_hip.hpp"
#include "provekit_lookup.h"

namespace provekit {

struct LookupClaims {
    FieldElement alpha, s;
    std::vector<FieldElement> r_f, r_t;  // the points, variable 0 first
    FieldElement hf_at_rf, f_at_rf, ht_at_rt, t_at_rt, m_at_rt, hf_at_half, ht_at_half;
    static LookupClaims from(const pkl_statement& st, const pkl_claims& c) {
        auto fe = [](const uint64_t* p) { return FieldElement{p[0], p[1], p[2], p[3]}; };
        LookupClaims o;
        o.alpha = fe(c.alpha), o.s = fe(c.s);
        for (unsigned i = 0; i < st.n; i++) o.r_f.push_back(fe(c.r_f[i]));
        for (unsigned i = 0; i < st.k; i++) o.r_t.push_back(fe(c.r_t[i]));
        o.hf_at_rf = fe(c.hf_at_rf), o.f_at_rf = fe(c.f_at_rf), o.ht_at_rt = fe(c.ht_at_rt), o.t_at_rt = fe(c.t_at_rt), o.m_at_rt = fe(c.m_at_rt);
        o.hf_at_half = fe(c.hf_at_half), o.ht_at_half = fe(c.ht_at_half);
        return o;
    }
};

struct LookupVerdict {
    bool accepted;
    int check;        // PKV_CHECK_* or PKS_CHECK_*
    int side;         // PKL_SIDE_*
    uint64_t offset;  // bytes of the proof consumed
    std::string message;
    LookupClaims claims;  // when accepted
    const char* check_name() const { return pks_check_name(check); }
    explicit operator bool() const { return accepted; }
};

struct LookupHelpers {
    FieldElement alpha;
    const uint64_t* h_f;  // 2^n elements in the prover's arena, valid until the next begin()
    const uint64_t* h_t;  // 2^k elements
};

struct LookupProof {
    std::vector<uint8_t> proof;
    LookupClaims claims;
};

class Lookup {
   public:
    Lookup(const Context& ctx, unsigned n, unsigned k, unsigned n_bind = 0, unsigned n_bind2 = 0) : st_{n, k, n_bind, n_bind2} {
        if (int rc = pkl_prover_create(ctx.get(), &st_, &p_)) throw Error(rc, pkl_create_error());
    }
    ~Lookup() { pkl_prover_destroy(p_); }
    Lookup(const Lookup&) = delete;
    Lookup& operator=(const Lookup&) = delete;
    const pkl_statement& statement() const { return st_; }

    // step 1: writes m (2^k elements), which stays valid and unchanged until finish().  A failed validation throws with code
    // PK_ERR_UNSATISFIED after storing the smallest bad x in *first_bad (if given)
    void multiplicities(const DeviceVec& f, const DeviceVec& t, const uint32_t* d_idx, DeviceVec& m_out, uint64_t* first_bad = nullptr) const {
        if (f.size() != (size_t)1 << st_.n || t.size() != (size_t)1 << st_.k || m_out.size() != t.size()) throw Error(PK_ERR_BAD_ARG, "f has 2^n elements, t and m 2^k");
        uint64_t bad = 0;
        const int rc = pkl_multiplicities(p_, f.data(), t.data(), d_idx, m_out.data(), &bad);
        if (first_bad) *first_bad = bad;
        if (rc) throw Error(rc, pkl_last_error(p_));
    }
    // steps 2 and 3: the helper tables to commit
    LookupHelpers begin(const DeviceVec& t, const uint32_t* d_idx, const std::vector<FieldElement>& bind = {}) const {
        if (bind.size() != st_.n_bind) throw Error(PK_ERR_BAD_ARG, "bind must have the statement's count");
        LookupHelpers h{};
        if (int rc = pkl_begin(p_, t.data(), d_idx, bind.empty() ? nullptr : bind[0].data(), h.alpha.data(), &h.h_f, &h.h_t)) throw Error(rc, pkl_last_error(p_));
        return h;
    }
    // steps 4 and 5
    LookupProof finish(const std::vector<FieldElement>& bind2 = {}) const {
        if (bind2.size() != st_.n_bind2) throw Error(PK_ERR_BAD_ARG, "bind2 must have the statement's count");
        size_t len = 0;
        pkl_proof_bytes(&st_, &len);
        LookupProof out;
        out.proof.resize(len);
        pkl_claims c;
        if (int rc = pkl_finish(p_, bind2.empty() ? nullptr : bind2[0].data(), out.proof.data(), out.proof.size(), &len, &c)) throw Error(rc, pkl_last_error(p_));
        out.claims = LookupClaims::from(st_, c);
        return out;
    }

    // host only
    static LookupVerdict verify(const pkl_statement& st, const std::vector<uint8_t>& proof, const std::vector<FieldElement>& bind = {},
                                const std::vector<FieldElement>& bind2 = {}) {
        if (bind.size() != st.n_bind || bind2.size() != st.n_bind2) throw Error(PK_ERR_BAD_ARG, "bind and bind2 must have the statement's counts");
        pkl_claims c;
        pkv_result r;
        int side = 0;
        const int rc = pkl_verify(&st, nullptr, 0, bind.empty() ? nullptr : bind[0].data(), bind2.empty() ? nullptr : bind2[0].data(), proof.data(), proof.size(), &c,
                                  &side, &r);
        if (rc) throw Error(rc, pkl_create_error());
        LookupVerdict v{r.accepted != 0, r.check, side, r.offset, r.message, {}};
        if (v.accepted) v.claims = LookupClaims::from(st, c);
        return v;
    }

   private:
    pkl_statement st_;
    pkl_prover* p_ = nullptr;
};

}  // namespace provekit
