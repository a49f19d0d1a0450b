// provekit_fracsum.hpp -- provekit::FractionalSum and provekit::GkrLookup: the C++ face of libprovekit_fracsum.so
// (include/provekit_fracsum.h), next to provekit_grandproduct.hpp's GrandProduct.  Prove that sum_x p[x] / q[x] = P / Q over device
// tables, or that every entry of a device column is an entry of a table with given multiplicities -- with no helper column and no
// second commitment phase; verify on the host.  An accepted fractional sum is accepted PROVIDED q(point) = value_q (and p(point) =
// value_p), an accepted lookup PROVIDED the three values of GkrLookupClaims: WhirPcs::open / WhirPcs::verify establish them for
// committed tables.  A rejected proof is a verdict, not an exception; only a failed call throws provekit::Error.
#pragma once
#include "provekit_fracsum.h"
#include "provekit_hip.hpp"

namespace provekit {

struct FractionalSumProof {
    std::vector<uint8_t> proof;
    FieldElement P, Q;
    std::vector<FieldElement> point;  // z_n, variable 0 first
    FieldElement value_p, value_q;    // cp_n (not set for a unit statement), cq_n
};

struct FractionalSumVerdict {
    bool accepted;
    int check;        // PKV_CHECK_*, PKS_CHECK_* or PKF_CHECK_*
    unsigned layer;   // the layer the verdict is about, 0: the outer framing, the top and the transcript
    uint64_t offset;  // bytes of the proof consumed
    std::string message;
    FieldElement P, Q, value_p, value_q;  // when accepted
    std::vector<FieldElement> point;      // when accepted
    const char* check_name() const { return pkf_check_name(check); }
    explicit operator bool() const { return accepted; }
};

class FractionalSum {
   public:
    FractionalSum(const Context& ctx, unsigned n, unsigned n_bind = 0, bool unit = false) : st_{n, n_bind, unit ? 1u : 0u} {
        if (int rc = pkf_prover_create(ctx.get(), &st_, &p_)) throw Error(rc, pkf_create_error());
    }
    ~FractionalSum() { pkf_prover_destroy(p_); }
    FractionalSum(const FractionalSum&) = delete;
    FractionalSum& operator=(const FractionalSum&) = delete;
    const pkf_statement& statement() const { return st_; }

    // p: nullptr exactly for a unit statement.  A zero denominator throws with code PK_ERR_UNSATISFIED; the prover stays usable
    FractionalSumProof prove(const DeviceVec* p, const DeviceVec& q, const std::vector<FieldElement>& bind = {}) const {
        if (q.size() != (size_t)1 << st_.n || (p && p->size() != q.size()) || bind.size() != st_.n_bind)
            throw Error(PK_ERR_BAD_ARG, "p and q have 2^n elements, bind the statement's count");
        size_t len = 0;
        pkf_proof_bytes(&st_, &len);
        FractionalSumProof out;
        out.proof.resize(len);
        out.point.resize(st_.n);
        uint64_t fraction[8];
        if (int rc = pkf_prove(p_, p ? p->data() : nullptr, q.data(), bind.empty() ? nullptr : bind[0].data(), out.proof.data(), out.proof.size(), &len, fraction,
                               out.point[0].data(), out.value_p.data(), out.value_q.data()))
            throw Error(rc, pkf_last_error(p_));
        out.P = {fraction[0], fraction[1], fraction[2], fraction[3]}, out.Q = {fraction[4], fraction[5], fraction[6], fraction[7]};
        return out;
    }

    // host only; expected: {num, den} or nullptr
    static FractionalSumVerdict verify(const pkf_statement& st, const std::vector<uint8_t>& proof, const std::vector<FieldElement>& bind = {},
                                       const std::array<FieldElement, 2>* expected = nullptr) {
        if (bind.size() != st.n_bind) throw Error(PK_ERR_BAD_ARG, "bind must have the statement's count");
        pkv_result r;
        FractionalSumVerdict v{};
        std::vector<FieldElement> point(PKF_MAX_VARS);
        uint64_t fraction[8] = {}, want[8];
        if (expected) std::memcpy(want, (*expected)[0].data(), 32), std::memcpy(want + 4, (*expected)[1].data(), 32);
        const int rc = pkf_verify(&st, nullptr, 0, bind.empty() ? nullptr : bind[0].data(), expected ? want : nullptr, proof.data(), proof.size(), fraction,
                                  point[0].data(), v.value_p.data(), v.value_q.data(), &v.layer, &r);
        if (rc) throw Error(rc, pkf_create_error());
        v.accepted = r.accepted != 0, v.check = r.check, v.offset = r.offset, v.message = r.message;
        if (v.accepted) {
            v.point.assign(point.begin(), point.begin() + st.n);
            v.P = {fraction[0], fraction[1], fraction[2], fraction[3]}, v.Q = {fraction[4], fraction[5], fraction[6], fraction[7]};
        }
        return v;
    }

   private:
    pkf_statement st_;
    pkf_prover* p_ = nullptr;
};

struct GkrLookupClaims {
    FieldElement alpha;
    std::vector<FieldElement> z_f, z_t;         // the points, variable 0 first
    FieldElement f_value, t_value, m_value;     // what f(z_f), t(z_t) and m(z_t) must be
    static GkrLookupClaims from(const pkf_lookup_statement& st, const pkf_lookup_claims& c) {
        auto fe = [](const uint64_t* p) { return FieldElement{p[0], p[1], p[2], p[3]}; };
        GkrLookupClaims o;
        o.alpha = fe(c.alpha), o.f_value = fe(c.f_value), o.t_value = fe(c.t_value), o.m_value = fe(c.m_value);
        for (unsigned i = 0; i < st.n; i++) o.z_f.push_back(fe(c.z_f[i]));
        for (unsigned i = 0; i < st.k; i++) o.z_t.push_back(fe(c.z_t[i]));
        return o;
    }
};

struct GkrLookupProof {
    std::vector<uint8_t> proof;
    GkrLookupClaims claims;
};

struct GkrLookupVerdict {
    bool accepted;
    int check;
    int side;  // PKF_SIDE_*
    unsigned layer;
    uint64_t offset;
    std::string message;
    GkrLookupClaims claims;  // when accepted
    const char* check_name() const { return pkf_check_name(check); }
    explicit operator bool() const { return accepted; }
};

class GkrLookup {
   public:
    GkrLookup(const Context& ctx, unsigned n, unsigned k, unsigned n_bind = 0) : st_{n, k, n_bind} {
        if (int rc = pkf_lookup_prover_create(ctx.get(), &st_, &p_)) throw Error(rc, pkf_create_error());
    }
    ~GkrLookup() { pkf_lookup_prover_destroy(p_); }
    GkrLookup(const GkrLookup&) = delete;
    GkrLookup& operator=(const GkrLookup&) = delete;
    const pkf_lookup_statement& statement() const { return st_; }

    // a column that is not inside the table under m, or an alpha that is an entry, throws with code PK_ERR_UNSATISFIED; the prover
    // stays usable
    GkrLookupProof prove(const DeviceVec& f, const DeviceVec& t, const DeviceVec& m, const std::vector<FieldElement>& bind = {}) const {
        if (f.size() != (size_t)1 << st_.n || t.size() != (size_t)1 << st_.k || m.size() != t.size() || bind.size() != st_.n_bind)
            throw Error(PK_ERR_BAD_ARG, "f has 2^n elements, t and m 2^k, bind the statement's count");
        size_t len = 0;
        pkf_lookup_proof_bytes(&st_, &len);
        GkrLookupProof out;
        out.proof.resize(len);
        pkf_lookup_claims c;
        if (int rc = pkf_lookup_prove(p_, f.data(), t.data(), m.data(), bind.empty() ? nullptr : bind[0].data(), out.proof.data(), out.proof.size(), &len, &c))
            throw Error(rc, pkf_lookup_last_error(p_));
        out.claims = GkrLookupClaims::from(st_, c);
        return out;
    }

    // host only
    static GkrLookupVerdict verify(const pkf_lookup_statement& st, const std::vector<uint8_t>& proof, const std::vector<FieldElement>& bind = {}) {
        if (bind.size() != st.n_bind) throw Error(PK_ERR_BAD_ARG, "bind must have the statement's count");
        pkf_lookup_claims c;
        pkv_result r;
        int side = 0;
        unsigned layer = 0;
        const int rc = pkf_lookup_verify(&st, nullptr, 0, bind.empty() ? nullptr : bind[0].data(), proof.data(), proof.size(), &c, &side, &layer, &r);
        if (rc) throw Error(rc, pkf_create_error());
        GkrLookupVerdict v{r.accepted != 0, r.check, side, layer, r.offset, r.message, {}};
        if (v.accepted) v.claims = GkrLookupClaims::from(st, c);
        return v;
    }

   private:
    pkf_lookup_statement st_;
    pkf_lookup_prover* p_ = nullptr;
};

}  // namespace provekit
