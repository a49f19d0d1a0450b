// provekit_grandproduct.hpp -- provekit::GrandProduct and provekit::MultisetEquality: the C++ face of libprovekit_grandproduct.so
// (include/provekit_grandproduct.h), next to provekit_lookup.hpp's Lookup.  Prove that a device table multiplies to P, or that two
// sides of w device columns hold the same rows as multisets; verify on the host.  An accepted grand product is accepted PROVIDED
// v(point) = value, an accepted multiset proof PROVIDED the two combinations of MultisetClaims: WhirPcs::open / WhirPcs::verify
// establish them for committed tables.  A rejected proof is a verdict, not an exception; only a failed call throws provekit::Error.
#pragma once
#include "provekit_grandproduct.h"
#include "provekit_hip.hpp"

namespace provekit {

struct GrandProductProof {
    std::vector<uint8_t> proof;
    FieldElement product;
    std::vector<FieldElement> point;  // z_n, variable 0 first
    FieldElement value;               // c_n
};

struct GrandProductVerdict {
    bool accepted;
    int check;        // PKV_CHECK_*, PKS_CHECK_* or PKG_CHECK_PRODUCT
    unsigned layer;   // the layer the verdict is about, 0: the outer framing and transcript
    uint64_t offset;  // bytes of the proof consumed
    std::string message;
    FieldElement product, value;      // when accepted
    std::vector<FieldElement> point;  // when accepted
    const char* check_name() const { return pkg_check_name(check); }
    explicit operator bool() const { return accepted; }
};

class GrandProduct {
   public:
    GrandProduct(const Context& ctx, unsigned n, unsigned n_bind = 0) : st_{n, n_bind} {
        if (int rc = pkg_prover_create(ctx.get(), &st_, &p_)) throw Error(rc, pkg_create_error());
    }
    ~GrandProduct() { pkg_prover_destroy(p_); }
    GrandProduct(const GrandProduct&) = delete;
    GrandProduct& operator=(const GrandProduct&) = delete;
    const pkg_statement& statement() const { return st_; }

    GrandProductProof prove(const DeviceVec& v, const std::vector<FieldElement>& bind = {}) const {
        if (v.size() != (size_t)1 << st_.n || bind.size() != st_.n_bind) throw Error(PK_ERR_BAD_ARG, "v has 2^n elements, bind the statement's count");
        size_t len = 0;
        pkg_proof_bytes(&st_, &len);
        GrandProductProof out;
        out.proof.resize(len);
        out.point.resize(st_.n);
        if (int rc = pkg_prove(p_, v.data(), bind.empty() ? nullptr : bind[0].data(), out.proof.data(), out.proof.size(), &len, out.product.data(),
                               out.point[0].data(), out.value.data()))
            throw Error(rc, pkg_last_error(p_));
        return out;
    }

    // host only
    static GrandProductVerdict verify(const pkg_statement& st, const std::vector<uint8_t>& proof, const std::vector<FieldElement>& bind = {},
                                      const FieldElement* expected_product = nullptr) {
        if (bind.size() != st.n_bind) throw Error(PK_ERR_BAD_ARG, "bind must have the statement's count");
        pkv_result r;
        GrandProductVerdict v{};
        std::vector<FieldElement> point(PKG_MAX_VARS);
        const int rc = pkg_verify(&st, nullptr, 0, bind.empty() ? nullptr : bind[0].data(), expected_product ? expected_product->data() : nullptr, proof.data(),
                                  proof.size(), v.product.data(), point[0].data(), v.value.data(), &v.layer, &r);
        if (rc) throw Error(rc, pkg_create_error());
        v.accepted = r.accepted != 0, v.check = r.check, v.offset = r.offset, v.message = r.message;
        if (v.accepted) v.point.assign(point.begin(), point.begin() + st.n);
        return v;
    }

   private:
    pkg_statement st_;
    pkg_prover* p_ = nullptr;
};

struct MultisetClaims {
    FieldElement gamma, beta;
    std::vector<FieldElement> z_a, z_b;  // the points, variable 0 first
    FieldElement comb_a, comb_b;         // what sum_j beta^j column_j must take at them
    static MultisetClaims from(const pkg_multiset_statement& st, const pkg_multiset_claims& c) {
        auto fe = [](const uint64_t* p) { return FieldElement{p[0], p[1], p[2], p[3]}; };
        MultisetClaims o;
        o.gamma = fe(c.gamma), o.beta = fe(c.beta), o.comb_a = fe(c.comb_a), o.comb_b = fe(c.comb_b);
        for (unsigned i = 0; i < st.n; i++) o.z_a.push_back(fe(c.z_a[i])), o.z_b.push_back(fe(c.z_b[i]));
        return o;
    }
};

struct MultisetProof {
    std::vector<uint8_t> proof;
    MultisetClaims claims;
};

struct MultisetVerdict {
    bool accepted;
    int check;
    int side;  // PKG_SIDE_*
    unsigned layer;
    uint64_t offset;
    std::string message;
    MultisetClaims claims;  // when accepted
    const char* check_name() const { return pkg_check_name(check); }
    explicit operator bool() const { return accepted; }
};

class MultisetEquality {
   public:
    MultisetEquality(const Context& ctx, unsigned n, unsigned w = 1, unsigned n_bind = 0) : st_{n, w, n_bind} {
        if (int rc = pkg_multiset_prover_create(ctx.get(), &st_, &p_)) throw Error(rc, pkg_create_error());
    }
    ~MultisetEquality() { pkg_multiset_prover_destroy(p_); }
    MultisetEquality(const MultisetEquality&) = delete;
    MultisetEquality& operator=(const MultisetEquality&) = delete;
    const pkg_multiset_statement& statement() const { return st_; }

    // sides that are not equal as multisets throw with code PK_ERR_UNSATISFIED; the prover stays usable
    MultisetProof prove(const std::vector<const DeviceVec*>& a, const std::vector<const DeviceVec*>& b, const std::vector<FieldElement>& bind = {}) const {
        if (a.size() != st_.w || b.size() != st_.w || bind.size() != st_.n_bind) throw Error(PK_ERR_BAD_ARG, "w columns per side, bind the statement's count");
        std::vector<const uint64_t*> pa, pb;
        for (unsigned j = 0; j < st_.w; j++) {
            if (a[j]->size() != (size_t)1 << st_.n || b[j]->size() != a[j]->size()) throw Error(PK_ERR_BAD_ARG, "every column has 2^n elements");
            pa.push_back(a[j]->data()), pb.push_back(b[j]->data());
        }
        size_t len = 0;
        pkg_multiset_proof_bytes(&st_, &len);
        MultisetProof out;
        out.proof.resize(len);
        pkg_multiset_claims c;
        if (int rc = pkg_multiset_prove(p_, pa.data(), pb.data(), bind.empty() ? nullptr : bind[0].data(), out.proof.data(), out.proof.size(), &len, &c))
            throw Error(rc, pkg_multiset_last_error(p_));
        out.claims = MultisetClaims::from(st_, c);
        return out;
    }

    // host only
    static MultisetVerdict verify(const pkg_multiset_statement& st, const std::vector<uint8_t>& proof, const std::vector<FieldElement>& bind = {}) {
        if (bind.size() != st.n_bind) throw Error(PK_ERR_BAD_ARG, "bind must have the statement's count");
        pkg_multiset_claims c;
        pkv_result r;
        int side = 0;
        unsigned layer = 0;
        const int rc = pkg_multiset_verify(&st, nullptr, 0, bind.empty() ? nullptr : bind[0].data(), proof.data(), proof.size(), &c, &side, &layer, &r);
        if (rc) throw Error(rc, pkg_create_error());
        MultisetVerdict v{r.accepted != 0, r.check, side, layer, r.offset, r.message, {}};
        if (v.accepted) v.claims = MultisetClaims::from(st, c);
        return v;
    }

   private:
    pkg_multiset_statement st_;
    pkg_multiset_prover* p_ = nullptr;
};

}  // namespace provekit
