// provekit_sumcheck.hpp -- provekit::ProductSumcheck: the C++ face of libprovekit_sumcheck.so (include/provekit_sumcheck.h), next to
// provekit_whir.hpp's WhirPcs.  Prove that sum_x eq(tau, x) sum_t c_t prod_{j in S_t} f_j(x) = s over device tables; verify on the host.
// An accepted proof is accepted PROVIDED f_j(point) = finals[j]: WhirPcs::open / WhirPcs::verify at `point` establish that for
// committed tables.  A rejected proof is a verdict, not an exception; only a failed call throws provekit::Error.
#pragma once
#include "provekit_hip.hpp"
#include "provekit_sumcheck.h"

namespace provekit {

struct SumcheckVerdict {
    bool accepted;
    int check;        // PKV_CHECK_* or PKS_CHECK_*
    uint64_t offset;  // bytes of the proof consumed
    std::string message;
    std::vector<FieldElement> point;   // n challenges, variable 0 first (when accepted)
    std::vector<FieldElement> finals;  // the m values the proof claims for f_j(point) (when accepted)
    const char* check_name() const { return pks_check_name(check); }
    explicit operator bool() const { return accepted; }
};

struct SumcheckProof {
    std::vector<uint8_t> proof;  // s first, canonical
    std::vector<FieldElement> point, finals;
};

// the statement: add_term(coefficient, {tables}) once per term
struct SumcheckStatement {
    pks_statement c{};
    SumcheckStatement(unsigned n, unsigned m, bool has_tau, unsigned n_bind = 0) {
        c.n = n, c.m = m, c.has_tau = has_tau ? 1 : 0, c.n_bind = n_bind;
    }
    SumcheckStatement& add_term(const FieldElement& coefficient, std::initializer_list<unsigned> tables) {
        if (c.T >= PKS_MAX_TERMS) throw Error(PK_ERR_BAD_ARG, "at most 4 terms");
        for (unsigned j : tables) c.masks[c.T] |= 1u << j;
        std::memcpy(c.coeffs[c.T], coefficient.data(), 32);
        c.T++;
        return *this;
    }
    std::string io_pattern() const {
        size_t n = 0;
        if (int rc = pks_io_pattern(&c, nullptr, 0, &n)) throw Error(rc, pks_create_error());
        std::string s(n, '\0');
        pks_io_pattern(&c, reinterpret_cast<uint8_t*>(&s[0]), n, &n);
        return s;
    }
    size_t proof_bytes() const {
        size_t n = 0;
        if (int rc = pks_proof_bytes(&c, &n)) throw Error(rc, pks_create_error());
        return n;
    }
};

class ProductSumcheck {
   public:
    ProductSumcheck(const Context& ctx, const SumcheckStatement& st) : st_(st.c) {
        if (int rc = pks_prover_create(ctx.get(), &st_, &p_)) throw Error(rc, pks_create_error());
    }
    ~ProductSumcheck() { pks_prover_destroy(p_); }
    ProductSumcheck(const ProductSumcheck&) = delete;
    ProductSumcheck& operator=(const ProductSumcheck&) = delete;

    // tables: m device vectors of 2^n elements (read only); tau: n elements if the statement has one; bind: n_bind elements
    SumcheckProof prove(const std::vector<const DeviceVec*>& tables, const std::vector<FieldElement>& tau = {},
                        const std::vector<FieldElement>& bind = {}) const {
        if (tables.size() != st_.m || tau.size() != (st_.has_tau ? st_.n : 0) || bind.size() != st_.n_bind)
            throw Error(PK_ERR_BAD_ARG, "tables, tau and bind must have the statement's counts");
        std::vector<const uint64_t*> p;
        for (const DeviceVec* v : tables) {
            if (v->size() != (size_t)1 << st_.n) throw Error(PK_ERR_BAD_ARG, "a table has 2^n elements");
            p.push_back(v->data());
        }
        SumcheckProof out;
        size_t len = 0;
        pks_proof_bytes(&st_, &len);
        out.proof.resize(len);
        out.point.resize(st_.n);
        out.finals.resize(st_.m);
        const int rc = pks_prove(p_, p.data(), tau.empty() ? nullptr : tau[0].data(), bind.empty() ? nullptr : bind[0].data(), out.proof.data(),
                                 out.proof.size(), &len, out.point[0].data(), out.finals[0].data());
        if (rc) throw Error(rc, pks_last_error(p_));
        return out;
    }

    // host only.  expected_sum null: the verdict holds for the s the proof states (its first 32 bytes)
    static SumcheckVerdict verify(const SumcheckStatement& st, const std::vector<uint8_t>& proof, const std::vector<FieldElement>& tau = {},
                                  const std::vector<FieldElement>& bind = {}, const FieldElement* expected_sum = nullptr) {
        if (tau.size() != (st.c.has_tau ? st.c.n : 0) || bind.size() != st.c.n_bind) throw Error(PK_ERR_BAD_ARG, "tau and bind must have the statement's counts");
        SumcheckVerdict v{};
        v.point.resize(st.c.n <= PKS_MAX_VARS ? st.c.n : 0);
        v.finals.resize(st.c.m <= PKS_MAX_TABLES ? st.c.m : 0);
        pkv_result r;
        const int rc = pks_verify(&st.c, nullptr, 0, tau.empty() ? nullptr : tau[0].data(), bind.empty() ? nullptr : bind[0].data(),
                                  expected_sum ? expected_sum->data() : nullptr, proof.data(), proof.size(), v.point.empty() ? nullptr : v.point[0].data(),
                                  v.finals.empty() ? nullptr : v.finals[0].data(), &r);
        if (rc) throw Error(rc, pks_create_error());
        v.accepted = r.accepted != 0, v.check = r.check, v.offset = r.offset, v.message = r.message;
        return v;
    }

   private:
    pks_statement st_;
    pks_prover* p_ = nullptr;
};

}  // namespace provekit
