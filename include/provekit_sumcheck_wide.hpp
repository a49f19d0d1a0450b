// provekit_sumcheck_wide.hpp -- provekit::WideSumcheck: the C++ face of the wide product sumcheck (include/provekit_sumcheck_wide.h),
// next to provekit_sumcheck.hpp's ProductSumcheck, whose proof and verdict types it shares.  Up to 16 tables, 16 terms, and powers of a
// table up to degree 5: add_term(coefficient, {0, 0, 1}) is c f_0^2 f_1.  An accepted proof is accepted PROVIDED f_j(point) = finals[j].
// A rejected proof is a verdict, not an exception; only a failed call throws provekit::Error.
#pragma once
#include "provekit_sumcheck.hpp"
#include "provekit_sumcheck_wide.h"

namespace provekit {

// the statement: add_term(coefficient, {tables, non-decreasing; a repeated table is a power}) once per term
struct WideSumcheckStatement {
    pksw_statement c{};
    WideSumcheckStatement(unsigned n, unsigned m, bool has_tau, unsigned n_bind = 0) { c.n = n, c.m = m, c.has_tau = has_tau ? 1 : 0, c.n_bind = n_bind; }
    WideSumcheckStatement& add_term(const FieldElement& coefficient, std::initializer_list<unsigned> tables) {
        if (c.T >= PKSW_MAX_TERMS) throw Error(PK_ERR_BAD_ARG, "at most 16 terms");
        if (tables.size() > PKSW_MAX_DEGREE) throw Error(PK_ERR_BAD_ARG, "at most 5 factors in a term");
        for (unsigned j : tables) c.factors[c.T][c.lens[c.T]++] = j;
        std::memcpy(c.coeffs[c.T], coefficient.data(), 32);
        c.T++;
        return *this;
    }
    std::string io_pattern() const {
        size_t n = 0;
        if (int rc = pksw_io_pattern(&c, nullptr, 0, &n)) throw Error(rc, pksw_create_error());
        std::string s(n, '\0');
        pksw_io_pattern(&c, reinterpret_cast<uint8_t*>(&s[0]), n, &n);
        return s;
    }
    size_t proof_bytes() const { return size(pksw_proof_bytes); }
    size_t arena_bytes() const { return size(pksw_arena_bytes); }

   private:
    size_t size(int (*fn)(const pksw_statement*, size_t*)) const {
        size_t n = 0;
        if (int rc = fn(&c, &n)) throw Error(rc, pksw_create_error());
        return n;
    }
};

class WideSumcheck {
   public:
    WideSumcheck(const Context& ctx, const WideSumcheckStatement& st) : st_(st.c) {
        if (int rc = pksw_prover_create(ctx.get(), &st_, &p_)) throw Error(rc, pksw_create_error());
    }
    ~WideSumcheck() { pksw_prover_destroy(p_); }
    WideSumcheck(const WideSumcheck&) = delete;
    WideSumcheck& operator=(const WideSumcheck&) = delete;

    // tables: m device vectors of 2^n elements (read only); tau: n elements if the statement has one; bind: n_bind elements
    SumcheckProof prove(const std::vector<const DeviceVec*>& tables, const std::vector<FieldElement>& tau = {}, const std::vector<FieldElement>& bind = {}) const {
        if (tables.size() != st_.m || tau.size() != (st_.has_tau ? st_.n : 0) || bind.size() != st_.n_bind)
            throw Error(PK_ERR_BAD_ARG, "tables, tau and bind must have the statement's counts");
        std::vector<const uint64_t*> p;
        for (const DeviceVec* v : tables) {
            if (v->size() != (size_t)1 << st_.n) throw Error(PK_ERR_BAD_ARG, "a table has 2^n elements");
            p.push_back(v->data());
        }
        SumcheckProof out;
        size_t len = 0;
        pksw_proof_bytes(&st_, &len);
        out.proof.resize(len);
        out.point.resize(st_.n);
        out.finals.resize(st_.m);
        const int rc = pksw_prove(p_, p.data(), tau.empty() ? nullptr : tau[0].data(), bind.empty() ? nullptr : bind[0].data(), out.proof.data(),
                                  out.proof.size(), &len, out.point[0].data(), out.finals[0].data());
        if (rc) throw Error(rc, pksw_last_error(p_));
        return out;
    }

    // host only.  expected_sum null: the verdict holds for the s the proof states (its first 32 bytes)
    static SumcheckVerdict verify(const WideSumcheckStatement& st, const std::vector<uint8_t>& proof, const std::vector<FieldElement>& tau = {},
                                  const std::vector<FieldElement>& bind = {}, const FieldElement* expected_sum = nullptr) {
        if (tau.size() != (st.c.has_tau ? st.c.n : 0) || bind.size() != st.c.n_bind) throw Error(PK_ERR_BAD_ARG, "tau and bind must have the statement's counts");
        SumcheckVerdict v{};
        v.point.resize(st.c.n <= PKS_MAX_VARS ? st.c.n : 0);
        v.finals.resize(st.c.m <= PKSW_MAX_TABLES ? st.c.m : 0);
        pkv_result r;
        const int rc = pksw_verify(&st.c, nullptr, 0, tau.empty() ? nullptr : tau[0].data(), bind.empty() ? nullptr : bind[0].data(),
                                   expected_sum ? expected_sum->data() : nullptr, proof.data(), proof.size(), v.point.empty() ? nullptr : v.point[0].data(),
                                   v.finals.empty() ? nullptr : v.finals[0].data(), &r);
        if (rc) throw Error(rc, pksw_create_error());
        v.accepted = r.accepted != 0, v.check = r.check, v.offset = r.offset, v.message = r.message;
        return v;
    }

   private:
    pksw_statement st_;
    pksw_prover* p_ = nullptr;
};

}  // namespace provekit
