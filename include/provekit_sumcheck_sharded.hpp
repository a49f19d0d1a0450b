// provekit_sumcheck_sharded.hpp -- provekit::ShardedProductSumcheck: ProductSumcheck (provekit_sumcheck.hpp) on one context of a
// device set (include/provekit_sumcheck_sharded.h).  Construction and prove() are collective: every rank of the set makes the same
// calls with the same statement, tau and bind, one host thread per rank, and every rank gets the lone prover's proof, byte for byte;
// ProductSumcheck::verify verifies it.  Ranks that disagree all throw; ranks handed different TABLES are not detected.
#pragma once
#include "provekit_sumcheck.hpp"
#include "provekit_sumcheck_sharded.h"

namespace provekit {

// what a sharded proof of `st` takes on each of `world` ranks (host only)
inline struct pkss_plan sharded_sumcheck_plan(const SumcheckStatement& st, unsigned world) {
    struct pkss_plan plan;
    if (int rc = pkss_plan(&st.c, world, &plan)) throw Error(rc, pks_create_error());
    return plan;
}

class ShardedProductSumcheck {
   public:
    ShardedProductSumcheck(const Context& ctx, const SumcheckStatement& st) : st_(st.c) {
        if (int rc = pkss_prover_create(ctx.get(), &st_, &p_)) throw Error(rc, pks_create_error());
    }
    ~ShardedProductSumcheck() { pks_prover_destroy(p_); }
    ShardedProductSumcheck(const ShardedProductSumcheck&) = delete;
    ShardedProductSumcheck& operator=(const ShardedProductSumcheck&) = delete;

    // tables: m device vectors of 2^n elements on this rank's context, the same contents on every rank (read only)
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
        const int rc = pkss_prove(p_, p.data(), tau.empty() ? nullptr : tau[0].data(), bind.empty() ? nullptr : bind[0].data(), out.proof.data(),
                                  out.proof.size(), &len, out.point[0].data(), out.finals[0].data());
        if (rc) throw Error(rc, pks_last_error(p_));
        return out;
    }

   private:
    pks_statement st_;
    pks_prover* p_ = nullptr;
};

}  // namespace provekit
