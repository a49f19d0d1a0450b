// provekit_memcheck.hpp -- provekit::MemCheck: the C++ face of libprovekit_memcheck.so (include/provekit_memcheck.h), next to
// provekit_tuplelookup.hpp's TupleLookup.  Build the columns of a read-write memory's trace on the device, prove that the trace is
// consistent -- every read returns what the last write to its address left there -- and verify on the host.  An accepted proof is
// accepted PROVIDED the four values of MemCheckClaims: WhirPcs::open / WhirPcs::verify give the columns' evaluations,
// MemCheck::check_claims forms the combinations.  A rejected proof is a verdict, not an exception; only a failed call throws
// provekit::Error.
#pragma once
#include "provekit_hip.hpp"
#include "provekit_memcheck.h"

namespace provekit {

struct MemCheckClaims {
    pkm_claims raw;  // what check_claims reads
    FieldElement gamma, beta;
    std::vector<FieldElement> z_ops, z_mem, z_f, z_t;  // the points, variable 0 first: a, wv, rv, rt at z_ops; init, fin, ft at z_mem; rt at z_f; m at z_t
    FieldElement ops_value, mem_value, rt_value, m_value;  // what the four combinations must be
    static MemCheckClaims from(const pkm_statement& st, const pkm_claims& c) {
        auto fe = [](const uint64_t* p) { return FieldElement{p[0], p[1], p[2], p[3]}; };
        MemCheckClaims o;
        o.raw = c;
        o.gamma = fe(c.gamma), o.beta = fe(c.beta);
        o.ops_value = fe(c.ops_value), o.mem_value = fe(c.mem_value), o.rt_value = fe(c.rt_value), o.m_value = fe(c.m_value);
        for (unsigned i = 0; i < st.n; i++) o.z_ops.push_back(fe(c.z_ops[i])), o.z_f.push_back(fe(c.z_f[i])), o.z_t.push_back(fe(c.z_t[i]));
        for (unsigned i = 0; i < st.k; i++) o.z_mem.push_back(fe(c.z_mem[i]));
        return o;
    }
};

struct MemCheckProof {
    std::vector<uint8_t> proof;
    MemCheckClaims claims;
};

struct MemCheckVerdict {
    bool accepted;
    int check;  // PKV_CHECK_*, PKS_CHECK_*, PKF_CHECK_* or PKM_CHECK_*
    int side;   // PKM_SIDE_*
    unsigned layer;
    uint64_t offset;
    std::string message;
    MemCheckClaims claims;  // when accepted
    const char* check_name() const { return pkm_check_name(check); }
    explicit operator bool() const { return accepted; }
};

// the eight device columns of a trace
struct MemCheckColumns {
    const DeviceVec *a, *wv, *rv, *rt, *init, *fin, *ft, *m;
};

class MemCheck {
   public:
    MemCheck(const Context& ctx, unsigned n, unsigned k, unsigned n_bind = 0) : st_{n, k, n_bind} {
        if (int rc = pkm_prover_create(ctx.get(), &st_, &p_)) throw Error(rc, pkm_create_error());
    }
    ~MemCheck() { pkm_prover_destroy(p_); }
    MemCheck(const MemCheck&) = delete;
    MemCheck& operator=(const MemCheck&) = delete;
    const pkm_statement& statement() const { return st_; }

    // 2^n addresses as a device column for `trace`
    static DeviceVec addresses(const Context& ctx, const std::vector<uint32_t>& addr) {
        DeviceVec d(ctx, (addr.size() * 4 + 31) / 32);
        if (!addr.empty()) ctx.check(pk_memcpy_h2d(ctx.get(), d.data(), addr.data(), 4 * addr.size()));
        return d;
    }

    // from the addresses (`addresses`), the values the operations leave and the initial contents: a, rv, rt, m (2^n elements) and fin,
    // ft (2^k).  An address >= 2^k throws with code PK_ERR_BAD_ARG; *first_bad: the smallest such operation
    void trace(const DeviceVec& addr, const DeviceVec& wv, const DeviceVec& init, DeviceVec& a, DeviceVec& rv, DeviceVec& rt, DeviceVec& fin, DeviceVec& ft, DeviceVec& m,
               uint64_t* first_bad = nullptr) const {
        const size_t N = (size_t)1 << st_.n, K = (size_t)1 << st_.k;
        if (addr.size() * 32 < 4 * N || wv.size() != N || a.size() != N || rv.size() != N || rt.size() != N || m.size() != N || init.size() != K || fin.size() != K ||
            ft.size() != K)
            throw Error(PK_ERR_BAD_ARG, "the operation columns have 2^n elements, the memory columns 2^k");
        if (int rc = pkm_trace(p_, reinterpret_cast<const uint32_t*>(addr.data()), wv.data(), init.data(), a.data(), rv.data(), rt.data(), fin.data(), ft.data(), m.data(),
                               first_bad))
            throw Error(rc, pkm_last_error(p_));
    }

    // an inconsistent trace throws with code PK_ERR_UNSATISFIED and a reason that names the case; the prover stays usable
    MemCheckProof prove(const MemCheckColumns& cols, const std::vector<FieldElement>& bind = {}) const {
        if (bind.size() != st_.n_bind) throw Error(PK_ERR_BAD_ARG, "bind has the statement's count");
        const size_t N = (size_t)1 << st_.n, K = (size_t)1 << st_.k;
        for (const DeviceVec* v : {cols.a, cols.wv, cols.rv, cols.rt, cols.m})
            if (!v || v->size() != N) throw Error(PK_ERR_BAD_ARG, "an operation column has 2^n elements");
        for (const DeviceVec* v : {cols.init, cols.fin, cols.ft})
            if (!v || v->size() != K) throw Error(PK_ERR_BAD_ARG, "a memory column has 2^k elements");
        const pkm_columns raw{cols.a->data(), cols.wv->data(), cols.rv->data(), cols.rt->data(), cols.init->data(), cols.fin->data(), cols.ft->data(), cols.m->data()};
        size_t len = 0;
        pkm_proof_bytes(&st_, &len);
        MemCheckProof out;
        out.proof.resize(len);
        pkm_claims c;
        if (int rc = pkm_prove(p_, &raw, bind.empty() ? nullptr : bind[0].data(), out.proof.data(), out.proof.size(), &len, &c)) throw Error(rc, pkm_last_error(p_));
        out.claims = MemCheckClaims::from(st_, c);
        return out;
    }

    // host only
    static MemCheckVerdict verify(const pkm_statement& st, const std::vector<uint8_t>& proof, const std::vector<FieldElement>& bind = {}) {
        if (bind.size() != st.n_bind) throw Error(PK_ERR_BAD_ARG, "bind must have the statement's count");
        pkm_claims c;
        pkv_result r;
        int side = 0;
        unsigned layer = 0;
        const int rc = pkm_verify(&st, nullptr, 0, bind.empty() ? nullptr : bind[0].data(), proof.data(), proof.size(), &c, &side, &layer, &r);
        if (rc) throw Error(rc, pkm_create_error());
        MemCheckVerdict v{r.accepted != 0, r.check, side, layer, r.offset, r.message, {}};
        if (v.accepted) v.claims = MemCheckClaims::from(st, c);
        return v;
    }

    // host only: ops_evals = (a, wv, rv, rt)(z_ops), mem_evals = (init, fin, ft)(z_mem), rt_eval = rt(z_f), m_eval = m(z_t) -> PKM_CLAIM_NONE
    // when the four claims hold, else the first that does not
    static int check_claims(const pkm_statement& st, const MemCheckClaims& claims, const std::vector<FieldElement>& ops_evals, const std::vector<FieldElement>& mem_evals,
                            const FieldElement& rt_eval, const FieldElement& m_eval) {
        if (ops_evals.size() != 4 || mem_evals.size() != 3) throw Error(PK_ERR_BAD_ARG, "ops_evals has 4 elements, mem_evals 3");
        int which = -1;
        if (int rc = pkm_check_claims(&st, &claims.raw, ops_evals[0].data(), mem_evals[0].data(), rt_eval.data(), m_eval.data(), &which)) throw Error(rc, pkm_create_error());
        return which;
    }

   private:
    pkm_statement st_;
    pkm_prover* p_ = nullptr;
};

}  // namespace provekit
