// provekit_whir.hpp -- provekit::WhirPcs: the C++ face of libprovekit_whir.so (include/provekit_whir.h), next to provekit_hip.hpp's
// prover types and provekit_verify.hpp's Verdict.  Commit to multilinear polynomials, open them at points, verify: PLAIN WHIR, not
// hiding.  A rejected proof is a Verdict, not an exception; only a failed call throws provekit::Error.
#pragma once
#include "provekit_hip.hpp"
#include "provekit_whir.h"

namespace provekit {

struct PcsVerdict {
    bool accepted;
    int check;        // PKV_CHECK_* or PKW_CHECK_*
    uint64_t offset;  // bytes of the proof consumed
    std::string message;
    const char* check_name() const { return pkw_check_name(check); }
    explicit operator bool() const { return accepted; }
};

using Point = std::vector<FieldElement>;  // n_vars coordinates, variable 0 <-> the most significant index bit

struct PcsOpening {
    std::vector<FieldElement> evaluations;  // [polynomial][point]
    std::vector<uint8_t> proof;
};

class WhirPcs;

class PcsCommitment {
   public:
    ~PcsCommitment() { pkw_commitment_destroy(c_); }
    PcsCommitment(PcsCommitment&& o) noexcept : c_(o.c_) { o.c_ = nullptr; }
    PcsCommitment(const PcsCommitment&) = delete;
    PcsCommitment& operator=(const PcsCommitment&) = delete;
    std::array<uint8_t, 32> root() const {
        std::array<uint8_t, 32> r{};
        pkw_commitment_root(c_, r.data());
        return r;
    }
    pkw_commitment* get() const { return c_; }

   private:
    friend class WhirPcs;
    explicit PcsCommitment(pkw_commitment* c) : c_(c) {}
    pkw_commitment* c_;
};

class WhirPcs {
   public:
    WhirPcs(const Context& ctx, const WhirConfig& cfg) : cfg_(cfg.to_c()) {
        if (int rc = pkw_scheme_create(ctx.get(), &cfg_, &s_)) throw Error(rc, pkw_create_error());
    }
    ~WhirPcs() { pkw_scheme_destroy(s_); }
    WhirPcs(const WhirPcs&) = delete;
    WhirPcs& operator=(const WhirPcs&) = delete;

    // evaluation tables over the hypercube, one per polynomial of the batch; copied, the caller keeps its own
    PcsCommitment commit(const std::vector<const DeviceVec*>& evals) const {
        if (evals.size() != cfg_.batch_size) throw Error(PK_ERR_BAD_ARG, "as many polynomials as the config's batch_size");
        std::vector<const uint64_t*> p;
        for (const DeviceVec* v : evals) p.push_back(v->data());
        pkw_commitment* c = nullptr;
        check(pkw_commit(s_, p.data(), &c));
        return PcsCommitment(c);
    }
    PcsOpening open(const PcsCommitment& com, const std::vector<Point>& points) const {
        const std::vector<uint64_t> flat = flatten(points, cfg_.n_vars);
        PcsOpening o;
        o.evaluations.resize((size_t)cfg_.batch_size * points.size());
        o.proof.resize(1 << 20);
        size_t len = 0;
        int rc = pkw_open(s_, com.get(), flat.data(), (unsigned)points.size(), o.evaluations[0].data(), o.proof.data(), o.proof.size(), &len);
        if (rc == PK_ERR_BAD_ARG && len > o.proof.size()) {  // the proof is larger: *len says by how much
            o.proof.resize(len);
            rc = pkw_open(s_, com.get(), flat.data(), (unsigned)points.size(), o.evaluations[0].data(), o.proof.data(), o.proof.size(), &len);
        }
        check(rc);
        o.proof.resize(len);
        return o;
    }
    // host only; evaluations_out (optional) receives what the proof binds
    static PcsVerdict verify(const WhirConfig& cfg, const std::vector<Point>& points, const std::vector<uint8_t>& proof,
                             const std::array<uint8_t, 32>* expected_root = nullptr, std::vector<FieldElement>* evaluations_out = nullptr,
                             int hash_version = 2) {
        const pk_whir_config c = cfg.to_c();
        const std::vector<uint64_t> flat = flatten(points, c.n_vars);
        std::vector<FieldElement> ev((size_t)c.batch_size * points.size());
        pkv_result r;
        if (int rc = pkw_verify(&c, nullptr, 0, hash_version, expected_root ? expected_root->data() : nullptr, flat.data(), (unsigned)points.size(),
                                proof.data(), proof.size(), ev.empty() ? nullptr : ev[0].data(), &r))
            throw Error(rc, pkw_create_error());
        if (evaluations_out) *evaluations_out = ev;
        return {r.accepted != 0, r.check, r.offset, r.message};
    }
    pkw_scheme* get() const { return s_; }

   private:
    static std::vector<uint64_t> flatten(const std::vector<Point>& points, unsigned n_vars) {
        std::vector<uint64_t> flat;
        for (const Point& p : points) {
            if (p.size() != n_vars) throw Error(PK_ERR_BAD_ARG, "a point has n_vars coordinates");
            for (const FieldElement& x : p) flat.insert(flat.end(), x.begin(), x.end());
        }
        if (flat.empty()) throw Error(PK_ERR_BAD_ARG, "at least one point");
        return flat;
    }
    void check(int rc) const {
        if (rc) throw Error(rc, pkw_last_error(s_));
    }
    pk_whir_config cfg_;
    pkw_scheme* s_ = nullptr;
};

}  // namespace provekit
