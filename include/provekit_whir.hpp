// provekit_whir.hpp -- provekit::WhirPcs: the C++ face of libprovekit_whir.so (include/provekit_whir.h), next to provekit_hip.hpp's
// prover types and provekit_verify.hpp's Verdict.  Commit to multilinear polynomials, open them at points or at linear statements
// over dense weight tables (provekit_whir_linear.h) or the same weights as index/value lists (provekit_whir_sparse.h), verify.  Those
// openings are plain WHIR, not hiding; commit_hiding / open_hiding / verify_hiding mask the polynomials (provekit_whir_hiding.h states
// the construction).  A rejected proof is a Verdict, not an exception; only a failed call throws provekit::Error.
#pragma once
#include "provekit_hip.hpp"
#include "provekit_whir.h"
#include "provekit_whir_hiding.h"
#include "provekit_whir_sparse.h"

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

// a linear statement's opening: <w_i, poly_b> = sums[b * l + i] next to the evaluations at the points
struct PcsLinearOpening {
    std::vector<FieldElement> evaluations;  // [polynomial][point]
    std::vector<FieldElement> sums;         // [polynomial][weight]
    std::vector<uint8_t> proof;
};

// what pkw_verify_linear hands back: with `unchecked` > 0 the verdict holds PROVIDED deferred[i] is the multilinear extension of
// weight i at fold_point, for every weight whose table the verifier was not given
struct PcsLinearVerdict {
    PcsVerdict verdict;
    std::vector<FieldElement> evaluations, sums;
    Point fold_point;
    std::vector<FieldElement> deferred;  // one per weight
    unsigned unchecked = 0;
    explicit operator bool() const { return verdict.accepted; }
};

// l sparse weights on the host (provekit_whir_sparse.h): weight i owns entries offsets[i] .. offsets[i + 1]; indexes increase
// strictly within a weight.  add() appends one weight
struct PcsSparseWeights {
    std::vector<uint64_t> offsets{0};
    std::vector<uint32_t> index;
    std::vector<FieldElement> value;
    void add(const std::vector<uint32_t>& idx, const std::vector<FieldElement>& val) {
        if (idx.size() != val.size()) throw Error(PK_ERR_BAD_ARG, "as many values as indexes");
        index.insert(index.end(), idx.begin(), idx.end());
        value.insert(value.end(), val.begin(), val.end());
        offsets.push_back(index.size());
    }
    unsigned count() const { return (unsigned)offsets.size() - 1; }
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

// a commitment to the caller's polynomials under masks (provekit_whir_hiding.h): opened once
class PcsHidingCommitment {
   public:
    ~PcsHidingCommitment() { pkw_hiding_commitment_destroy(c_); }
    PcsHidingCommitment(PcsHidingCommitment&& o) noexcept : c_(o.c_) { o.c_ = nullptr; }
    PcsHidingCommitment(const PcsHidingCommitment&) = delete;
    PcsHidingCommitment& operator=(const PcsHidingCommitment&) = delete;
    std::array<uint8_t, 32> root() const {
        std::array<uint8_t, 32> r{};
        pkw_hiding_commitment_root(c_, r.data());
        return r;
    }
    pkw_hiding_commitment* get() const { return c_; }

   private:
    friend class WhirPcs;
    explicit PcsHidingCommitment(pkw_hiding_commitment* c) : c_(c) {}
    pkw_hiding_commitment* c_;
};

class WhirPcs {
   public:
    WhirPcs(const Context& ctx, const WhirConfig& cfg) : cfg_(cfg.to_c()) {
        if (int rc = pkw_scheme_create(ctx.get(), &cfg_, &s_)) throw Error(rc, pkw_create_error());
    }
    // The scheme of hiding commitments: cfg describes the EXTENDED batch (n_vars = n + 1, batch_size = B + 1) and must keep their two
    // rules.  A factory of its own, so that only its callers name pkw_hiding_scheme_create
    static WhirPcs hiding(const Context& ctx, const WhirConfig& cfg) {
        const pk_whir_config c = cfg.to_c();
        pkw_scheme* s = nullptr;
        if (int rc = pkw_hiding_scheme_create(ctx.get(), &c, &s)) throw Error(rc, pkw_create_error());
        return WhirPcs(c, s);
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
        PcsLinearOpening o = open_with(points.size(), 0, [&](uint64_t* evals, uint64_t*, uint8_t* proof, size_t cap, size_t* len) {
            return pkw_open(s_, com.get(), flat.data(), (unsigned)points.size(), evals, proof, cap, len);
        });
        return {std::move(o.evaluations), std::move(o.proof)};
    }
    // host only; evaluations_out (optional) receives what the proof binds
    static PcsVerdict verify(const WhirConfig& cfg, const std::vector<Point>& points, const std::vector<uint8_t>& proof,
                             const std::array<uint8_t, 32>* expected_root = nullptr, std::vector<FieldElement>* evaluations_out = nullptr,
                             int hash_version = 2) {
        const pk_whir_config c = cfg.to_c();
        const std::vector<uint64_t> flat = flatten(points, c.n_vars);
        const PcsLinearVerdict out = verify_with(c, points.size(), 0, [&](uint64_t* evals, uint64_t*, uint64_t*, uint64_t*, unsigned*, pkv_result* r) {
            return pkw_verify(&c, nullptr, 0, hash_version, root_ptr(expected_root), flat.data(), (unsigned)points.size(), proof.data(), proof.size(), evals, r);
        });
        if (evaluations_out) *evaluations_out = out.evaluations;
        return out.verdict;
    }
    // q >= 0 points and l >= 1 dense weight tables on the device, bound by the caller's tags (provekit_whir.h, "TAGS AND SOUNDNESS")
    PcsLinearOpening open_linear(const PcsCommitment& com, const std::vector<Point>& points, const std::vector<const DeviceVec*>& weights,
                                 const std::vector<FieldElement>& tags) const {
        if (weights.size() != tags.size()) throw Error(PK_ERR_BAD_ARG, "as many tags as weights");
        const std::vector<uint64_t> flat = flatten(points, cfg_.n_vars, /*may_be_empty=*/true);
        std::vector<const uint64_t*> w;
        for (const DeviceVec* v : weights) w.push_back(v->data());
        return open_with(points.size(), weights.size(), [&](uint64_t* evals, uint64_t* sums, uint8_t* proof, size_t cap, size_t* len) {
            return pkw_open_linear(s_, com.get(), flat.data(), (unsigned)points.size(), w.data(), ptr(tags), (unsigned)weights.size(), evals, sums, proof, cap,
                                   len);
        });
    }
    // host only.  weights: host tables (2^n_vars elements each), or nullptr entries / an empty vector for "not given"
    static PcsLinearVerdict verify_linear(const WhirConfig& cfg, const std::vector<Point>& points, const std::vector<FieldElement>& tags,
                                          const std::vector<const std::vector<FieldElement>*>& weights, const std::vector<uint8_t>& proof,
                                          const std::array<uint8_t, 32>* expected_root = nullptr, int hash_version = 2) {
        const pk_whir_config c = cfg.to_c();
        const std::vector<uint64_t> flat = flatten(points, c.n_vars, /*may_be_empty=*/true);
        if (!weights.empty() && weights.size() != tags.size()) throw Error(PK_ERR_BAD_ARG, "as many weights as tags, or none");
        std::vector<const uint64_t*> w;
        for (const std::vector<FieldElement>* t : weights) {
            if (t && t->size() != (size_t)1 << c.n_vars) throw Error(PK_ERR_BAD_ARG, "a weight table has 2^n_vars elements");
            w.push_back(t ? (*t)[0].data() : nullptr);
        }
        return verify_with(c, points.size(), tags.size(),
                           [&](uint64_t* evals, uint64_t* sums, uint64_t* fold, uint64_t* deferred, unsigned* unchecked, pkv_result* r) {
                               return pkw_verify_linear(&c, nullptr, 0, hash_version, root_ptr(expected_root), flat.data(), (unsigned)points.size(), ptr(tags),
                                                        w.empty() ? nullptr : w.data(), (unsigned)tags.size(), proof.data(), proof.size(), evals, sums, fold,
                                                        deferred, unchecked, r);
                           });
    }
    // open_linear with the weights as lists: the same statement and the same bytes.  The lists are copied to the device for the
    // call (a caller that keeps them there calls pkw_open_sparse); the library validates the indexes before it uses one
    PcsLinearOpening open_sparse(const Context& ctx, const PcsCommitment& com, const std::vector<Point>& points, const PcsSparseWeights& weights,
                                 const std::vector<FieldElement>& tags) const {
        if (weights.count() != tags.size()) throw Error(PK_ERR_BAD_ARG, "as many tags as weights");
        const std::vector<uint64_t> flat = flatten(points, cfg_.n_vars, /*may_be_empty=*/true);
        const size_t entries = weights.index.size();
        const DeviceVec d_value(ctx, weights.value), d_index(ctx, (entries + 7) / 8);  // 8 indexes per 32 bytes
        if (entries) ctx.check(pk_memcpy_h2d(ctx.get(), d_index.data(), weights.index.data(), 4 * entries));
        return open_with(points.size(), tags.size(), [&](uint64_t* evals, uint64_t* sums, uint8_t* proof, size_t cap, size_t* len) {
            return pkw_open_sparse(s_, com.get(), flat.data(), (unsigned)points.size(), weights.offsets.data(), reinterpret_cast<const uint32_t*>(d_index.data()),
                                   d_value.data(), ptr(tags), weights.count(), evals, sums, proof, cap, len);
        });
    }
    // host only; every weight's deferred value is judged from its entries: `unchecked` stays 0 and the verdict is unconditional
    static PcsLinearVerdict verify_sparse(const WhirConfig& cfg, const std::vector<Point>& points, const std::vector<FieldElement>& tags,
                                          const PcsSparseWeights& weights, const std::vector<uint8_t>& proof,
                                          const std::array<uint8_t, 32>* expected_root = nullptr, int hash_version = 2) {
        const pk_whir_config c = cfg.to_c();
        const std::vector<uint64_t> flat = flatten(points, c.n_vars, /*may_be_empty=*/true);
        if (weights.count() != tags.size()) throw Error(PK_ERR_BAD_ARG, "as many weights as tags");
        return verify_with(c, points.size(), tags.size(), [&](uint64_t* evals, uint64_t* sums, uint64_t* fold, uint64_t* deferred, unsigned*, pkv_result* r) {
            return pkw_verify_sparse(&c, nullptr, 0, hash_version, root_ptr(expected_root), flat.data(), (unsigned)points.size(), ptr(tags),
                                     weights.offsets.data(), weights.index.empty() ? nullptr : weights.index.data(), ptr(weights.value), weights.count(),
                                     proof.data(), proof.size(), evals, sums, fold, deferred, r);
        });
    }
    // batch_size - 1 tables of 2^(n_vars - 1) evaluations; the masks and g are drawn on the device.  seed: a test hook, nullptr
    // takes the key from the OS
    PcsHidingCommitment commit_hiding(const std::vector<const DeviceVec*>& evals, const std::array<uint8_t, 32>* seed = nullptr) const {
        if (evals.size() + 1 != cfg_.batch_size) throw Error(PK_ERR_BAD_ARG, "one polynomial fewer than the config's batch_size");
        std::vector<const uint64_t*> p;
        for (const DeviceVec* v : evals) p.push_back(v->data());
        pkw_hiding_commitment* c = nullptr;
        check(pkw_commit_hiding(s_, p.data(), seed ? seed->data() : nullptr, &c));
        return PcsHidingCommitment(c);
    }
    // points of n_vars - 1 coordinates; evaluations [polynomial][point] of the caller's polynomials.  Once per commitment
    PcsOpening open_hiding(PcsHidingCommitment& com, const std::vector<Point>& points) const {
        const std::vector<uint64_t> flat = flatten(points, cfg_.n_vars - 1);
        PcsLinearOpening o = open_with(points.size(), 0, [&](uint64_t* evals, uint64_t*, uint8_t* proof, size_t cap, size_t* len) {
            return pkw_open_hiding(s_, com.get(), flat.data(), (unsigned)points.size(), evals, proof, cap, len);
        });
        o.evaluations.resize((cfg_.batch_size - 1) * points.size());
        return {std::move(o.evaluations), std::move(o.proof)};
    }
    // host only; evaluations_out (optional) receives f_b(z_i) as the proof binds them
    static PcsVerdict verify_hiding(const WhirConfig& cfg, const std::vector<Point>& points, const std::vector<uint8_t>& proof,
                                    const std::array<uint8_t, 32>* expected_root = nullptr, std::vector<FieldElement>* evaluations_out = nullptr,
                                    int hash_version = 2) {
        const pk_whir_config c = cfg.to_c();
        if (c.n_vars < 2 || c.batch_size < 2) throw Error(PK_ERR_BAD_ARG, "not a hiding config");
        const std::vector<uint64_t> flat = flatten(points, c.n_vars - 1);
        PcsLinearVerdict out = verify_with(c, points.size(), 0, [&](uint64_t* evals, uint64_t*, uint64_t*, uint64_t*, unsigned*, pkv_result* r) {
            return pkw_verify_hiding(&c, nullptr, 0, hash_version, root_ptr(expected_root), flat.data(), (unsigned)points.size(), proof.data(), proof.size(), evals,
                                     r);
        });
        out.evaluations.resize((c.batch_size - 1) * points.size());
        if (evaluations_out) *evaluations_out = out.evaluations;
        return out.verdict;
    }
    pkw_scheme* get() const { return s_; }

   private:
    WhirPcs(const pk_whir_config& c, pkw_scheme* s) : cfg_(c), s_(s) {}
    static std::vector<uint64_t> flatten(const std::vector<Point>& points, unsigned n_vars, bool may_be_empty = false) {
        std::vector<uint64_t> flat;
        for (const Point& p : points) {
            if (p.size() != n_vars) throw Error(PK_ERR_BAD_ARG, "a point has n_vars coordinates");
            for (const FieldElement& x : p) flat.insert(flat.end(), x.begin(), x.end());
        }
        if (flat.empty() && !may_be_empty) throw Error(PK_ERR_BAD_ARG, "at least one point");
        if (flat.empty()) flat.resize(4);  // a valid pointer for q = 0
        return flat;
    }
    void check(int rc) const {
        if (rc) throw Error(rc, pkw_last_error(s_));
    }
    static const uint64_t* ptr(const std::vector<FieldElement>& v) { return v.empty() ? nullptr : v[0].data(); }
    static uint64_t* ptr(std::vector<FieldElement>& v) { return v.empty() ? nullptr : v[0].data(); }
    static const uint8_t* root_ptr(const std::array<uint8_t, 32>* root) { return root ? root->data() : nullptr; }
    // An opening at q points and l weights: call(evals, sums, proof, cap, &len) writes into buffers this owns; the proof buffer grows
    // once when *len says the proof is larger
    template <class Call>
    PcsLinearOpening open_with(size_t q, size_t l, Call call) const {
        PcsLinearOpening o;
        o.evaluations.resize(cfg_.batch_size * q);
        o.sums.resize(cfg_.batch_size * l);
        o.proof.resize(1 << 20);
        size_t len = 0;
        int rc = call(ptr(o.evaluations), ptr(o.sums), o.proof.data(), o.proof.size(), &len);
        if (rc == PK_ERR_BAD_ARG && len > o.proof.size()) {
            o.proof.resize(len);
            rc = call(ptr(o.evaluations), ptr(o.sums), o.proof.data(), o.proof.size(), &len);
        }
        check(rc);
        o.proof.resize(len);
        return o;
    }
    // A verification of q points and l weights: call(evals, sums, fold, deferred, &unchecked, &result) fills outputs sized here
    template <class Call>
    static PcsLinearVerdict verify_with(const pk_whir_config& c, size_t q, size_t l, Call call) {
        PcsLinearVerdict out;
        out.evaluations.resize(c.batch_size * q);
        out.sums.resize(c.batch_size * l);
        out.fold_point.resize(c.n_vars);
        out.deferred.resize(l);
        std::vector<uint64_t> fold(4 * (size_t)c.n_vars + 4);  // flat storage: a valid pointer whatever n_vars is
        pkv_result r;
        if (int rc = call(ptr(out.evaluations), ptr(out.sums), fold.data(), ptr(out.deferred), &out.unchecked, &r)) throw Error(rc, pkw_create_error());
        for (unsigned j = 0; j < c.n_vars; j++) std::copy(fold.begin() + 4 * j, fold.begin() + 4 * j + 4, out.fold_point[j].begin());
        out.verdict = {r.accepted != 0, r.check, r.offset, r.message};
        return out;
    }
    pk_whir_config cfg_;
    pkw_scheme* s_ = nullptr;
};

}  // namespace provekit
