// provekit_verify.hpp -- provekit::Verifier: the C++ face of libprovekit_verify.so (include/provekit_verify.h), next to
// provekit_hip.hpp's prover types.  WhirR1CSVerifier::verify (provekit/verifier/src/whir_r1cs.rs:38-90): `verify` is the host core,
// `verify_many` the device path.  A rejected proof is a Verdict, not an exception; only a failed call throws provekit::Error.
#pragma once
#include "provekit_hip.hpp"
#include "provekit_verify.h"

namespace provekit {

struct Verdict {
    bool accepted;
    int check;        // PKV_CHECK_*
    uint64_t offset;  // bytes of the proof consumed
    std::string message;
    const char* check_name() const { return pkv_check_name(check); }
    explicit operator bool() const { return accepted; }
};

class Verifier {
   public:
    // the statement of `scheme`'s proofs, under the IO pattern the scheme has in force
    explicit Verifier(const WhirR1CSScheme& scheme, int hash_version = 2)
        : Verifier(scheme.m, scheme.m_0, scheme.whir_witness, scheme.whir_for_hiding_spartan, scheme.domain_separator(), hash_version) {}
    Verifier(unsigned m, unsigned m_0, const WhirConfig& whir_witness, const WhirConfig& whir_for_hiding_spartan, const std::string& io_pattern = "",
             int hash_version = 2) {
        const pk_whir_config cw = whir_witness.to_c(), cb = whir_for_hiding_spartan.to_c();
        if (int rc = pkv_verifier_create(m, m_0, &cw, &cb, io_pattern.empty() ? nullptr : reinterpret_cast<const uint8_t*>(io_pattern.data()),
                                         io_pattern.size(), hash_version, &v_))
            throw Error(rc, pkv_create_error());
    }
    ~Verifier() { pkv_verifier_destroy(v_); }
    Verifier(const Verifier&) = delete;
    Verifier& operator=(const Verifier&) = delete;
    // enables the matrix-evaluation check of the deferred weights; call before attach
    void set_r1cs(const SparseMatrix& a, const SparseMatrix& b, const SparseMatrix& c, const std::vector<FieldElement>& interner) {
        const SparseMatrix* ms[3] = {&a, &b, &c};
        pk_sparse_matrix mats[3];
        for (int k = 0; k < 3; k++) {
            if (ms[k]->num_rows != a.num_rows || ms[k]->num_cols != a.num_cols || ms[k]->new_row_indices.size() != a.num_rows)
                throw Error(PK_ERR_BAD_ARG, "matrix shape mismatch");
            mats[k] = {ms[k]->new_row_indices.data(), ms[k]->col_indices.data(), ms[k]->values.data(), ms[k]->col_indices.size()};
        }
        check(pkv_verifier_set_r1cs(v_, a.num_rows, a.num_cols, mats, interner.empty() ? nullptr : interner[0].data(), interner.size()));
    }
    void attach(const Context& ctx) { check(pkv_verifier_attach_device(v_, ctx.get())); }
    Verdict verify(const std::vector<uint8_t>& proof) const {
        pkv_result r;
        check(pkv_verify(v_, proof.data(), proof.size(), &r));
        return {r.accepted != 0, r.check, r.offset, r.message};
    }
    std::vector<Verdict> verify_many(const std::vector<const std::vector<uint8_t>*>& proofs) const {
        std::vector<const uint8_t*> p;
        std::vector<size_t> n;
        for (const auto* x : proofs) {
            p.push_back(x->data());
            n.push_back(x->size());
        }
        std::vector<pkv_result> r(proofs.size());
        check(pkv_verify_many(v_, p.data(), n.data(), proofs.size(), r.data()));
        std::vector<Verdict> out;
        for (const pkv_result& x : r) out.push_back({x.accepted != 0, x.check, x.offset, x.message});
        return out;
    }
    pkv_verifier* get() const { return v_; }

   private:
    void check(int rc) const {
        if (rc) throw Error(rc, pkv_last_error(v_));
    }
    pkv_verifier* v_ = nullptr;
};

}  // namespace provekit
