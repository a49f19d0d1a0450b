// provekit_bitwise.hpp -- provekit::Bitwise: the C++ face of libprovekit_bitwise.so (include/provekit_bitwise.h), next to
// provekit_rangecheck.hpp's RangeCheck.  Prove that a device column c is a AND / XOR / OR b, entry by entry, on words of L digits of d
// bits, by digit rows looked up in the operation's table; `decompose` builds c, the digit columns and the multiplicities on the device;
// verify on the host.  An accepted proof is accepted PROVIDED the five claims of BitwiseClaims: WhirPcs::open / WhirPcs::verify give the
// evaluations of a, b, c and the digit columns at z_lo and of m at z_t, Bitwise::check_claims forms the combinations.  A rejected proof
// is a verdict, not an exception; only a failed call throws provekit::Error.
#pragma once
#include "provekit_bitwise.h"
#include "provekit_hip.hpp"

namespace provekit {

struct BitwiseClaims {
    pkb_claims raw;                       // what check_claims reads
    std::vector<FieldElement> z_lo, z_t;  // the points, variable 0 first: a, b, c and every digit column are opened at z_lo, m at z_t
    FieldElement digits_value, m_value;
    static BitwiseClaims from(const pkb_statement& st, const pkb_claims& c) {
        auto fe = [](const uint64_t* p) { return FieldElement{p[0], p[1], p[2], p[3]}; };
        BitwiseClaims o;
        o.raw = c;
        o.digits_value = fe(c.digits_value), o.m_value = fe(c.m_value);
        for (unsigned i = 0; i < st.n; i++) o.z_lo.push_back(fe(c.z_lo[i]));
        for (unsigned i = 0; i < 2 * st.d; i++) o.z_t.push_back(fe(c.z_t[i]));
        return o;
    }
};

struct BitwiseProof {
    std::vector<uint8_t> proof;
    BitwiseClaims claims;
};

struct BitwiseVerdict {
    bool accepted;
    int check;  // PKV_CHECK_*, PKS_CHECK_*, PKF_CHECK_* or PKB_CHECK_TABLE
    int side;   // PKT_SIDE_*
    unsigned layer;
    uint64_t offset;
    std::string message;
    BitwiseClaims claims;  // when accepted
    const char* check_name() const { return pkb_check_name(check); }
    explicit operator bool() const { return accepted; }
};

class Bitwise {
   public:
    // the plan of a statement; a statement the library does not take throws with its reason
    static pkb_digit_plan plan(const pkb_statement& st) {
        pkb_digit_plan p;
        if (int rc = pkb_plan(&st, &p)) throw Error(rc, pkb_create_error());
        return p;
    }

    Bitwise(const Context& ctx, unsigned n, unsigned op, unsigned d, unsigned L, unsigned n_bind = 0) : st_{n, op, d, L, n_bind} {
        if (int rc = pkb_prover_create(ctx.get(), &st_, &p_)) throw Error(rc, pkb_create_error());
    }
    ~Bitwise() { pkb_prover_destroy(p_); }
    Bitwise(const Bitwise&) = delete;
    Bitwise& operator=(const Bitwise&) = delete;
    const pkb_statement& statement() const { return st_; }

    // a, b (2^n elements) -> c = a op b (c_given: c is read and compared), the 3 L digit columns digits_out[j L + i] (2^n elements each)
    // and m (2^(2d) elements).  An operand >= 2^bits or a given c that differs throws with code PK_ERR_UNSATISFIED; *first_bad: the
    // smallest such entry
    void decompose(const DeviceVec& a, const DeviceVec& b, DeviceVec& c, bool c_given, const std::vector<DeviceVec*>& digits_out, DeviceVec& m,
                   uint64_t* first_bad = nullptr) const {
        const size_t N = (size_t)1 << st_.n;
        if (a.size() != N || b.size() != N || c.size() != N || digits_out.size() != 3 * st_.L || m.size() != (size_t)1 << (2 * st_.d))
            throw Error(PK_ERR_BAD_ARG, "a, b, c have 2^n elements, there are 3 L digit columns, m has 2^(2d) elements");
        std::vector<uint64_t*> out;
        for (DeviceVec* v : digits_out) {
            if (!v || v->size() != N) throw Error(PK_ERR_BAD_ARG, "a digit column has 2^n elements");
            out.push_back(v->data());
        }
        if (int rc = pkb_decompose(p_, a.data(), b.data(), c.data(), c_given ? 1 : 0, out.data(), m.data(), first_bad)) throw Error(rc, pkb_last_error(p_));
    }

    // a digit row outside the table or a wrong m throws with code PK_ERR_UNSATISFIED and a reason that names the digit and the entry; the
    // prover stays usable
    BitwiseProof prove(const std::vector<const DeviceVec*>& digits, const DeviceVec& m, const std::vector<FieldElement>& bind = {}) const {
        if (digits.size() != 3 * st_.L || m.size() != (size_t)1 << (2 * st_.d) || bind.size() != st_.n_bind)
            throw Error(PK_ERR_BAD_ARG, "there are 3 L digit columns, m has 2^(2d) elements, bind the statement's count");
        std::vector<const uint64_t*> in;
        for (const DeviceVec* v : digits) {
            if (!v || v->size() != (size_t)1 << st_.n) throw Error(PK_ERR_BAD_ARG, "a digit column has 2^n elements");
            in.push_back(v->data());
        }
        size_t len = 0;
        pkb_proof_bytes(&st_, &len);
        BitwiseProof out;
        out.proof.resize(len);
        pkb_claims c;
        if (int rc = pkb_prove(p_, in.data(), m.data(), bind.empty() ? nullptr : bind[0].data(), out.proof.data(), out.proof.size(), &len, &c))
            throw Error(rc, pkb_last_error(p_));
        out.claims = BitwiseClaims::from(st_, c);
        return out;
    }

    // host only
    static BitwiseVerdict verify(const pkb_statement& st, const std::vector<uint8_t>& proof, const std::vector<FieldElement>& bind = {}) {
        if (bind.size() != st.n_bind) throw Error(PK_ERR_BAD_ARG, "bind must have the statement's count");
        pkb_claims c;
        pkv_result r;
        int side = 0;
        unsigned layer = 0;
        const int rc = pkb_verify(&st, nullptr, 0, bind.empty() ? nullptr : bind[0].data(), proof.data(), proof.size(), &c, &side, &layer, &r);
        if (rc) throw Error(rc, pkb_create_error());
        BitwiseVerdict v{r.accepted != 0, r.check, side, layer, r.offset, r.message, {}};
        if (v.accepted) v.claims = BitwiseClaims::from(st, c);
        return v;
    }

    // host only: abc_evals = a, b, c at z_lo, digit_evals[j L + i] = digit_{j,i}(z_lo), m_eval = m(z_t) -> PKB_CLAIM_NONE when the five
    // claims hold, else the first that does not
    static int check_claims(const pkb_statement& st, const BitwiseClaims& claims, const std::vector<FieldElement>& abc_evals, const std::vector<FieldElement>& digit_evals,
                            const FieldElement& m_eval) {
        if (abc_evals.size() != 3 || digit_evals.size() != 3 * st.L) throw Error(PK_ERR_BAD_ARG, "abc_evals has 3 elements, digit_evals 3 L");
        int which = -1;
        if (int rc = pkb_check_claims(&st, &claims.raw, abc_evals[0].data(), digit_evals[0].data(), m_eval.data(), &which)) throw Error(rc, pkb_create_error());
        return which;
    }

   private:
    pkb_statement st_;
    pkb_prover* p_ = nullptr;
};

}  // namespace provekit
