// core.hpp -- the host core of libprovekit_verify.so: WhirR1CSVerifier::verify on one thread, no device.
//
// Restates provekit/verifier/src/whir_r1cs.rs:38-90,110-172 and whir's verifier as the Go circuit spells it
// (recursive-verifier/app/circuit/whir.go:51-220, whir_utilities.go:13-186, mtUtilities.go:12-114, utilities/utilities.go:15-190)
// against this repository's wire format (protocol.hpp, shared with the prover): the checks and their order are the acceptance oracle's.
//
// One body serves the host core and the device path (verify.hip).  The three data-parallel pieces -- does an opening reach its
// root, an opening's fold value, the bilinear forms over the R1CS matrices -- go through a Backend:
//   HostBackend    computes them here;
//   a recorder     (device path, pass 1) notes the work and answers with placeholders; from its first placeholder on the walk
//                  is "tainted": relations between scalars are no longer judged, framing and Fiat-Shamir checks still are;
//   a replayer     (pass 2) answers with what the kernels computed, so pass 2 IS the host core on the same values: same
//                  verdict, same failing check, by construction.
// Nothing here throws on its own; allocation failures surface as std::bad_alloc and are caught at the C boundary.  Every count
// read from a proof is bounded by the bytes that remain before anything is reserved.
#pragma once
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/provekit_verify.h"
#include "../protocol.hpp"
#include "../skyscraper29.hpp"

namespace pkv {

using pk::fe;
using pk::HintFe;
using pk::load_raw;
using pk::Rd;

struct Statement {
    unsigned m = 0, m_0 = 0;
    pk_whir_config w{}, b{};
    std::string pattern;
    std::vector<pk::IoOp> ops;
    int hash_version = 2;
    bool has_r1cs = false;
    size_t nc = 0, nw = 0;
    std::vector<uint32_t> rows[3], cols[3], vals[3];  // one entry per non-zero (rows expanded from the CSR offsets)
    std::vector<fe> interner;                         // Montgomery
};

// ---- field helpers above protocol.hpp's ---------------------------------------------------------------------------------------
inline fe f_one() { return pk::fe_one(); }
inline fe f_zero() { return pk::fe_zero(); }
// compress on canonical values (any 256-bit input is taken mod p, as the reference's permutation does)
inline fe h_compress(int version, const fe& l, const fe& r) {
    if (version == 2) {
        fe a = pk::fe_reduce_any(l), b = pk::fe_reduce_any(r), l0 = a;
        pk::sky_permute_host(a, b);
        return pk::fe_add(a, l0);
    }
    return pk::pack29(pk::compress29<1, true>(pk::unpack_reduce29(l), pk::unpack_reduce29(r)));
}

// ---- the verdict -------------------------------------------------------------------------------------------------------------
struct Verdict {
    bool failed = false;
    int check = PKV_CHECK_NONE;
    uint64_t offset = 0;
    std::string message;
};
inline void to_result(const Verdict& v, pkv_result* r) {
    memset(r, 0, sizeof *r);
    r->accepted = v.failed ? 0 : 1;
    r->check = v.failed ? v.check : PKV_CHECK_NONE;
    r->offset = v.offset;
    snprintf(r->message, sizeof r->message, "%s", v.failed ? v.message.c_str() : "");
}

// ---- one round's openings, as the backend sees them --------------------------------------------------------------------------
struct RoundOpenings {
    size_t k = 0;
    unsigned width = 0, depth = 0;
    std::vector<const uint8_t*> leaves;    // k: width canonical elements each, contiguous in the proof
    std::vector<const uint8_t*> siblings;  // k
    std::vector<const uint8_t*> paths;     // k * depth, root -> leaf order
    std::vector<uint64_t> indices;         // k
    fe root;                               // canonical
    std::vector<fe> weights;               // width, Montgomery: fold_i = sum_j leaf_i[j] * weights[j]
};
struct Backend {
    bool tainted = false;  // set by a backend that answers with placeholders
    // reached[i] = 1 when opening i ends in ro.root; folds[i] = its fold value (Montgomery)
    virtual void openings(int hash_version, const RoundOpenings& ro, std::vector<uint8_t>& reached, std::vector<fe>& folds) = 0;
    // eq(alpha)^T M_k eq(point), k = A, B, C (Montgomery); point = the folding point without its first coordinate
    virtual void matrix_evaluations(const Statement& st, const std::vector<fe>& alpha, const std::vector<fe>& point, fe out[3]) = 0;
    virtual ~Backend() {}
};

inline void eq_table_host(const std::vector<fe>& r, std::vector<fe>& out) {  // sumcheck.rs:146-171, variable 0 <-> MSB
    out.assign((size_t)1 << r.size(), f_zero());
    out[0] = f_one();
    size_t len = 1;
    for (size_t j = 0; j < r.size(); j++) {  // after step j: out[0..2^(j+1)) indexed by the j+1 leading variables
        for (size_t i = len; i-- > 0;) {
            const fe hi = pk::h_mul(out[i], r[j]);
            out[2 * i + 1] = hi;
            out[2 * i] = pk::h_sub(out[i], hi);
        }
        len *= 2;
    }
}

struct HostBackend : Backend {
    void openings(int ver, const RoundOpenings& ro, std::vector<uint8_t>& reached, std::vector<fe>& folds) override {
        reached.assign(ro.k, 0);
        folds.assign(ro.k, f_zero());
        for (size_t q = 0; q < ro.k; q++) {
            const uint8_t* lp = ro.leaves[q];
            fe h = pk::fe_reduce_any(load_raw(lp));
            fe acc = pk::h_mul(h, ro.weights[0]);
            for (unsigned j = 1; j < ro.width; j++) {
                const fe x = pk::fe_reduce_any(load_raw(lp + 32 * j));
                h = h_compress(ver, h, x);
                acc = pk::h_add(acc, pk::h_mul(x, ro.weights[j]));
            }
            uint64_t i = ro.indices[q];
            const fe s = load_raw(ro.siblings[q]);
            h = (i & 1) ? h_compress(ver, s, h) : h_compress(ver, h, s);
            i >>= 1;
            for (unsigned d = ro.depth; d-- > 0;) {
                const fe node = load_raw(ro.paths[q * ro.depth + d]);
                h = (i & 1) ? h_compress(ver, node, h) : h_compress(ver, h, node);
                i >>= 1;
            }
            reached[q] = pk::fe_eq(h, ro.root) ? 1 : 0;
            folds[q] = pk::h_from_canon(acc);  // canonical leaf x Montgomery weight = canonical sum
        }
    }
    void matrix_evaluations(const Statement& st, const std::vector<fe>& alpha, const std::vector<fe>& point, fe out[3]) override {
        std::vector<fe> eq_a, eq_y;
        eq_table_host(alpha, eq_a);
        eq_table_host(point, eq_y);
        for (int k = 0; k < 3; k++) {
            fe acc = f_zero();
            const size_t nnz = st.rows[k].size();
            for (size_t e = 0; e < nnz; e++)
                acc = pk::h_add(acc, pk::h_mul(pk::h_mul(st.interner[st.vals[k][e]], eq_a[st.rows[k][e]]), eq_y[st.cols[k][e]]));
            out[k] = acc;
        }
    }
};

// ---- the verifier side of the transcript (spongefish VerifierState): protocol.hpp's sponge and cursor over a bounded byte source ----
class Arthur {
  public:
    Arthur(const Statement& st, const uint8_t* t, size_t len, Verdict& v) : t_(t), len_(len), sponge_(st.pattern), cur_(st.ops), v_(v) {}
    size_t pos() const { return i_; }
    size_t remaining() const { return len_ - i_; }
    bool fail(int check, const std::string& msg) {
        if (!v_.failed) {
            v_.failed = true;
            v_.check = check;
            v_.offset = i_;
            v_.message = msg;
        }
        return false;
    }
    // canonical values as read (canon_out, may be NULL) and their Montgomery images (mont_out)
    bool next_scalars(size_t n, fe* mont_out, fe* canon_out = nullptr) {
        if (!expect('A', n)) return false;
        for (size_t k = 0; k < n; k++) {
            const uint8_t* p;
            if (!read(32, p)) return false;
            const fe c = load_raw(p);
            if (!pk::is_canonical(c)) return fail(PKV_CHECK_NON_CANONICAL, "non-canonical scalar");
            sponge_.absorb(c);
            if (canon_out) canon_out[k] = c;
            mont_out[k] = pk::fe_to_montx(c);
        }
        return true;
    }
    bool challenge_scalars(size_t n, fe* out) {
        if (!expect('S', n)) return false;
        for (size_t k = 0; k < n; k++) out[k] = pk::fe_to_montx(sponge_.squeeze());
        return true;
    }
    bool challenge_bytes(size_t n, uint8_t* out) {
        if (!expect('S', pk::units_for_bytes(n))) return false;
        sponge_.squeeze_bytes(out, n);
        return true;
    }
    bool next_bytes(size_t n, uint8_t* out) {
        if (!expect('A', n)) return false;
        const uint8_t* p;
        if (!read(n, p)) return false;
        sponge_.absorb_bytes(p, n);
        memcpy(out, p, n);
        return true;
    }
    bool hint(const uint8_t*& p, size_t& n) {
        if (!expect('H', 1)) return false;
        const uint8_t* lp;
        pk::hint_len_t ln;
        if (!read(sizeof ln, lp)) return false;
        memcpy(&ln, lp, sizeof ln);
        n = ln;
        return read(ln, p);
    }
    bool done() const { return i_ == len_ && cur_.at_end(); }

  private:
    const uint8_t* t_;
    size_t len_, i_ = 0;
    pk::DuplexSponge sponge_;
    pk::IoCursor cur_;
    Verdict& v_;
    bool read(size_t n, const uint8_t*& p) {
        if (n > len_ - i_) return fail(PKV_CHECK_TRANSCRIPT_SHORT, "transcript too short");
        p = t_ + i_;
        i_ += n;
        return true;
    }
    bool expect(char kind, size_t n) {
        if (cur_.take(kind, n)) return true;
        return fail(PKV_CHECK_IO_PATTERN, std::string("operation ") + kind + std::to_string(n) + " does not follow the IO pattern (operation #" +
                                              std::to_string(cur_.op_index() + 1) + ")");
    }
};

// ---- algebra -----------------------------------------------------------------------------------------------------------------
inline fe eq_poly(const fe* a, const fe* b, size_t n) {  // EqPolyOutside
    fe acc = f_one();
    for (size_t i = 0; i < n; i++) {
        const fe xy = pk::h_mul(a[i], b[i]);
        // x y + (1-x)(1-y) = 1 - x - y + 2 x y
        acc = pk::h_mul(acc, pk::h_sub(pk::h_add(pk::h_add(xy, xy), f_one()), pk::h_add(a[i], b[i])));
    }
    return acc;
}
inline fe quad_from_evals(const fe* ev, const fe& x) {  // utilities.go:148-154
    const fe half = pk::h_half();
    const fe two1 = pk::h_add(ev[1], ev[1]), four1 = pk::h_add(two1, two1), three0 = pk::h_add(pk::h_add(ev[0], ev[0]), ev[0]);
    const fe b1 = pk::h_mul(pk::h_sub(pk::h_sub(four1, ev[2]), three0), half);
    const fe b2 = pk::h_mul(pk::h_add(pk::h_sub(ev[2], two1), ev[0]), half);
    return pk::h_add(pk::h_add(pk::h_mul(pk::h_mul(x, x), b2), pk::h_mul(x, b1)), ev[0]);
}
inline std::vector<fe> expand_randomness(const fe& base, size_t n) {
    std::vector<fe> out(n);
    fe acc = f_one();
    for (size_t i = 0; i < n; i++) {
        out[i] = acc;
        acc = pk::h_mul(acc, base);
    }
    return out;
}
inline fe multivar_poly(std::vector<fe> c, const std::vector<fe>& vs) {  // utilities.go:15-22: vs[t] <-> index bit t
    size_t len = c.size();
    for (size_t t = vs.size(); t-- > 0;) {
        len /= 2;
        for (size_t i = 0; i < len; i++) c[i] = pk::h_add(c[i], pk::h_mul(vs[t], c[i + len]));
    }
    return c[0];
}
inline fe eval_univariate(const std::vector<fe>& c, const fe& z) {
    fe acc = f_zero();
    for (size_t i = c.size(); i-- > 0;) acc = pk::h_add(pk::h_mul(acc, z), c[i]);
    return acc;
}
inline fe mle_eval_table(std::vector<fe> v, const std::vector<fe>& point) {  // variable 0 <-> MSB
    size_t len = v.size();
    for (const fe& x : point) {
        len /= 2;
        for (size_t i = 0; i < len; i++) v[i] = pk::h_add(v[i], pk::h_mul(x, pk::h_sub(v[i + len], v[i])));
    }
    return v[0];
}

// ---- the statement's shape: what a prover of this library accepts --------------------------------------------------------------
// max_fold: pk_scheme_create takes folding factors up to 8 (whir_config.hip whir_config_error) and so does the walk of its proofs
// (statement_ok); libprovekit_whir's prover stops at 4 (whir_pcs/pcs.hpp config_ok)
inline bool config_ok(const pk_whir_config& c, std::string& why, unsigned max_fold = 4) {
    auto bad = [&](const char* s) {
        why = s;
        return false;
    };
    if (c.folding_factor < 1 || c.folding_factor > max_fold) return bad(max_fold == 4 ? "folding_factor must be 1..4" : "folding_factor must be 1..8");
    if (c.batch_size < 1 || c.batch_size > 4) return bad("batch_size must be 1..4");
    if (c.n_rounds > PK_MAX_WHIR_ROUNDS) return bad("too many WHIR rounds");
    if (c.n_vars > 28 || c.starting_log_inv_rate < 1 || c.n_vars + c.starting_log_inv_rate > 28) return bad("n_vars + log_inv_rate must be <= 28");
    if ((uint64_t)c.folding_factor * (c.n_rounds + 1) > c.n_vars) return bad("n_vars < folding_factor * (rounds + 1)");
    if (c.n_vars - c.folding_factor * (c.n_rounds + 1) > 16) return bad("final polynomial too large");
    // the tree opened in round r has 2^(n + rate - r - fold) leaves; at least two
    if (c.n_vars + c.starting_log_inv_rate < c.n_rounds + c.folding_factor + 1) return bad("a round's tree would have fewer than two leaves");
    if (c.commitment_ood_samples > 8) return bad("too many OOD samples");
    for (unsigned r = 0; r < c.n_rounds; r++) {
        if (c.ood_samples[r] > 8) return bad("too many OOD samples");
        if (c.num_queries[r] > (1u << 16)) return bad("too many queries");
        if (!(c.pow_bits[r] < 80.0)) return bad("pow_bits must be below 80");
    }
    if (c.final_queries > (1u << 16)) return bad("too many queries");
    if (!(c.final_pow_bits < 80.0) || !(c.final_folding_pow_bits < 80.0)) return bad("pow_bits must be below 80");
    return true;
}
inline bool statement_ok(const Statement& st, std::string& why) {
    if (st.m < 1 || st.m_0 < 1 || st.m_0 > 28) {
        why = "m / m_0 out of range";
        return false;
    }
    if (st.hash_version != 1 && st.hash_version != 2) {
        why = "hash version must be 1 or 2";
        return false;
    }
    if (!config_ok(st.w, why, 8) || !config_ok(st.b, why, 8)) return false;
    if (st.w.n_vars != st.m) {
        why = "whir_witness.n_vars must equal m";
        return false;
    }
    if (st.b.n_vars > 12 || ((size_t)1 << st.b.n_vars) < 4 * (size_t)st.m_0) {
        why = "whir_for_hiding_spartan.n_vars does not hold the 4*m_0 blinding coefficients";
        return false;
    }
    return true;
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------
class Walk {
  public:
    Walk(const Statement& st, Backend& be, const uint8_t* proof, size_t len, Verdict& v) : st_(st), be_(be), v_(v), A(st, proof, len, v) {}

    // deferred-weight inputs of the matrix evaluation, valid once the walk got that far (the recorder reads them)
    std::vector<fe> alpha, point;
    bool reached_matrix_evaluation = false;

    bool run() {
        const unsigned m_0 = st_.m_0;
        Commitment wcom, bcom;
        if (!parse_commitment(st_.w, wcom)) return false;
        std::vector<fe> r(m_0);
        if (!A.challenge_scalars(m_0, r.data())) return false;
        if (!parse_commitment(st_.b, bcom)) return false;
        fe sum_g, rho;
        if (!A.next_scalars(1, &sum_g) || !A.challenge_scalars(1, &rho)) return false;
        fe saved = pk::h_mul(rho, sum_g);
        alpha.resize(m_0);
        for (unsigned i = 0; i < m_0; i++) {  // whir_r1cs.rs:131-144
            fe hhat[4], a_i;
            if (!A.next_scalars(4, hhat) || !A.challenge_scalars(1, &a_i)) return false;
            const fe at01 = pk::h_add(pk::h_add(pk::h_add(hhat[0], hhat[0]), hhat[1]), pk::h_add(hhat[2], hhat[3]));
            if (!relation(pk::fe_eq(saved, at01), PKV_CHECK_ZK_SUMCHECK, "Sumcheck equality assertion failed")) return false;
            saved = pk::eval_cubic(hhat, a_i);
            alpha[i] = a_i;
        }
        fe bsums[2];
        if (!A.next_scalars(2, bsums)) return false;
        std::vector<fe> brev, wrev;
        std::vector<HintFe> bdef, wdef;
        if (!whir_verify(bcom, st_.b, {pk::h_add(bsums[0], pk::h_mul(bcom.beta, bsums[1]))}, brev, bdef)) return false;
        {  // the blinding weight is public: expand_powers(alpha), zero-extended; its MLE at the folding point
            std::vector<fe> table((size_t)1 << st_.b.n_vars, f_zero());
            for (unsigned i = 0; i < m_0; i++) {
                table[4 * i] = f_one();
                table[4 * i + 1] = alpha[i];
                table[4 * i + 2] = pk::h_mul(alpha[i], alpha[i]);
                table[4 * i + 3] = pk::h_mul(table[4 * i + 2], alpha[i]);
            }
            if (!relation(bdef[0].canonical && pk::fe_eq(bdef[0].mont, mle_eval_table(table, brev)), PKV_CHECK_BLINDING_WEIGHT,
                          "deferred evaluation of the blinding weight is wrong"))
                return false;
        }
        const fe f_at_alpha = pk::h_sub(saved, pk::h_mul(rho, bsums[0]));
        std::vector<HintFe> f_sums, g_sums;
        {  // claimed_evaluations
            const uint8_t* p;
            size_t n;
            if (!A.hint(p, n)) return false;
            Rd rd{p, n};
            if (!pk::parse_vec(rd, f_sums) || !pk::parse_vec(rd, g_sums) || !rd.end() || f_sums.size() != 3 || g_sums.size() != 3)
                return A.fail(PKV_CHECK_HINT_FORMAT, "bad claimed_evaluations hint");
        }
        std::vector<fe> claims(3);
        for (int k = 0; k < 3; k++) claims[k] = pk::h_add(f_sums[k].mont, pk::h_mul(wcom.beta, g_sums[k].mont));
        if (!whir_verify(wcom, st_.w, claims, wrev, wdef)) return false;
        if (!A.done()) return A.fail(PKV_CHECK_TRAILING_BYTES, "trailing bytes after the proof");
        // the Spartan relation (whir_r1cs.rs:78-86)
        const fe abc = pk::h_sub(pk::h_mul(f_sums[0].mont, f_sums[1].mont), f_sums[2].mont);
        if (!relation(pk::fe_eq(f_at_alpha, pk::h_mul(abc, eq_poly(r.data(), alpha.data(), m_0))), PKV_CHECK_SPARTAN,
                      "last sumcheck value does not match"))
            return false;
        if (st_.has_r1cs) {  // matrix_evaluation.go: deferred_k == eq(alpha)^T M_k eq(wrev[1:]) (1 - wrev[0])
            if (((size_t)1 << (st_.m - 1)) < st_.nw) return A.fail(PKV_CHECK_WITNESS_FIT, "witness does not fit");
            point.assign(wrev.begin() + 1, wrev.end());
            reached_matrix_evaluation = true;
            fe evals[3];
            be_.matrix_evaluations(st_, alpha, point, evals);
            const fe one_minus = pk::h_sub(f_one(), wrev[0]);
            for (int k = 0; k < 3; k++)
                if (!relation(wdef[k].canonical && pk::fe_eq(wdef[k].mont, pk::h_mul(evals[k], one_minus)), PKV_CHECK_MATRIX_EVAL,
                              "deferred evaluation of weight " + std::to_string(k) + " does not match the R1CS matrix"))
                    return false;
        }
        v_.offset = A.pos();
        return true;
    }

  protected:  // a walk of another statement around the same WHIR proof (whir_pcs/) derives from this one
    struct Commitment {
        fe root;  // canonical
        std::vector<fe> ood_pts;
        std::vector<std::vector<fe>> ood_ans;
        fe beta;
    };
    const Statement& st_;
    Backend& be_;
    Verdict& v_;
    Arthur A;

    // a relation between scalars: judged unless placeholders have entered the walk
    bool relation(bool holds, int check, const std::string& msg) {
        if (be_.tainted || holds) return true;
        return A.fail(check, msg);
    }
    bool parse_commitment(const pk_whir_config& cfg, Commitment& c) {  // mtUtilities.go:51-76
        fe root_m;
        if (!A.next_scalars(1, &root_m, &c.root)) return false;
        c.ood_pts.resize(cfg.commitment_ood_samples);
        if (!A.challenge_scalars(cfg.commitment_ood_samples, c.ood_pts.data())) return false;
        c.ood_ans.assign(cfg.batch_size, std::vector<fe>(cfg.commitment_ood_samples));
        for (unsigned b = 0; b < cfg.batch_size; b++)
            if (!A.next_scalars(cfg.commitment_ood_samples, c.ood_ans[b].data())) return false;
        c.beta = f_one();
        if (cfg.batch_size > 1 && !A.challenge_scalars(1, &c.beta)) return false;
        return true;
    }
    bool check_pow(double bits) {  // utilities.go:84-101; pow.rs:24-26
        if (!(bits > 0)) return true;
        uint8_t ch[pk::POW_CHALLENGE_BYTES], nb[pk::POW_NONCE_BYTES];
        if (!A.challenge_bytes(sizeof ch, ch) || !A.next_bytes(sizeof nb, nb)) return false;
        const uint64_t nonce = pk::nonce_from_bytes(nb);
        fe n = f_zero();
        n.v[0] = (uint32_t)nonce;
        n.v[1] = (uint32_t)(nonce >> 32);
        const fe h = h_compress(2, load_raw(ch), n);
        uint64_t thr[4];
        pk::pow_threshold(bits, thr);
        fe t;
        memcpy(t.v, thr, 32);
        if (!pk::fe_lt(h, t)) return A.fail(PKV_CHECK_POW, "proof of work below difficulty");
        return true;
    }
    bool stir_indexes(uint64_t domain, unsigned fold, unsigned nq, std::vector<uint64_t>& out) {  // whir_utilities.go:48-77
        std::vector<uint8_t> raw(pk::stir_query_bytes(domain, fold) * nq);
        if (!A.challenge_bytes(raw.size(), raw.data())) return false;
        out = pk::stir_indexes(raw.data(), domain, fold, nq);
        return true;
    }
    // stir_answers (Vec<Vec<F>>) and merkle_proof (MultiPath, prefix-compressed) of the tree with 2^(depth+1) leaves
    bool read_openings(unsigned width, unsigned depth, RoundOpenings& ro) {
        const uint8_t* p;
        size_t n;
        if (!A.hint(p, n)) return false;
        ro.width = width;
        ro.depth = depth;
        {
            Rd rd{p, n};
            uint64_t k;
            if (!rd.count(k, 8 + 32 * (size_t)width)) return A.fail(PKV_CHECK_HINT_FORMAT, "stir_answers: the leaf count exceeds the hint");
            ro.leaves.resize((size_t)k);
            for (auto& leaf : ro.leaves) {
                uint64_t w;
                if (!rd.u64(w) || w != width || !rd.skip(32 * (size_t)width, leaf))
                    return A.fail(PKV_CHECK_HINT_FORMAT, "stir_answers: a leaf is not " + std::to_string(width) + " elements wide");
            }
            if (!rd.end()) return A.fail(PKV_CHECK_HINT_FORMAT, "trailing bytes in stir_answers");
        }
        if (!A.hint(p, n)) return false;
        Rd rd{p, n};
        uint64_t ns, np, nsuf, ni;
        if (!rd.count(ns, 32)) return A.fail(PKV_CHECK_HINT_FORMAT, "merkle_proof: the sibling count exceeds the hint");
        ro.siblings.resize((size_t)ns);
        for (auto& s : ro.siblings) rd.skip(32, s);
        if (!rd.count(np, 8)) return A.fail(PKV_CHECK_HINT_FORMAT, "merkle_proof: the prefix count exceeds the hint");
        std::vector<uint64_t> pre((size_t)np);
        for (auto& x : pre) rd.u64(x);
        if (!rd.count(nsuf, 8)) return A.fail(PKV_CHECK_HINT_FORMAT, "merkle_proof: the suffix count exceeds the hint");
        std::vector<std::pair<const uint8_t*, uint64_t>> suf((size_t)nsuf);
        for (auto& s : suf) {
            if (!rd.count(s.second, 32)) return A.fail(PKV_CHECK_HINT_FORMAT, "merkle_proof: a path suffix exceeds the hint");
            rd.skip(32 * (size_t)s.second, s.first);
        }
        if (!rd.count(ni, 8)) return A.fail(PKV_CHECK_HINT_FORMAT, "merkle_proof: the index count exceeds the hint");
        ro.indices.resize((size_t)ni);
        for (auto& x : ro.indices) rd.u64(x);
        if (!rd.end()) return A.fail(PKV_CHECK_HINT_FORMAT, "trailing bytes in merkle_proof");
        ro.k = ro.leaves.size();
        if (ns != ro.k || np != ro.k || nsuf != ro.k || ni != ro.k) return A.fail(PKV_CHECK_OPENING_COUNT, "opening count mismatch");
        // a path is the previous path's first pre[o] digests (no more than it has), then the suffix (utilities.go:71-82); `depth` in all
        ro.paths.assign(ro.k * (size_t)depth, nullptr);
        for (size_t o = 0; o < ro.k; o++) {
            const uint64_t shared = std::min<uint64_t>(pre[o], o ? depth : 0);
            if (shared + suf[o].second != depth)
                return A.fail(PKV_CHECK_HINT_FORMAT, "merkle_proof: an authentication path is not " + std::to_string(depth) + " digests long");
            for (unsigned d = 0; d < depth; d++)
                ro.paths[o * depth + d] = d < shared ? ro.paths[(o - 1) * depth + d] : suf[o].first + 32 * (size_t)(d - shared);
        }
        return true;
    }
    // parse + Merkle + index-set check + fold values of one round's openings
    bool open_round(const pk_whir_config& cfg, bool first, uint64_t domain, const fe& root, const fe& beta, const std::vector<fe>& rs,
                    const std::vector<uint64_t>& expected, const char* what, RoundOpenings& ro, std::vector<fe>& folds) {
        const unsigned k = cfg.folding_factor, fw = 1u << k;
        unsigned log_rows = 0;
        while (((domain >> k) >> (log_rows + 1)) != 0) log_rows++;
        if (!read_openings(first ? cfg.batch_size * fw : fw, log_rows - 1, ro)) return false;
        ro.root = root;
        ro.weights.resize(ro.width);
        fe bp = f_one();
        for (unsigned b = 0; b < ro.width / fw; b++) {  // rlcBatchedLeaves (mtUtilities.go:98-114) folded into computeFold's weights
            for (unsigned j = 0; j < fw; j++) {
                fe w = bp;
                for (unsigned t = 0; t < k; t++)
                    if ((j >> t) & 1) w = pk::h_mul(w, rs[t]);
                ro.weights[b * fw + j] = w;
            }
            bp = pk::h_mul(bp, beta);
        }
        std::vector<uint8_t> reached;
        be_.openings(st_.hash_version, ro, reached, folds);
        for (size_t q = 0; q < ro.k; q++)
            if (!reached[q]) return A.fail(PKV_CHECK_MERKLE, "Merkle opening does not reach the root");
        if (ro.indices != expected) return A.fail(PKV_CHECK_STIR_INDICES, std::string(what) + " are not the STIR challenge set");
        return true;
    }
    bool sumcheck(unsigned rounds, fe& last, std::vector<fe>& rs) {
        rs.clear();
        for (unsigned i = 0; i < rounds; i++) {
            fe ev[3], r;
            if (!A.next_scalars(3, ev) || !A.challenge_scalars(1, &r)) return false;
            if (!relation(pk::fe_eq(pk::h_add(ev[0], ev[1]), last), PKV_CHECK_WHIR_SUMCHECK, "WHIR sumcheck: h(0)+h(1) != claim")) return false;
            last = quad_from_evals(ev, r);
            rs.push_back(r);
        }
        return true;
    }
    // RunZKWhir (whir.go:51-220): claimed_sums = per linear statement the batched claim f + beta g
    bool whir_verify(const Commitment& com, const pk_whir_config& cfg, const std::vector<fe>& claimed_sums, std::vector<fe>& rev,
                     std::vector<HintFe>& deferred) {
        const unsigned n = cfg.n_vars, k = cfg.folding_factor;
        const size_t n_ood = com.ood_pts.size();
        std::vector<fe> firsts(n_ood + claimed_sums.size());
        for (size_t j = 0; j < n_ood; j++) {  // OOD answers combined over the batch (mt.go:71-100)
            fe acc = f_zero(), bp = f_one();
            for (unsigned b = 0; b < cfg.batch_size; b++) {
                acc = pk::h_add(acc, pk::h_mul(com.ood_ans[b][j], bp));
                bp = pk::h_mul(bp, com.beta);
            }
            firsts[j] = acc;
        }
        for (size_t i = 0; i < claimed_sums.size(); i++) firsts[n_ood + i] = claimed_sums[i];
        fe g0;
        if (!A.challenge_scalars(1, &g0)) return false;
        const std::vector<fe> comb0 = expand_randomness(g0, firsts.size());
        fe last = f_zero();
        for (size_t i = 0; i < firsts.size(); i++) last = pk::h_add(last, pk::h_mul(comb0[i], firsts[i]));
        std::vector<fe> rs, total;
        if (!sumcheck(k, last, rs)) return false;
        total = rs;
        fe exp_gen = pk::folded_domain_generator(n + cfg.starting_log_inv_rate, k);
        uint64_t domain = (uint64_t)1 << (n + cfg.starting_log_inv_rate);
        fe prev_root = com.root;
        bool first = true;
        struct RoundData {
            std::vector<fe> pts, comb;
        };
        std::vector<RoundData> rounds_data;
        std::vector<uint64_t> expected;
        std::vector<fe> folds;
        for (unsigned r = 0; r < cfg.n_rounds; r++) {
            fe root_m, root;
            if (!A.next_scalars(1, &root_m, &root)) return false;
            std::vector<fe> ood_pts(cfg.ood_samples[r]), ood_ans(cfg.ood_samples[r]);
            if (!A.challenge_scalars(ood_pts.size(), ood_pts.data()) || !A.next_scalars(ood_ans.size(), ood_ans.data())) return false;
            if (!check_pow(cfg.pow_bits[r])) return false;
            if (!stir_indexes(domain, k, cfg.num_queries[r], expected)) return false;
            RoundOpenings ro;
            if (!open_round(cfg, first, domain, prev_root, com.beta, rs, expected, "opened leaves", ro, folds)) return false;
            first = false;
            RoundData rd;
            rd.pts = ood_pts;
            for (uint64_t i : ro.indices) rd.pts.push_back(pk::h_pow(exp_gen, i));
            fe gr;
            if (!A.challenge_scalars(1, &gr)) return false;
            rd.comb = expand_randomness(gr, ood_pts.size() + folds.size());
            for (size_t i = 0; i < ood_ans.size(); i++) last = pk::h_add(last, pk::h_mul(rd.comb[i], ood_ans[i]));
            for (size_t i = 0; i < folds.size(); i++) last = pk::h_add(last, pk::h_mul(rd.comb[ood_ans.size() + i], folds[i]));
            rounds_data.push_back(std::move(rd));
            if (!sumcheck(k, last, rs)) return false;
            total.insert(total.end(), rs.begin(), rs.end());
            prev_root = root;
            domain /= 2;
            exp_gen = pk::h_mul(exp_gen, exp_gen);
        }
        const unsigned final_vars = n - k * (cfg.n_rounds + 1);
        std::vector<fe> final_coeffs((size_t)1 << final_vars);
        if (!A.next_scalars(final_coeffs.size(), final_coeffs.data())) return false;
        if (!check_pow(cfg.final_pow_bits)) return false;
        if (!stir_indexes(domain, k, cfg.final_queries, expected)) return false;
        {
            RoundOpenings ro;
            if (!open_round(cfg, first, domain, prev_root, com.beta, rs, expected, "final opened leaves", ro, folds)) return false;
            for (size_t q = 0; q < ro.k; q++)
                if (!relation(pk::fe_eq(folds[q], eval_univariate(final_coeffs, pk::h_pow(exp_gen, ro.indices[q]))), PKV_CHECK_FINAL_POLY,
                              "final polynomial mismatch at a STIR point"))
                    return false;
        }
        std::vector<fe> rs_final;
        if (!sumcheck(final_vars, last, rs_final)) return false;
        total.insert(total.end(), rs_final.begin(), rs_final.end());
        if (!check_pow(cfg.final_folding_pow_bits)) return false;  // whir.go:196-201
        deferred.clear();
        if (!claimed_sums.empty()) {
            const uint8_t* p;
            size_t hn;
            if (!A.hint(p, hn)) return false;
            Rd rd{p, hn};
            if (!pk::parse_vec(rd, deferred) || !rd.end() || deferred.size() != claimed_sums.size())
                return A.fail(PKV_CHECK_HINT_FORMAT, "bad deferred_weight_evaluations hint");
        }
        rev.assign(total.rbegin(), total.rend());
        // computeWPoly (whir_utilities.go:127-157)
        fe value = f_zero();
        std::vector<fe> pt(n);
        for (size_t j = 0; j < n_ood; j++) {
            pk::expand_from_univariate(com.ood_pts[j], n, pt.data());
            value = pk::h_add(value, pk::h_mul(comb0[j], eq_poly(pt.data(), rev.data(), n)));
        }
        for (size_t i = 0; i < deferred.size(); i++) value = pk::h_add(value, pk::h_mul(comb0[n_ood + i], deferred[i].mont));
        unsigned nv = n;
        for (const RoundData& rd : rounds_data) {
            nv -= k;
            for (size_t i = 0; i < rd.pts.size(); i++) {
                pk::expand_from_univariate(rd.pts[i], nv, pt.data());
                value = pk::h_add(value, pk::h_mul(rd.comb[i], eq_poly(pt.data(), rev.data(), nv)));
            }
        }
        return relation(pk::fe_eq(last, pk::h_mul(value, multivar_poly(final_coeffs, rs_final))), PKV_CHECK_WHIR_FINAL, "WHIR final check failed");
    }
};

inline void verify_host(const Statement& st, const uint8_t* proof, size_t len, pkv_result* out) {
    Verdict v;
    HostBackend be;
    Walk w(st, be, proof, len, v);
    w.run();
    to_result(v, out);
}

}  // namespace pkv
