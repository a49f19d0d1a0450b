// verify_host.cpp -- the host half of libprovekit_whir.so: the IO pattern, the arena size and pkw_verify.  No device code and no
// HIP call.  The WHIR proof inside an opening is walked by verify/core.hpp's Walk::whir_verify, unchanged; what is new here is the
// statement around it: the points and evaluations on the transcript, and the deferred weight evaluations, which for the weights
// eq(point_i, .) have the closed form eq(point_i, folding point).  A linear statement (pkw_verify_linear) adds tags, sums and dense
// weight tables, whose deferred evaluations are their multilinear extensions at the folding point: 2^n_vars products per table the
// caller hands over, the caller's own business for the others.  Sparse weights (pkw_verify_sparse) are index/value lists: their
// extensions at the folding point cost one product per 8 index bits and entry (sparse.hpp's chunked eq tables), so the verifier
// always judges them itself.
#include "pcs.hpp"
#include "sparse.hpp"

namespace pkw {

thread_local std::string g_error;

namespace {

const char* const kNames[PKW_CHECK_COUNT - PKV_CHECK_COUNT] = {"POINTS", "ROOT", "DEFERRED"};
const char* const kWalkNames[PKV_CHECK_COUNT] = {
    "NONE",          "TRANSCRIPT_SHORT", "NON_CANONICAL", "IO_PATTERN", "HINT_FORMAT", "OPENING_COUNT",   "MERKLE",         "ZK_SUMCHECK", "WHIR_SUMCHECK",
    "POW",           "STIR_INDICES",     "FINAL_POLY",    "WHIR_FINAL", "BLINDING_WEIGHT", "TRAILING_BYTES", "SPARTAN", "WITNESS_FIT", "MATRIX_EVAL"};

class PcsWalk : public pkv::Walk {
  public:
    PcsWalk(const pkv::Statement& st, pkv::Backend& be, const uint8_t* proof, size_t len, pkv::Verdict& v, const pk_whir_config& cfg, const Statement& s,
            const fe* expected_root)
        : Walk(st, be, proof, len, v), cfg_(cfg), s_(s), expected_root_(expected_root) {}

    std::vector<fe> evals;  // [polynomial][point], Montgomery: what the proof binds, once the walk got past them
    std::vector<fe> sums;   // [polynomial][weight], likewise
    std::vector<fe> fold_point, weight_deferred;  // once the WHIR walk is through: the folding point, the l deferred values of the weights
    unsigned unchecked = 0;                       // weights without a table: their deferred values are the caller's to check

    bool run_opening() {
        const unsigned n = cfg_.n_vars, batch = cfg_.batch_size, q = s_.q, l = s_.l;
        const fe *points = reinterpret_cast<const fe*>(s_.points), *tags = reinterpret_cast<const fe*>(s_.tags);
        const SparseWeights* sparse = s_.sparse;
        Commitment com;
        if (!parse_commitment(cfg_, com)) return false;
        if (expected_root_ && !pk::fe_eq(com.root, *expected_root_)) return A.fail(PKW_CHECK_ROOT, "the proof's root is not the expected commitment");
        std::vector<fe> pts((size_t)q * n);
        if (!pts.empty() && !A.next_scalars(pts.size(), pts.data())) return false;
        for (size_t j = 0; j < pts.size(); j++)
            if (!pk::fe_eq(pts[j], points[j]))
                return A.fail(PKW_CHECK_POINTS, "point " + std::to_string(j / n) + " of the proof is not the caller's (coordinate " + std::to_string(j % n) + ")");
        std::vector<fe> tg(l);
        if (l && !A.next_scalars(l, tg.data())) return false;
        for (unsigned i = 0; i < l; i++)
            if (!pk::fe_eq(tg[i], tags[i])) return A.fail(PKW_CHECK_POINTS, "tag " + std::to_string(i) + " of the proof is not the caller's");
        std::vector<fe> ev((size_t)batch * q), sm((size_t)batch * l);
        if (!ev.empty() && !A.next_scalars(ev.size(), ev.data())) return false;
        evals = ev;
        if (!sm.empty() && !A.next_scalars(sm.size(), sm.data())) return false;
        sums = sm;
        std::vector<fe> claims(q + l);
        for (unsigned i = 0; i < q + l; i++) {  // the statement of the beta-combined polynomial: evaluations, then sums
            fe acc = pkv::f_zero(), bp = pkv::f_one();
            for (unsigned b = 0; b < batch; b++) {
                acc = pk::h_add(acc, pk::h_mul(bp, i < q ? ev[(size_t)b * q + i] : sm[(size_t)b * l + (i - q)]));
                bp = pk::h_mul(bp, com.beta);
            }
            claims[i] = acc;
        }
        std::vector<fe> rev;
        std::vector<pk::HintFe> deferred;
        if (!whir_verify(com, cfg_, claims, rev, deferred)) return false;
        fold_point = rev;
        for (unsigned i = 0; i < l; i++) weight_deferred.push_back(deferred[q + i].mont);
        if (!A.done()) return A.fail(PKV_CHECK_TRAILING_BYTES, "trailing bytes after the proof");
        for (unsigned i = 0; i < q; i++)  // the MLE of eq(point_i, .) at the folding point
            if (!relation(deferred[i].canonical && pk::fe_eq(deferred[i].mont, pkv::eq_poly(points + (size_t)i * n, rev.data(), n)), PKW_CHECK_DEFERRED,
                          "deferred evaluation of weight " + std::to_string(i) + " is not eq(point, folding point)"))
                return false;
        const SparseEqTables eq(rev.data(), sparse ? n : 0);  // sparse weights: the chunks' eq tables at the folding point, once for all l
        for (unsigned i = 0; i < l; i++) {  // the MLE of a weight at the folding point: of the entries, or of a dense table the caller gave
            const pk::HintFe& d = deferred[q + i];
            if (!relation(d.canonical, PKW_CHECK_DEFERRED, "deferred evaluation of weight " + std::to_string(i) + " is not canonical")) return false;
            if (sparse) {
                const size_t at = sparse->begin(i);
                if (!relation(pk::fe_eq(d.mont, eq.weight_at(sparse->index + at, sparse->value + 4 * at, sparse->nnz(i))), PKW_CHECK_DEFERRED,
                              "deferred evaluation of weight " + std::to_string(i) + " is not the extension of the caller's entries at the folding point"))
                    return false;
                continue;
            }
            if (!s_.dense || !s_.dense[i]) {
                unchecked++;
                continue;
            }
            if (!relation(pk::fe_eq(d.mont, table_at(s_.dense[i], rev)), PKW_CHECK_DEFERRED,
                          "deferred evaluation of weight " + std::to_string(i) + " is not the extension of the caller's table at the folding point"))
                return false;
        }
        v_.offset = A.pos();
        return true;
    }

  private:
    const pk_whir_config& cfg_;
    const Statement& s_;
    const fe* expected_root_;

    // the multilinear extension of a dense table (2^n Montgomery elements, any 256-bit values) at `point`, variable 0 <-> the most
    // significant index bit: the first fold reads the caller's table, the rest work on the half-size copy
    static fe table_at(const uint64_t* table, const std::vector<fe>& point) {
        auto at = [&](size_t i) { return pk::fe_reduce_any(pk::h_load(table + 4 * i)); };
        if (point.empty()) return at(0);
        size_t len = (size_t)1 << (point.size() - 1);
        std::vector<fe> v(len);
        for (size_t i = 0; i < len; i++) {
            const fe lo = at(i);
            v[i] = pk::h_add(lo, pk::h_mul(point[0], pk::h_sub(at(i + len), lo)));
        }
        for (size_t j = 1; j < point.size(); j++) {
            len /= 2;
            for (size_t i = 0; i < len; i++) v[i] = pk::h_add(v[i], pk::h_mul(point[j], pk::h_sub(v[i + len], v[i])));
        }
        return v[0];
    }
};

// what pkw_verify, pkw_verify_linear and pkw_verify_sparse share once their counts and pointers are checked; s.l = 0: pkw_verify
int verify_checked(const pk_whir_config* cfg, const uint8_t* io_pattern, size_t io_pattern_len, int hash_version, const uint8_t* expected_root,
                   const Statement& s, const uint8_t* proof, size_t len, const VerifyOutputs& out, pkv_result* result) {
    std::string why;
    if (hash_version != 1 && hash_version != 2) return refuse("hash version must be 1 or 2");
    try {
        pkv::Statement st;
        st.w = st.b = *cfg;
        st.hash_version = hash_version;
        if (io_pattern && io_pattern_len)
            st.pattern.assign(reinterpret_cast<const char*>(io_pattern), io_pattern_len);
        else
            st.pattern = pkw::io_pattern(*cfg, s.q, s.l, s.hiding);
        if (!pk::io_pattern_parse(st.pattern, st.ops, why)) {
            g_error = why;
            return PK_ERR_IO_PATTERN;
        }
        pkv::Verdict verdict;
        if (io_pattern && io_pattern_len) {
            // a caller's pattern may spell the labels otherwise; its operations are this config's.  Held against them here: under
            // another config's pattern every challenge differs, and the walk would stop at its first relation, long before the
            // operation that differs
            std::vector<pk::IoOp> own;
            if (!pk::io_pattern_parse(pkw::io_pattern(*cfg, s.q, s.l), own, why)) return refuse("internal: " + why);
            size_t i = 0;
            while (i < own.size() && i < st.ops.size() && own[i].kind == st.ops[i].kind && own[i].count == st.ops[i].count) i++;
            if (i < own.size() || i < st.ops.size()) {
                verdict.failed = true;
                verdict.check = PKV_CHECK_IO_PATTERN;
                verdict.message = "the IO pattern does not declare this config's operations (operation #" + std::to_string(i + 1) + ")";
                pkv::to_result(verdict, result);
                if (out.unchecked) *out.unchecked = 0;
                return PK_OK;
            }
        }
        static const uint8_t none = 0;
        pk::fe root;
        if (expected_root) root = pk::load_raw(expected_root);
        pkv::HostBackend be;
        PcsWalk walk(st, be, len ? proof : &none, len, verdict, *cfg, s, expected_root ? &root : nullptr);
        walk.run_opening();
        pkv::to_result(verdict, result);
        auto give = [](uint64_t* to, const std::vector<fe>& v) {
            if (to && !v.empty()) memcpy(to, v.data(), 32 * v.size());
        };
        give(out.evals, walk.evals);
        give(out.sums, walk.sums);
        give(out.fold_point, walk.fold_point);
        give(out.deferred, walk.weight_deferred);
        if (out.unchecked) *out.unchecked = walk.unchecked;
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

// the pattern of a statement with q points and l weights into (buf, cap, *len): both pattern entry points, their counts checked
int write_pattern(const pk_whir_config& cfg, unsigned q, unsigned l, uint8_t* buf, size_t cap, size_t* len, bool hiding = false) {
    try {
        const std::string d = io_pattern(cfg, q, l, hiding);
        *len = d.size();
        if (buf && cap >= d.size()) memcpy(buf, d.data(), d.size());
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

}  // namespace
}  // namespace pkw

extern "C" {

int pkw_abi_version(void) { return 1; }

const char* pkw_check_name(int check) {
    if (check >= 0 && check < PKV_CHECK_COUNT) return pkw::kWalkNames[check];
    if (check >= PKV_CHECK_COUNT && check < PKW_CHECK_COUNT) return pkw::kNames[check - PKV_CHECK_COUNT];
    return "UNKNOWN";
}

const char* pkw_create_error(void) { return pkw::g_error.c_str(); }

#ifndef PKW_HOST_ONLY  // the arena's plan asks the evaluation kernel's launch code, which the sanitizer build does not have
int pkw_scheme_arena_bytes(const pk_whir_config* cfg, size_t* bytes) {
    std::string why;
    if (!bytes) return pkw::refuse("null pointer");
    if (!pkw::config_ok(cfg, why)) return pkw::refuse(why);
    *bytes = 32 * pkw::plan(*cfg).total;
    return PK_OK;
}
#endif

int pkw_io_pattern(const pk_whir_config* cfg, unsigned q, uint8_t* buf, size_t cap, size_t* len) {
    std::string why;
    if (!len) return pkw::refuse("null pointer");
    if (!pkw::config_ok(cfg, why)) return pkw::refuse(why);
    if (q < 1 || q > PKW_MAX_POINTS) return pkw::refuse("the number of points must be 1..64");
    return pkw::write_pattern(*cfg, q, 0, buf, cap, len);
}

int pkw_verify(const pk_whir_config* cfg, const uint8_t* io_pattern, size_t io_pattern_len, int hash_version, const uint8_t* expected_root,
               const uint64_t* points, unsigned q, const uint8_t* proof, size_t len, uint64_t* evals_out, pkv_result* result) {
    std::string why;
    if (!result || !points || (len && !proof)) return pkw::refuse("null pointer");
    if (!pkw::config_ok(cfg, why)) return pkw::refuse(why);
    if (q < 1 || q > PKW_MAX_POINTS) return pkw::refuse("the number of points must be 1..64");
    return pkw::verify_checked(cfg, io_pattern, io_pattern_len, hash_version, expected_root, pkw::Statement{points, q}, proof, len,
                               pkw::VerifyOutputs{evals_out}, result);
}

// provekit_whir_linear.h
int pkw_io_pattern_linear(const pk_whir_config* cfg, unsigned q, unsigned l, uint8_t* buf, size_t cap, size_t* len) {
    std::string why;
    if (!len) return pkw::refuse("null pointer");
    if (!pkw::config_ok(cfg, why) || !pkw::linear_counts_ok(q, l, why)) return pkw::refuse(why);
    return pkw::write_pattern(*cfg, q, l, buf, cap, len);
}

int pkw_verify_linear(const pk_whir_config* cfg, const uint8_t* io_pattern, size_t io_pattern_len, int hash_version, const uint8_t* expected_root,
                      const uint64_t* points, unsigned q, const uint64_t* tags, const uint64_t* const* weights, unsigned l, const uint8_t* proof, size_t len,
                      uint64_t* evals_out, uint64_t* sums_out, uint64_t* fold_point_out, uint64_t* deferred_out, unsigned* unchecked_out,
                      pkv_result* result) {
    std::string why;
    if (!pkw::config_ok(cfg, why) || !pkw::linear_counts_ok(q, l, why)) return pkw::refuse(why);
    if (!result || (q && !points) || !tags || (len && !proof)) return pkw::refuse("null pointer");
    return pkw::verify_checked(cfg, io_pattern, io_pattern_len, hash_version, expected_root, pkw::Statement{points, q, tags, l, weights}, proof, len,
                               pkw::VerifyOutputs{evals_out, sums_out, fold_point_out, deferred_out, unchecked_out}, result);
}

// provekit_whir_sparse.h: pkw_verify_linear's walk over lists the host checks first, entry by entry
int pkw_verify_sparse(const pk_whir_config* cfg, const uint8_t* io_pattern, size_t io_pattern_len, int hash_version, const uint8_t* expected_root,
                      const uint64_t* points, unsigned q, const uint64_t* tags, const uint64_t* offsets, const uint32_t* index, const uint64_t* value, unsigned l,
                      const uint8_t* proof, size_t len, uint64_t* evals_out, uint64_t* sums_out, uint64_t* fold_point_out, uint64_t* deferred_out,
                      pkv_result* result) {
    std::string why;
    if (!pkw::config_ok(cfg, why) || !pkw::linear_counts_ok(q, l, why)) return pkw::refuse(why);
    if (!result || (q && !points) || !tags || !offsets || (len && !proof)) return pkw::refuse("null pointer");
    const unsigned n = cfg->n_vars;
    if (!pkw::sparse_offsets_ok(offsets, l, n, why)) return pkw::refuse(why);
    if (offsets[l] && (!index || !value)) return pkw::refuse("null index or value list");
    const pkw::SparseWeights w{offsets, index, value, l};
    for (unsigned i = 0; i < l; i++)
        for (size_t k = w.begin(i); k < w.begin(i + 1); k++) {
            const bool first = k == w.begin(i);
            if (((uint64_t)index[k] >> n) != 0 || (!first && index[k - 1] >= index[k])) return pkw::refuse(pkw::sparse_index_reason(w, k, index[k], first ? 0 : index[k - 1], n));
            if (!pkw::below_p(pk::h_load(value + 4 * k)))
                return pkw::refuse("weight " + std::to_string(i) + ", entry " + std::to_string(k - w.begin(i)) + ": the value is not below p");
        }
    return pkw::verify_checked(cfg, io_pattern, io_pattern_len, hash_version, expected_root, pkw::Statement{points, q, tags, l, nullptr, &w}, proof, len,
                               pkw::VerifyOutputs{evals_out, sums_out, fold_point_out, deferred_out}, result);
}

// provekit_whir_hiding.h
int pkw_io_pattern_hiding(const pk_whir_config* cfg, unsigned q, uint8_t* buf, size_t cap, size_t* len) {
    std::string why;
    if (!len) return pkw::refuse("null pointer");
    if (!pkw::config_ok(cfg, why) || !pkw::hiding_config_ok(*cfg, why)) return pkw::refuse(why);
    if (q < 1 || q > PKW_MAX_POINTS) return pkw::refuse("the number of points must be 1..64");
    return pkw::write_pattern(*cfg, q, 0, buf, cap, len, /*hiding=*/true);
}

// pkw_verify over the extended statement: every point prefixed by 0, the hiding pattern, the first B rows of evaluations handed back
int pkw_verify_hiding(const pk_whir_config* cfg, const uint8_t* io_pattern, size_t io_pattern_len, int hash_version, const uint8_t* expected_root,
                      const uint64_t* points, unsigned q, const uint8_t* proof, size_t len, uint64_t* evals_out, pkv_result* result) {
    std::string why;
    if (!result || !points || (len && !proof)) return pkw::refuse("null pointer");
    if (!pkw::config_ok(cfg, why) || !pkw::hiding_config_ok(*cfg, why)) return pkw::refuse(why);
    if (q < 1 || q > PKW_MAX_POINTS) return pkw::refuse("the number of points must be 1..64");
    try {
        const unsigned nv = cfg->n_vars, batch = cfg->batch_size;
        std::vector<uint64_t> ext(4 * (size_t)q * nv), evals(4 * (size_t)batch * q);
        for (unsigned i = 0; i < q; i++) memcpy(&ext[4 * ((size_t)i * nv + 1)], points + 4 * (size_t)i * (nv - 1), 32 * (size_t)(nv - 1));
        pkw::Statement st{ext.data(), q};
        st.hiding = true;
        const int rc = pkw::verify_checked(cfg, io_pattern, io_pattern_len, hash_version, expected_root, st, proof, len, pkw::VerifyOutputs{evals.data()}, result);
        if (!rc && evals_out) memcpy(evals_out, evals.data(), 32 * (size_t)(batch - 1) * q);
        return rc;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

}  // extern "C"
