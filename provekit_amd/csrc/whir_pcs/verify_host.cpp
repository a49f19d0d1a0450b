// verify_host.cpp -- the host half of libprovekit_whir.so: the IO pattern, the arena size and pkw_verify.  No device code and no
// HIP call.  The WHIR proof inside an opening is walked by verify/core.hpp's Walk::whir_verify, unchanged; what is new here is the
// statement around it: the points and evaluations on the transcript, and the deferred weight evaluations, which for the weights
// eq(point_i, .) have the closed form eq(point_i, folding point).
#include "pcs.hpp"

namespace pkw {

thread_local std::string g_error;

namespace {

const char* const kNames[PKW_CHECK_COUNT - PKV_CHECK_COUNT] = {"POINTS", "ROOT", "DEFERRED"};
const char* const kWalkNames[PKV_CHECK_COUNT] = {
    "NONE",          "TRANSCRIPT_SHORT", "NON_CANONICAL", "IO_PATTERN", "HINT_FORMAT", "OPENING_COUNT",   "MERKLE",         "ZK_SUMCHECK", "WHIR_SUMCHECK",
    "POW",           "STIR_INDICES",     "FINAL_POLY",    "WHIR_FINAL", "BLINDING_WEIGHT", "TRAILING_BYTES", "SPARTAN", "WITNESS_FIT", "MATRIX_EVAL"};

class PcsWalk : public pkv::Walk {
  public:
    PcsWalk(const pkv::Statement& st, pkv::Backend& be, const uint8_t* proof, size_t len, pkv::Verdict& v, const pk_whir_config& cfg, const fe* points,
            unsigned q, const fe* expected_root)
        : Walk(st, be, proof, len, v), cfg_(cfg), points_(points), q_(q), expected_root_(expected_root) {}

    std::vector<fe> evals;  // [polynomial][point], Montgomery: what the proof binds, once the walk got past them

    bool run_opening() {
        const unsigned n = cfg_.n_vars, batch = cfg_.batch_size;
        Commitment com;
        if (!parse_commitment(cfg_, com)) return false;
        if (expected_root_ && !pk::fe_eq(com.root, *expected_root_)) return A.fail(PKW_CHECK_ROOT, "the proof's root is not the expected commitment");
        std::vector<fe> pts((size_t)q_ * n);
        if (!A.next_scalars(pts.size(), pts.data())) return false;
        for (size_t j = 0; j < pts.size(); j++)
            if (!pk::fe_eq(pts[j], points_[j]))
                return A.fail(PKW_CHECK_POINTS, "point " + std::to_string(j / n) + " of the proof is not the caller's (coordinate " + std::to_string(j % n) + ")");
        std::vector<fe> ev((size_t)batch * q_);
        if (!A.next_scalars(ev.size(), ev.data())) return false;
        evals = ev;
        std::vector<fe> claims(q_);
        for (unsigned i = 0; i < q_; i++) {  // the statement of the beta-combined polynomial
            fe acc = pkv::f_zero(), bp = pkv::f_one();
            for (unsigned b = 0; b < batch; b++) {
                acc = pk::h_add(acc, pk::h_mul(bp, ev[(size_t)b * q_ + i]));
                bp = pk::h_mul(bp, com.beta);
            }
            claims[i] = acc;
        }
        std::vector<fe> rev;
        std::vector<pk::HintFe> deferred;
        if (!whir_verify(com, cfg_, claims, rev, deferred)) return false;
        if (!A.done()) return A.fail(PKV_CHECK_TRAILING_BYTES, "trailing bytes after the proof");
        for (unsigned i = 0; i < q_; i++)  // the MLE of eq(point_i, .) at the folding point
            if (!relation(deferred[i].canonical && pk::fe_eq(deferred[i].mont, pkv::eq_poly(points_ + (size_t)i * n, rev.data(), n)), PKW_CHECK_DEFERRED,
                          "deferred evaluation of weight " + std::to_string(i) + " is not eq(point, folding point)"))
                return false;
        v_.offset = A.pos();
        return true;
    }

  private:
    const pk_whir_config& cfg_;
    const fe* points_;
    unsigned q_;
    const fe* expected_root_;
};

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

int pkw_scheme_arena_bytes(const pk_whir_config* cfg, size_t* bytes) {
    std::string why;
    if (!bytes) return pkw::refuse("null pointer");
    if (!pkw::config_ok(cfg, why)) return pkw::refuse(why);
    *bytes = 32 * pkw::plan(*cfg).total;
    return PK_OK;
}

int pkw_io_pattern(const pk_whir_config* cfg, unsigned q, uint8_t* buf, size_t cap, size_t* len) {
    std::string why;
    if (!len) return pkw::refuse("null pointer");
    if (!pkw::config_ok(cfg, why)) return pkw::refuse(why);
    if (q < 1 || q > PKW_MAX_POINTS) return pkw::refuse("the number of points must be 1..64");
    try {
        const std::string d = pkw::io_pattern(*cfg, q);
        *len = d.size();
        if (buf && cap >= d.size()) memcpy(buf, d.data(), d.size());
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

int pkw_verify(const pk_whir_config* cfg, const uint8_t* io_pattern, size_t io_pattern_len, int hash_version, const uint8_t* expected_root,
               const uint64_t* points, unsigned q, const uint8_t* proof, size_t len, uint64_t* evals_out, pkv_result* result) {
    std::string why;
    if (!result || !points || (len && !proof)) return pkw::refuse("null pointer");
    if (!pkw::config_ok(cfg, why)) return pkw::refuse(why);
    if (q < 1 || q > PKW_MAX_POINTS) return pkw::refuse("the number of points must be 1..64");
    if (hash_version != 1 && hash_version != 2) return pkw::refuse("hash version must be 1 or 2");
    try {
        pkv::Statement st;
        st.w = st.b = *cfg;
        st.hash_version = hash_version;
        if (io_pattern && io_pattern_len)
            st.pattern.assign(reinterpret_cast<const char*>(io_pattern), io_pattern_len);
        else
            st.pattern = pkw::io_pattern(*cfg, q);
        if (!pk::io_pattern_parse(st.pattern, st.ops, why)) {
            pkw::g_error = why;
            return PK_ERR_IO_PATTERN;
        }
        static const uint8_t none = 0;
        pk::fe root;
        if (expected_root) root = pk::load_raw(expected_root);
        pkv::Verdict verdict;
        pkv::HostBackend be;
        pkw::PcsWalk walk(st, be, len ? proof : &none, len, verdict, *cfg, reinterpret_cast<const pk::fe*>(points), q, expected_root ? &root : nullptr);
        walk.run_opening();
        pkv::to_result(verdict, result);
        if (evals_out && !walk.evals.empty()) memcpy(evals_out, walk.evals.data(), 32 * walk.evals.size());
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

}  // extern "C"
