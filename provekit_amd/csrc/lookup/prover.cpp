// prover.cpp -- the device half of libprovekit_lookup.so's C ABI: the prover (one arena, the launches of lookup.hip, the prover side
// of the outer transcript, the two pks proofs).  Host code; of other libraries it calls what provekit_hip.h and provekit_sumcheck.h
// declare.
#include "prover.hpp"

using pk::between;
using pk::elements_below_p;
using pk::fail;
using pk::fe;
using pk::host_ms_since;

extern "C" {

int pkl_prover_create(pk_ctx* ctx, const pkl_statement* stmt, pkl_prover** out) {
    if (out) *out = nullptr;
    std::string why;
    if (!ctx || !out) return pkl::refuse("null pointer");
    if (!pkl::statement_ok(stmt, why)) return pkl::refuse(why);
    auto stop = [](int rc, const std::string& reason) { return pkl::g_error = reason, rc; };
    try {
        std::unique_ptr<pkl_prover> p(new pkl_prover());  // its destructor gives back what a return or a throw below leaves behind
        p->ctx = ctx;
        p->st = *stmt;
        p->pattern = pkl::io_pattern(*stmt);
        p->lay = pkl::layout(*stmt);
        if (int rc = pkl::framing(*stmt, p->fr)) return stop(rc, pks_create_error());
        void* base = nullptr;
        if (int rc = pk_malloc(ctx, p->lay.total, &base)) return stop(rc, "pk_malloc of the arena failed");
        p->arena = (char*)base;
        for (hipEvent_t& e : p->ev)
            if (hipEventCreate(&e) != hipSuccess) return stop(PK_ERR_HIP, "hipEventCreate failed");
        if (int rc = pkl::gather_prepare(p->gather)) return stop(rc, "the device refused the staged gather's LDS or did not name its compute units");
        for (int i = 0; i < 2; i++) {
            const pks_statement ps = pkl::side_statement(*stmt, PKL_SIDE_F + i);
            if (int rc = pks_prover_create(ctx, &ps, &p->side[i])) return stop(rc, std::string("pks_prover_create failed: ") + pks_create_error());
        }
        *out = p.release();
        pkl::g_error.clear();
        return PK_OK;
    } catch (...) {
        return pk::out_of_host_memory(pkl::g_error);
    }
}

int pkl_prover_destroy(pkl_prover* p) {
    if (!p) return PK_OK;
    const int rc = p->give_back();
    delete p;
    return rc;
}

const char* pkl_last_error(const pkl_prover* p) { return p ? p->err.c_str() : "null prover"; }

// Host only; here and not next to the verifier because the sumcheck provers' share comes from their launch header.
int pkl_prover_arena_bytes(const pkl_statement* stmt, size_t* bytes) {
    std::string why;
    if (!bytes) return pkl::refuse("null pointer");
    if (!pkl::statement_ok(stmt, why)) return pkl::refuse(why);
    *bytes = pkl::layout(*stmt).total + pkl::sides_arena_bytes(*stmt);
    return PK_OK;
}

int pkl_multiplicities(pkl_prover* p, const uint64_t* d_f, const uint64_t* d_t, const uint32_t* d_idx, uint64_t* d_m_out, uint64_t* first_bad) {
    if (!p) return PK_ERR_BAD_ARG;
    if (first_bad) *first_bad = UINT64_MAX;
    if (!d_f || !d_t || !d_idx || !d_m_out || !first_bad) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    p->state = 0;
    // the caller's work on the context is finished before anything here reads its tables; the library's own launches go to the null stream
    if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
    unsigned long long* const d_bad = p->at<unsigned long long>(p->lay.bad);
    (void)hipEventRecord(p->ev[0], nullptr);
    if (int rc = pkl::count_launch(nullptr, p->st.n, p->st.k, d_f, d_t, d_idx, p->at<uint32_t>(p->lay.counts), d_bad, d_m_out, p->grid))
        return fail(p, rc, "the count kernel's launch failed");
    (void)hipEventRecord(p->ev[1], nullptr);
    unsigned long long bad = 0;
    if (hipMemcpy(&bad, d_bad, 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(p, PK_ERR_HIP, "the validation's result did not arrive");
    p->prof.count_ms = between(p->ev[0], p->ev[1]);
    if (bad != ~0ull) {
        *first_bad = bad;
        return fail(p, PK_ERR_UNSATISFIED, "lookup " + std::to_string(bad) + " fails: idx is out of range or f differs from t[idx]");
    }
    p->d_t = d_t, p->d_idx = d_idx, p->d_m = d_m_out;
    p->state = 1;
    p->err.clear();
    return PK_OK;
}

int pkl_begin(pkl_prover* p, const uint64_t* d_t, const uint32_t* d_idx, const uint64_t* bind, uint64_t* alpha_out, const uint64_t** d_hf_out,
              const uint64_t** d_ht_out) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkl_statement& st = p->st;
    if (!d_t || !d_idx || !d_hf_out || !d_ht_out) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    if (p->state < 1) return fail(p, PK_ERR_BAD_ARG, "pkl_begin needs a successful pkl_multiplicities on this prover first");
    if (d_t != p->d_t || d_idx != p->d_idx) return fail(p, PK_ERR_BAD_ARG, "t and idx are not the ones pkl_multiplicities validated");
    if (st.n_bind && !bind) return fail(p, PK_ERR_BAD_ARG, "the statement binds elements: pass them");
    if (!elements_below_p(bind, st.n_bind)) return fail(p, PK_ERR_BAD_ARG, "a bind element is not below p");
    try {
        p->state = 1;
        if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
        std::unique_ptr<pk::Transcript> tr(new pk::Transcript(p->pattern));
        for (unsigned i = 0; i < st.n_bind; i++) tr->add_scalar(pk::h_load(bind + 4 * i));
        const fe alpha = tr->challenge_scalar();
        uint32_t* const d_flags = p->at<uint32_t>(p->lay.flags);
        (void)hipEventRecord(p->ev[0], nullptr);
        if (int rc = pkl::table_launch(nullptr, st.k, d_t, p->at<uint32_t>(p->lay.counts), (const uint64_t*)alpha.v, p->at<uint64_t>(p->lay.d_t),
                                       p->at<uint64_t>(p->lay.g), p->at<uint64_t>(p->lay.h_t), p->at<uint64_t>(p->lay.partials), p->at<uint64_t>(p->lay.sum),
                                       d_flags, p->grid))
            return fail(p, rc, "the table kernel's launch failed");
        (void)hipEventRecord(p->ev[1], nullptr);
        if (int rc = pkl::gather_launch(nullptr, p->gather, st.n, st.k, d_idx, p->at<uint64_t>(p->lay.g), p->at<uint64_t>(p->lay.d_t), p->at<uint64_t>(p->lay.h_f),
                                        p->at<uint64_t>(p->lay.d_f), d_flags, p->grid))
            return fail(p, rc, "the gather kernel's launch failed");
        (void)hipEventRecord(p->ev[2], nullptr);
        uint32_t flags[2] = {0, 0};
        if (hipMemcpy(flags, d_flags, 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(p, PK_ERR_HIP, "the helper kernels' flags did not arrive");
        p->prof.table_ms = between(p->ev[0], p->ev[1]);
        p->prof.gather_ms = between(p->ev[1], p->ev[2]);
        if (flags[0]) return fail(p, PK_ERR_UNSATISFIED, "alpha is an entry of t (a zero denominator): bind something else to draw another alpha");
        if (flags[1]) return fail(p, PK_ERR_BAD_ARG, "idx changed since pkl_multiplicities validated it: an index is out of range");
        if (!tr->violation().empty()) return fail(p, PK_ERR_IO_PATTERN, "the transcript left its pattern: " + tr->violation());
        p->tr = std::move(tr);
        p->alpha = alpha;
        if (alpha_out) memcpy(alpha_out, alpha.v, 32);
        *d_hf_out = p->at<uint64_t>(p->lay.h_f);
        *d_ht_out = p->at<uint64_t>(p->lay.h_t);
        p->state = 2;
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

int pkl_finish(pkl_prover* p, const uint64_t* bind2, uint8_t* proof_out, size_t cap, size_t* len, pkl_claims* claims_out) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkl_statement& st = p->st;
    if (!len || (!proof_out && cap)) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    *len = p->fr.total;
    if (p->state < 2) return fail(p, PK_ERR_BAD_ARG, "pkl_finish needs a successful pkl_begin on this prover first");
    if (cap < p->fr.total) return fail(p, PK_ERR_BAD_ARG, "the proof buffer holds " + std::to_string(cap) + " bytes, the proof has " + std::to_string(p->fr.total));
    if (st.n_bind2 && !bind2) return fail(p, PK_ERR_BAD_ARG, "the statement binds elements after the helper tables: pass them");
    if (!elements_below_p(bind2, st.n_bind2)) return fail(p, PK_ERR_BAD_ARG, "a bind2 element is not below p");
    try {
        // from here on the transcript moves: whatever happens, the next proof starts at pkl_begin (the counts stay valid)
        std::unique_ptr<pk::Transcript> tr = std::move(p->tr);
        p->state = 1;
        if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
        fe s;
        if (hipMemcpy(s.v, p->at<uint64_t>(p->lay.sum), 32, hipMemcpyDeviceToHost) != hipSuccess) return fail(p, PK_ERR_HIP, "the sum did not arrive");
        for (unsigned i = 0; i < st.n_bind2; i++) tr->add_scalar(pk::h_load(bind2 + 4 * i));
        tr->add_scalar(s);
        fe tau_f[PKL_MAX_VARS], tau_t[PKL_MAX_VARS];
        tr->challenge_scalars(tau_f, st.n);
        tr->challenge_scalars(tau_t, st.k);
        const fe seed = tr->challenge_scalar();
        if (!tr->finished()) return fail(p, PK_ERR_IO_PATTERN, "the transcript left its pattern: " + tr->violation());

        const fe canon = pk::h_to_canon(s);
        memcpy(proof_out, canon.v, 32);
        fe r_f[PKL_MAX_VARS], r_t[PKL_MAX_VARS], finals_f[2], finals_t[3];
        const uint64_t* const tables_f[2] = {p->at<uint64_t>(p->lay.h_f), p->at<uint64_t>(p->lay.d_f)};
        const uint64_t* const tables_t[3] = {p->at<uint64_t>(p->lay.h_t), p->at<uint64_t>(p->lay.d_t), p->d_m};
        size_t part = 0;
        auto t0 = std::chrono::steady_clock::now();
        if (int rc = pks_prove(p->side[0], tables_f, (const uint64_t*)tau_f, (const uint64_t*)seed.v, proof_out + p->fr.f_at, p->fr.f_len, &part, (uint64_t*)r_f,
                               (uint64_t*)finals_f))
            return fail(p, rc, std::string("the f side's sumcheck failed: ") + pks_last_error(p->side[0]));
        p->prof.sumcheck_f_ms = host_ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        if (int rc = pks_prove(p->side[1], tables_t, (const uint64_t*)tau_t, (const uint64_t*)seed.v, proof_out + p->fr.t_at, p->fr.t_len, &part, (uint64_t*)r_t,
                               (uint64_t*)finals_t))
            return fail(p, rc, std::string("the t side's sumcheck failed: ") + pks_last_error(p->side[1]));
        p->prof.sumcheck_t_ms = host_ms_since(t0);
        if (claims_out) pkl::derive_claims(st, p->alpha, s, r_f, r_t, finals_f, finals_t, claims_out);
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

}  // extern "C"
