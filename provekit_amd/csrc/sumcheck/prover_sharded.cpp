// prover_sharded.cpp -- the entry points of include/provekit_sumcheck_sharded.h that need a device: a prover on one rank of a device
// set, and one rank's slice of a round by itself.  Host code above provekit_hip.h's C ABI.  The prover, its loop and the single round
// are prover.cpp's, where a lone context is a device set of one; shard.hpp states who owns what.  What is here is what only a device
// set has: the world's refusals and the agreement on the statement at creation.
#include "../prover_transcript.hpp"
#include "prover.hpp"

using pk::fail;
using pk::fe;

namespace {

// what the ranks compare at creation: a sponge over the statement's counts and masks, the coefficients absorbed
fe statement_digest(const pks_statement& st) {
    std::string pat = "provekit-hip/sumcheck-sharded/v1/statement/n" + std::to_string(st.n) + "/m" + std::to_string(st.m) + "/tau" + std::to_string(st.has_tau) +
                      "/bind" + std::to_string(st.n_bind) + "/masks";
    for (unsigned t = 0; t < st.T; t++) pat += (t ? "." : "") + std::to_string(st.masks[t]);
    pat.push_back('\0');
    pat += "A" + std::to_string(st.T) + "coefficients";
    pat.push_back('\0');
    pat += "S1digest";
    pk::Transcript tr(pat);
    for (unsigned t = 0; t < st.T; t++) tr.add_scalar(pk::h_load(st.coeffs[t]));
    return tr.challenge_scalar();
}

}  // namespace

extern "C" {

int pkss_prover_create(pk_ctx* ctx, const pks_statement* stmt, pks_prover** out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return pks::refuse("null pointer");
    int rank = 0, world = 0, kind = PK_COMM_NONE;
    if (pk_comm_info(ctx, &rank, &world, &kind) != PK_OK || kind == PK_COMM_NONE || world < 2 || rank < 0 || rank >= world)
        return pks::refuse("the context is not in a device set: pks_prover_create proves on a lone context");
    if ((world & (world - 1)) || world > 1 << PKSS_MAX_WORLD_LOG2)
        return pks::refuse("a world of " + std::to_string(world) + " ranks: it must be a power of two, at most " + std::to_string(1 << PKSS_MAX_WORLD_LOG2) +
                           ", for every rank to own whole index bits");
    // collective from here: a rank that refuses its statement says so in the exchange, on the arena of the smallest statement
    std::string why;
    const bool ok = pks::statement_ok(stmt, why);
    try {
        std::unique_ptr<pks_prover> p;
        // a failure here has nothing to exchange on: the peers' wait ends at pk_comm's deadline
        if (int rc = pks::make_prover(ctx, ok ? stmt : nullptr, (unsigned)rank, (unsigned)world, p)) return rc;
        fe digest = pk::fe_zero();
        if (ok)
            digest = statement_digest(*stmt);
        else
            p->err = why;
        std::vector<fe> all;
        int rc = pks::exchange(p.get(), ok ? PK_OK : PK_ERR_BAD_ARG, &digest, 1, all);
        if (!rc)
            if (const unsigned r = pks::first_differing(all))
                rc = fail(p.get(), PK_ERR_BAD_ARG, "the ranks disagree on the statement: rank " + std::to_string(r) + "'s differs from rank 0's");
        if (rc) return pks::g_error = p->err, rc;
        *out = p.release();
        pks::g_error.clear();
        return PK_OK;
    } catch (...) {
        return pk::out_of_host_memory(pks::g_error);
    }
}

int pkss_prove(pks_prover* p, const uint64_t* const* d_tables, const uint64_t* tau_or_null, const uint64_t* bind, uint8_t* proof_out, size_t cap,
               size_t* len, uint64_t* point_out, uint64_t* finals_out) {
    if (!p) return PK_ERR_BAD_ARG;
    if (p->world < 2) return fail(p, PK_ERR_BAD_ARG, "a prover of pks_prover_create proves with pks_prove");
    return pks::prove(p, d_tables, tau_or_null, bind, proof_out, cap, len, point_out, finals_out);
}

int pkss_last_profile(const pks_prover* p, pkss_round_profile* rounds, unsigned cap, double* handover_seconds, double* total_seconds) {
    if (!p || p->world < 2 || (!rounds && cap)) return PK_ERR_BAD_ARG;
    for (unsigned i = 0; i < cap && i < p->profile.size(); i++) rounds[i] = p->profile[i];
    if (handover_seconds) *handover_seconds = p->handover_seconds;
    if (total_seconds) *total_seconds = p->total_seconds;
    return PK_OK;
}

int pkss_round_shard(pk_ctx* ctx, const pks_statement* stmt, const uint64_t* const* d_tables, size_t len, const uint64_t* tau_rest_or_null,
                     const uint64_t* fold_or_null, uint64_t* const* d_out_local, unsigned world, unsigned rank, unsigned grid, uint64_t* out) {
    if (!ctx || !d_tables || !out) return pks::refuse("null pointer");
    struct pkss_plan plan;
    if (int rc = pkss_plan(stmt, world, &plan)) return rc;  // the statement's and the world's refusals
    if (rank >= world) return pks::refuse("rank must be below world");
    const size_t round_len = fold_or_null ? len / 2 : len;
    if ((len & (len - 1)) || len > ((size_t)1 << stmt->n) || round_len < pkss::handover_len(plan.g))
        return pks::refuse("len must be a power of two, at most 2^n, and the round's length at least 2^(c+g+1) = " + std::to_string(pkss::handover_len(plan.g)) +
                           ": a shorter round is not sharded");
    const size_t pairs = round_len / 2;
    const pks::ShardSlice slice{plan.g, rank, true};
    return pks::round_alone(ctx, *stmt, d_tables, d_out_local, pairs, pairs >> plan.g, tau_rest_or_null, fold_or_null, grid, &slice, out);
}

}  // extern "C"
