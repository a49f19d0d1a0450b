// shard_host.cpp -- the host-only part of the sharded prover's C ABI (include/provekit_sumcheck_sharded.h): pkss_plan, what a
// sharded proof of a statement takes on each of `world` ranks.  No device, no product call: the sanitizer build links it as it is.
#include "layout.hpp"

extern "C" {

int pkss_abi_version(void) { return 1; }

int pkss_plan(const pks_statement* stmt, unsigned world, struct pkss_plan* out) {
    std::string why;
    if (!out) return pks::refuse("null pointer");
    *out = {};
    if (!pks::statement_ok(stmt, why)) return pks::refuse(why);
    if (world < 2) return pks::refuse("world must be at least 2: a lone context proves with pks_prove");
    if (world & (world - 1)) return pks::refuse("world must be a power of two: " + std::to_string(world) + " ranks do not own whole index bits");
    if (world > 1u << PKSS_MAX_WORLD_LOG2) return pks::refuse("world must be at most " + std::to_string(1u << PKSS_MAX_WORLD_LOG2));
    unsigned g = 0;
    while ((1u << g) < world) g++;
    const pkss::Layout L = pkss::layout(stmt->n, stmt->m, g);
    out->g = g, out->c = pkss::C, out->S = L.S;
    out->local_len = L.S ? ((size_t)1 << stmt->n) >> g : 0;
    out->handover_len = L.handover;
    out->arena_bytes = 32 * L.total;
    pks::g_error.clear();
    return PK_OK;
}

}  // extern "C"
