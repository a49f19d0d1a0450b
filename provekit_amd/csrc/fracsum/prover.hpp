// prover.hpp -- what a pkf_prover and a pkf_lookup_prover hold, for prover.cpp; and for the lab (tools/probes/fracsum.hip), which
// sets the grid and the layers per launch of a prover's kernels and reads where its last proof's time went: test and benchmark knobs
// that the C ABI does not carry.
#pragma once
#include "../sumcheck/round.hpp"
#include "kernels.hpp"

namespace pkf {

// Where the last proof's time went, in milliseconds: the device time of the tree phase and of each layer's combine pass (events around
// their launches), and each layer's pks_prove in host time -- two clocks.  Index d is layer d's (1 <= d < n); what has not run reads 0.
struct Profile {
    double tree_ms = 0;
    double combine_ms[PKF_MAX_VARS] = {};
    double layer_ms[PKF_MAX_VARS] = {};
};

// the n - 1 pks provers' arenas (sumcheck/round.hpp states what pks_prover_create allocates)
inline size_t layers_arena_bytes(const pkf_statement& s) {
    size_t fes = 0;
    for (unsigned d = 1; d < s.n; d++) fes += pks::lone_arena_fes(d, layer_tables(s, d));
    return 32 * fes;
}

}  // namespace pkf

// gkr/chain.hpp's frame (ctx, pattern, err, layer[], grid, layers; ev[4]: around the tree phase and around a layer's combine pass, on
// the null stream) and what is the fractional sum's own
struct pkf_prover : pk::gkr::ProverFrame<4> {
    pkf_statement st{};
    uint64_t* arena = nullptr;  // ptree | qtree | u (layout.hpp)
    uint64_t *ptree = nullptr, *qtree = nullptr, *u = nullptr;
    pk::fe top[4], P, Q;  // of the trees as they stand (build / build_lookup)
    pkf::Profile prof;

    int give_back() {
        ptree = qtree = u = nullptr;
        return ProverFrame::give_back(arena);
    }
    ~pkf_prover() { (void)give_back(); }
};

struct pkf_lookup_prover {
    pk_ctx* ctx = nullptr;
    pkf_lookup_statement st{};
    std::string pattern, err;
    uint64_t* leaf[2] = {nullptr, nullptr};  // alpha - f (2^n elements) and alpha - t (2^k)
    pkf_prover* side[2] = {nullptr, nullptr};  // PKF_SIDE_F: (n, unit), PKF_SIDE_T: (k, numerators m)

    pkf_lookup_prover() = default;
    pkf_lookup_prover(const pkf_lookup_prover&) = delete;
    pkf_lookup_prover& operator=(const pkf_lookup_prover&) = delete;
    int give_back() {
        int rc = PK_OK;
        for (int which = 0; which < 2; which++) {
            if (side[which]) {
                if (int r = side[which]->give_back()) rc = rc ? rc : r;
                delete side[which];
            }
            side[which] = nullptr;
            if (leaf[which])
                if (int r = pk_free(ctx, leaf[which])) rc = rc ? rc : r;
            leaf[which] = nullptr;
        }
        return rc;
    }
    ~pkf_lookup_prover() { (void)give_back(); }
};
