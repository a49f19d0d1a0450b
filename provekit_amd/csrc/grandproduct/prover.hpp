// prover.hpp -- what a pkg_prover and a pkg_multiset_prover hold, for prover.cpp; and for the lab (tools/probes/grandproduct.hip),
// which sets the grid and the layers per launch of a prover's kernels and reads where its last proof's time went: test and benchmark
// knobs that the C ABI does not carry.
#pragma once
#include "../sumcheck/round.hpp"
#include "kernels.hpp"

namespace pkg {

// Where the last proof's time went, in milliseconds: the tree phase's device time (events around its launches) and each layer's
// pks_prove in host time -- two clocks.  layer_ms[d] is layer d's (1 <= d < n); what has not run reads 0.
struct Profile {
    double tree_ms = 0;
    double layer_ms[PKG_MAX_VARS] = {};
};

// the n - 1 pks provers' arenas (sumcheck/round.hpp states what pks_prover_create allocates)
inline size_t layers_arena_bytes(unsigned n) {
    size_t fes = 0;
    for (unsigned d = 1; d < n; d++) fes += pks::lone_arena_fes(d, 2);
    return 32 * fes;
}

}  // namespace pkg

// gkr/chain.hpp's frame (ctx, pattern, err, layer[], grid, layers; ev[2]: around the tree phase, on the null stream) and what is the
// grand product's own
struct pkg_prover : pk::gkr::ProverFrame<2> {
    pkg_statement st{};
    uint64_t* tree = nullptr;  // the arena: 2^n elements, heap layout
    pk::fe top[2], product;    // of the tree as it stands (build / build_leaves)
    pkg::Profile prof;

    int give_back() { return ProverFrame::give_back(tree); }
    ~pkg_prover() { (void)give_back(); }
};

struct pkg_multiset_prover {
    pk_ctx* ctx = nullptr;
    pkg_multiset_statement st{};
    std::string pattern, err;
    uint64_t* leaf = nullptr;  // the one leaf table, 2^n elements: side B's while the products are compared, then A's, then B's again
    pkg_prover* inner = nullptr;

    pkg_multiset_prover() = default;
    pkg_multiset_prover(const pkg_multiset_prover&) = delete;
    pkg_multiset_prover& operator=(const pkg_multiset_prover&) = delete;
    int give_back() {
        int rc = PK_OK;
        if (inner) {
            rc = inner->give_back();
            delete inner;
        }
        inner = nullptr;
        if (leaf)
            if (int r = pk_free(ctx, leaf)) rc = rc ? rc : r;
        leaf = nullptr;
        return rc;
    }
    ~pkg_multiset_prover() { (void)give_back(); }
};
