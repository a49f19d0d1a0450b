// prover.hpp -- what a pkl_prover holds, for prover.cpp; and for the lab (tools/probes/lookup.hip), which sets the grid of a prover's
// kernels and reads where its last proof's time went: test and benchmark knobs that the C ABI does not carry.
#pragma once
#include <memory>

#include "../prover_transcript.hpp"
#include "../sumcheck/round.hpp"
#include "kernels.hpp"

namespace pkl {

// Where the last proof's time went, in milliseconds: the three kernel phases' device time (events around each phase's launches) and
// the two pks_prove calls' host time -- two clocks.  A phase that has not run since the prover was made reads 0.
struct Profile {
    double count_ms = 0;       // count_kernel and the Montgomery pass over m (pkl_multiplicities)
    double table_ms = 0;       // table_kernel and the finish of s (pkl_begin)
    double gather_ms = 0;      // the gather (pkl_begin)
    double sumcheck_f_ms = 0;  // pks_prove of the f side (pkl_finish)
    double sumcheck_t_ms = 0;  // pks_prove of the t side (pkl_finish)
};

// the two pks provers' arenas (sumcheck/round.hpp states what pks_prover_create allocates)
inline size_t sides_arena_bytes(const pkl_statement& s) {
    size_t fes = 0;
    for (int side = PKL_SIDE_F; side <= PKL_SIDE_T; side++) {
        const pks_statement ps = side_statement(s, side);
        fes += pks::lone_arena_fes(ps.n, ps.m);
    }
    return 32 * fes;
}

}  // namespace pkl

struct pkl_prover {
    pk_ctx* ctx = nullptr;
    pkl_statement st{};
    std::string pattern, err;
    pkl::Layout lay;
    pkl::Framing fr;
    char* arena = nullptr;
    pks_prover* side[2] = {nullptr, nullptr};  // F, T
    pkl::GatherPlan gather;
    unsigned grid = 0;  // the workgroups of every kernel here; 0: each kernel's rule.  No bit of a result depends on it
    // 0: nothing counted; 1: pkl_multiplicities succeeded; 2: pkl_begin succeeded, the transcript stands after alpha
    int state = 0;
    const uint64_t* d_t = nullptr;
    const uint32_t* d_idx = nullptr;
    const uint64_t* d_m = nullptr;
    std::unique_ptr<pk::Transcript> tr;
    pk::fe alpha;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // around the launches of one call, on the null stream
    pkl::Profile prof;

    pkl_prover() = default;
    pkl_prover(const pkl_prover&) = delete;
    pkl_prover& operator=(const pkl_prover&) = delete;
    // gives back whatever the prover holds, so a creation that stops half way leaks nothing; rc: the first failure's code
    int give_back() {
        int rc = PK_OK;
        for (pks_prover*& s : side) {
            if (s)
                if (int r = pks_prover_destroy(s)) rc = rc ? rc : r;
            s = nullptr;
        }
        for (hipEvent_t& e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        if (arena)
            if (int r = pk_free(ctx, arena)) rc = rc ? rc : r;
        arena = nullptr;
        return rc;
    }
    ~pkl_prover() { (void)give_back(); }

    template <class T>
    T* at(size_t offset) const {
        return (T*)(arena + offset);
    }
};
