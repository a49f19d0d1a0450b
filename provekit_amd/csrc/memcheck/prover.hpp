// prover.hpp -- what a pkm_prover holds, for prover.cpp; and for the lab (tools/probes/memcheck.hip), which sets the grid of a
// prover's kernels and reads where its last calls' time went: test and benchmark knobs that the C ABI does not carry.
#pragma once
#include <memory>
#include <vector>

#include "../prover_transcript.hpp"
#include "kernels.hpp"

namespace pkm {

// Where the last calls' time went, in milliseconds: the device time of the last pkm_trace's four phases and of the last proof's two
// leaf launches (events around them), and the three sides' inner proofs in host time -- two clocks.  What has not run reads 0.
struct Profile {
    double key_ms = 0, sort_ms = 0, resolve_ms = 0, count_ms = 0, leaf_ms = 0;
    double side_ms[3] = {};
};

}  // namespace pkm

struct pkm_prover {
    pk_ctx* ctx = nullptr;
    pkm_statement st{};
    std::string pattern, err;
    uint8_t* arena = nullptr;  // layout.hpp
    pkm::Layout at;
    pkf_prover* sum[2] = {nullptr, nullptr};  // PKM_SIDE_OPS: (n + 1, numerators the signs), PKM_SIDE_MEM: (k + 1, the same)
    pkf_lookup_prover* time = nullptr;        // PKM_SIDE_TIME: (n, n)
    size_t side_bytes[3] = {0, 0, 0};         // the three parts of a proof
    std::vector<uint8_t> staging;             // all three, until the balance and the lookup's fractions have been checked
    unsigned grid = 0;  // the workgroups of every kernel of mem.hip; 0: the rule.  No bit of a result depends on it
    hipEvent_t ev[5] = {};  // around a call's phases, on the null stream
    pkm::Profile prof;

    uint64_t* q(int side) const { return (uint64_t*)(arena + at.q[side]); }
    uint64_t* sign(int side) const { return (uint64_t*)(arena + at.sign[side]); }
    uint64_t* f() const { return (uint64_t*)(arena + at.f); }
    uint64_t* t() const { return (uint64_t*)(arena + at.t); }
    pkm::TraceScratch scratch() const {
        return pkm::TraceScratch{(unsigned long long*)(arena + at.keys), (unsigned long long*)(arena + at.sorted), (uint32_t*)(arena + at.counts), arena + at.sort_tmp,
                                 at.bad - at.sort_tmp, (unsigned long long*)(arena + at.bad)};
    }

    pkm_prover() = default;
    pkm_prover(const pkm_prover&) = delete;
    pkm_prover& operator=(const pkm_prover&) = delete;
    // gives back whatever the prover holds, so a creation that stops half way leaks nothing; rc: the first failure's code
    int give_back() {
        int rc = PK_OK;
        for (pkf_prover*& s : sum) {
            if (s)
                if (int r = pkf_prover_destroy(s)) rc = rc ? rc : r;
            s = nullptr;
        }
        if (time)
            if (int r = pkf_lookup_prover_destroy(time)) rc = rc ? rc : r;
        time = nullptr;
        for (hipEvent_t& e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        if (arena)
            if (int r = pk_free(ctx, arena)) rc = rc ? rc : r;
        arena = nullptr;
        return rc;
    }
    ~pkm_prover() { (void)give_back(); }
};
