// prover_transcript.hpp -- the prover side of the Fiat-Shamir transcript (spongefish ProverState): protocol.hpp's sponge and
// IO-pattern cursor, the proof string the operations write, and the timing PK_PROVE_TIMING reports.
#pragma once
#include <chrono>

#include "protocol.hpp"

namespace pk {

class Transcript {
  public:
    std::vector<uint8_t> narg;  // the proof string (WhirR1CSProof::transcript)
    double permute_seconds = 0.0;  // host time spent in the sponge, which is its permutation's (PK_PROVE_TIMING)
    double hint_seconds = 0.0;     // host time spent serialising opening hints (PK_PROVE_TIMING)

    explicit Transcript(const std::string& io_pattern) : sponge_(io_pattern) {
        if (!io_pattern_parse(io_pattern, ops_, violation_)) ops_.clear();
    }
    Transcript(const Transcript&) = delete;  // cur_ refers to ops_
    unsigned permutes() const { return sponge_.permutes; }
    // "" while every operation so far matched the declared pattern; otherwise the first mismatch (spongefish: InvalidIOPattern)
    const std::string& violation() const { return violation_; }
    // ... and nothing declared was left undone (spongefish checks this when the state is dropped)
    bool finished() const { return violation_.empty() && cur_.at_end(); }
    // what a verifier challenge would be at this point, from a copy of the sponge: the transcript itself does not move (the ranks
    // of a device set compare it to see that they absorbed the same statement)
    fe peek_challenge() const {
        DuplexSponge copy = sponge_;
        return copy.squeeze();
    }
    // prover -> verifier: field elements (Montgomery in memory), written canonical LE and absorbed
    void add_scalars(const fe* mont, size_t n) {
        for (size_t i = 0; i < n; i++) add_canon(h_to_canon(mont[i]));
    }
    void add_scalar(const fe& mont) { add_scalars(&mont, 1); }
    // a digest is already a canonical value (provekit/common/src/skyscraper/whir.rs:96-102)
    void add_canon(const fe& canon) {
        expect('A', 1);
        append(canon.v, 32);
        Lap lap{permute_seconds};
        sponge_.absorb(canon);
    }
    // verifier -> prover
    fe challenge_scalar() {
        expect('S', 1);
        Lap lap{permute_seconds};
        return h_from_canon(sponge_.squeeze());
    }
    void challenge_scalars(fe* out, size_t n) {
        for (size_t i = 0; i < n; i++) out[i] = challenge_scalar();
    }
    void challenge_bytes(uint8_t* out, size_t n) {
        expect('S', units_for_bytes(n));
        Lap lap{permute_seconds};
        sponge_.squeeze_bytes(out, n);
    }
    void add_bytes(const uint8_t* b, size_t n) {
        expect('A', n);
        append(b, n);
        Lap lap{permute_seconds};
        sponge_.absorb_bytes(b, n);
    }
    void hint(const void* payload, size_t len) {
        expect('H', 1);
        const hint_len_t l = (hint_len_t)len;
        append(&l, sizeof l);
        append(payload, len);
    }

  private:
    struct Lap {  // adds the time to the end of its scope to `acc`
        double& acc;
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        ~Lap() { acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    };
    DuplexSponge sponge_;
    std::vector<IoOp> ops_;
    IoCursor cur_{ops_};
    std::string violation_;
    void expect(char kind, size_t n) {
        if (!violation_.empty() || cur_.take(kind, n)) return;
        violation_ = std::string("transcript operation ") + kind + std::to_string(n) + " does not follow the IO pattern: operation #" +
                     std::to_string(cur_.op_index() + 1) + " is " +
                     (cur_.at_end() ? std::string("past the end") : std::string(1, cur_.kind()) + std::to_string(cur_.remaining()) + " (remaining)");
    }
    void append(const void* p, size_t n) {
        const uint8_t* b = static_cast<const uint8_t*>(p);
        narg.insert(narg.end(), b, b + n);
    }
};

}  // namespace pk
