// argument.hpp -- the host frame the argument libraries above the product's C ABI share (sumcheck/, lookup/, grandproduct/, fracsum/,
// tuplelookup/; gkr/chain.hpp builds on it): how a call refuses and a prover fails, the checks and copies of public elements, a prove
// call's opening checks, the IO pattern's zero-count rule, a verifier's "caller's pattern or our own", a verdict written by hand, the
// pattern's and a size's copy-out, a prover's creation and destruction, the two halves of a two-sided verifier (its squeeze-only outer transcript and the walk
// over its two parts), and the two clocks of a profile.  Host only; nothing beyond verify/core.hpp.
#pragma once
#include <chrono>
#include <initializer_list>
#include <memory>

#include "verify/core.hpp"

namespace pk {

// a refused call: the reason into the library's creation-error slot (one thread-local per library: each reports its own)
inline int refuse(std::string& slot, const std::string& why) {
    slot = why;
    return PK_ERR_BAD_ARG;
}
// a prover's failed call: the reason into the prover
template <class Prover>
int fail(Prover* p, int rc, const std::string& why) {
    p->err = why;
    return rc;
}
// what a creation's catch (...) returns
inline int out_of_host_memory(std::string& slot) {
    try {
        slot = "out of host memory while the prover was made";
    } catch (...) {
    }
    return PK_ERR_OOM;
}

// n Montgomery elements, each below p?  false: why = "<what> element <i> is not below p"
inline bool elements_below_p(const uint64_t* v, size_t n, const char* what, std::string& why) {
    for (size_t i = 0; i < n; i++)
        if (!is_canonical(h_load(v + 4 * i))) return why = std::string(what) + " element " + std::to_string(i) + " is not below p", false;
    return true;
}
// ... for a caller that states its own reason
inline bool elements_below_p(const uint64_t* v, size_t n) {
    std::string unused;
    return elements_below_p(v, n, "", unused);
}

// A prove call's opening lines once its own pointers are checked, with the prover's failure or PK_OK: room for the `need` bytes of the
// proof (*len = need in any case) ...
template <class Prover>
int proof_room(Prover* p, size_t need, size_t cap, size_t* len) {
    *len = need;
    if (cap < need) return fail(p, PK_ERR_BAD_ARG, "the proof buffer holds " + std::to_string(cap) + " bytes, the proof has " + std::to_string(need));
    return PK_OK;
}
// ... and the statement's bind elements present and below p
template <class Prover>
int bind_ok(Prover* p, const uint64_t* bind, size_t n_bind) {
    if (n_bind && !bind) return fail(p, PK_ERR_BAD_ARG, "the statement binds elements: pass them");
    std::string why;
    if (!elements_below_p(bind, n_bind, "bind", why)) return fail(p, PK_ERR_BAD_ARG, why);
    return PK_OK;
}
template <class Prover>
int proof_room_and_bind(Prover* p, size_t need, size_t cap, size_t* len, const uint64_t* bind, size_t n_bind) {
    const int rc = proof_room(p, need, cap, len);
    return rc ? rc : bind_ok(p, bind, n_bind);
}

inline bool is_zero(const fe& x) { return fe_eq(x, fe_zero()); }

// I(z) = sum_j z_j 2^(v-1-j): the multilinear extension of x -> x over v variables, variable 0 the most significant bit (the memory
// check's cell and time columns, Spark's index column)
inline fe index_at(const fe* z, unsigned v) {
    fe acc = fe_zero();
    for (unsigned j = 0; j < v; j++) acc = h_add(h_add(acc, acc), z[j]);  // Horner in 2
    return acc;
}

// whir_config.hip's zero-count rule: an operation of no elements is no operation
inline void pattern_op(std::string& d, char kind, size_t n, const char* label) {
    if (!n) return;
    d.push_back('\0');
    d += kind + std::to_string(n) + label;
}

inline void put_fe(uint64_t* dst, const fe& x) { memcpy(dst, x.v, 32); }

// public elements as the transcript reads them in front of the proof: canonical bytes
inline void put_canonical(std::vector<uint8_t>& bytes, const uint64_t* v, size_t n) {
    for (size_t i = 0; i < n; i++) {
        const fe c = h_to_canon(h_load(v + 4 * i));
        bytes.insert(bytes.end(), (const uint8_t*)c.v, (const uint8_t*)c.v + 32);
    }
}

// a verifier's pattern: the caller's or our own, parsed.  PK_ERR_IO_PATTERN: the reason is in the slot
inline int parse_pattern(pkv::Statement& st, const uint8_t* given, size_t given_len, const std::string& own, std::string& slot) {
    if (given && given_len)
        st.pattern.assign((const char*)given, given_len);
    else
        st.pattern = own;
    std::string why;
    if (io_pattern_parse(st.pattern, st.ops, why)) return PK_OK;
    slot = why;
    return PK_ERR_IO_PATTERN;
}

// a verdict that no transcript walk made: PKV_CHECK_NONE accepts
inline void verdict(pkv_result* r, int check, uint64_t offset, const std::string& msg) {
    pkv::Verdict v;
    v.failed = check != PKV_CHECK_NONE, v.check = check, v.offset = offset, v.message = msg;
    pkv::to_result(v, r);
}

// *_io_pattern's answer: the length always, the bytes when they fit
inline int pattern_out(const std::string& d, uint8_t* buf, size_t cap, size_t* len) {
    *len = d.size();
    if (buf && cap >= d.size()) memcpy(buf, d.data(), d.size());
    return PK_OK;
}
// What follows serves any statement type of a library.  Lib names the library's overload sets: Lib::ok(stmt, why) its statement_ok,
// Lib::pattern(*stmt) its io_pattern, Lib::error() its creation-error slot.
// *_io_pattern
template <class Lib, class S>
int pattern_out(const S* stmt, uint8_t* buf, size_t cap, size_t* len) {
    std::string why;
    if (!len) return refuse(Lib::error(), "null pointer");
    if (!Lib::ok(stmt, why)) return refuse(Lib::error(), why);
    try {
        return pattern_out(Lib::pattern(*stmt), buf, cap, len);
    } catch (...) {
        return PK_ERR_OOM;
    }
}
// *_proof_bytes and *_arena_bytes: size(*stmt) into *out
template <class Lib, class S, class Size>
int size_out(const S* stmt, size_t* out, Size&& size) {
    std::string why;
    if (!out) return refuse(Lib::error(), "null pointer");
    if (!Lib::ok(stmt, why)) return refuse(Lib::error(), why);
    *out = size(*stmt);
    return PK_OK;
}
// *_prover_create: make(p) fills the std::unique_ptr<Prover> or says why not in the slot; *_prover_destroy
template <class Lib, class S, class Prover, class Make>
int create(pk_ctx* ctx, const S* stmt, Prover** out, Make&& make) {
    if (out) *out = nullptr;
    std::string why;
    if (!ctx || !out) return refuse(Lib::error(), "null pointer");
    if (!Lib::ok(stmt, why)) return refuse(Lib::error(), why);
    try {
        std::unique_ptr<Prover> p;
        if (int rc = make(p)) return rc;
        *out = p.release();
        Lib::error().clear();
        return PK_OK;
    } catch (...) {
        return out_of_host_memory(Lib::error());
    }
}
template <class Prover>
int destroy(Prover* p) {
    if (!p) return PK_OK;
    const int rc = p->give_back();
    delete p;
    return rc;
}

// A two-sided verifier's outer transcript absorbs bind and only squeezes: each {count, where to} in order, a count of 0 being no
// operation.  false: the verdict (offset 0: nothing of the proof was read) is in *result
struct Squeeze {
    size_t count;
    fe* out;
};
inline bool squeeze_outer(const pkv::Statement& st, const uint64_t* bind, size_t n_bind, std::initializer_list<Squeeze> squeezes, pkv_result* result) {
    std::vector<uint8_t> bytes;
    put_canonical(bytes, bind, n_bind);
    pkv::Verdict v;
    pkv::Arthur A(st, bytes.data(), bytes.size(), v);
    std::vector<fe> scratch(n_bind);
    bool walked = !n_bind || A.next_scalars(n_bind, scratch.data());
    for (const Squeeze& s : squeezes) walked = walked && (!s.count || A.challenge_scalars(s.count, s.out));
    walked = walked && (A.done() || A.fail(PKV_CHECK_IO_PATTERN, "declared operations left after the outer transcript"));
    if (walked) return true;
    v.offset = 0;
    pkv::to_result(v, result);
    return false;
}

// The two parts of a two-sided proof, side 0's then side 1's, each of a fixed length: where a failure points.  *side_out and *layer_out
// (either may be NULL) start at 0.
struct TwoSides {
    size_t at[2], total;
    int* side_out;
    unsigned* layer_out;
    pkv_result* result;
    TwoSides(size_t bytes0, size_t bytes1, int* side, unsigned* layer, pkv_result* r) : at{0, bytes0}, total(bytes0 + bytes1), side_out(side), layer_out(layer), result(r) {
        if (layer_out) *layer_out = 0;
        if (side_out) *side_out = 0;
    }
    // framing first: both parts have a fixed length, so a proof of another length is judged before any part is read.  false: judged
    bool framed(size_t len) const {
        if (len < total) return verdict(result, PKV_CHECK_TRANSCRIPT_SHORT, len, "the proof is shorter than its two parts"), false;
        if (len > total) return verdict(result, PKV_CHECK_TRAILING_BYTES, total, "bytes left after the proof"), false;
        return true;
    }
    // verify_side(which, layer) judges the part at at[which] into *result, its offset in bytes of that part.  rc != 0: a refusal, passed
    // on.  PK_OK: *result is the first rejecting side's verdict or, accepted, the second side's, in bytes of the whole proof
    template <class F>
    int each(F&& verify_side) const {
        for (int which = 0; which < 2; which++) {
            unsigned layer = 0;
            if (int rc = verify_side(which, layer)) return rc;
            result->offset += at[which];
            if (side_out) *side_out = which;
            if (layer_out) *layer_out = layer;
            if (!result->accepted) return PK_OK;
        }
        return PK_OK;
    }
    // both sides and their comparison passed: no part to point at
    void accept() const {
        verdict(result, PKV_CHECK_NONE, total, "");
        if (side_out) *side_out = 0;
    }
};

// device milliseconds between two recorded events whose work has completed
inline double between(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? (double)ms : 0.0;
}
inline double host_ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace pk
