// argument.hpp -- the host frame the argument libraries above the product's C ABI share (sumcheck/, lookup/, grandproduct/): how a
// call refuses and a prover fails, the checks and copies of public elements, the IO pattern's zero-count rule, a verifier's
// "caller's pattern or our own", the pattern's copy-out, and the two clocks of a profile.  Host only; nothing beyond verify/core.hpp.
#pragma once
#include <chrono>

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

// *_io_pattern's answer: the length always, the bytes when they fit
inline int pattern_out(const std::string& d, uint8_t* buf, size_t cap, size_t* len) {
    *len = d.size();
    if (buf && cap >= d.size()) memcpy(buf, d.data(), d.size());
    return PK_OK;
}

// device milliseconds between two recorded events whose work has completed
inline double between(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? (double)ms : 0.0;
}
inline double host_ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace pk
