// asan_case.hpp -- the case-file reader of the sanitizer drivers (sumcheck/, lookup/, grandproduct/, fracsum/, tuplelookup/
// asan_main.cpp): the file in one buffer, taken from front to back, and the loop over a case's proofs that four of them share.  A case
// that ends early ends the program with status 2.  Host only.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace asan_case {

inline std::vector<uint8_t> buf;  // the case file
inline size_t at = 0;

inline bool read_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t chunk[65536];
    for (size_t got; (got = fread(chunk, 1, sizeof chunk, f)) > 0;) buf.insert(buf.end(), chunk, chunk + got);
    fclose(f);
    return true;
}
inline void take(void* dst, size_t n) {
    if (buf.size() - at < n) exit(2);
    if (n) memcpy(dst, buf.data() + at, n);
    at += n;
}
// the next n bytes in a heap block of exactly that size, so that a read past its end is a report, not a read of the next item
inline void* take_block(size_t n) {
    if (buf.size() - at < n) exit(2);
    void* p = malloc(n ? n : 1);
    take(p, n);
    return p;
}

// What the drivers of lookup/, grandproduct/, fracsum/ and tuplelookup/ share once the statement's head is read and the library took it:
//     u32 pattern length | pattern | bind (n_bind elements) [| bind2 (n_bind2 elements)] | u32 count | count x (u64 length | bytes)
// pattern, bind elements and every proof in exact-size heap blocks; per proof one line "0 accepted check side [layer] offset", or the
// REFUSED line where the library refuses the call.
struct Proofs {
    unsigned n_bind = 0, n_bind2 = 0;
    bool layer_column = true;  // lookup/ has no layers
    int side = 0;              // what a verifier that names no side leaves
    const char* (*create_error)() = nullptr;
    const char* (*check_name)(int) = nullptr;
};
// "rc 0 REFUSED 0 .. reason": a zero for every column after the check
inline void refused(const Proofs& d, int rc) { printf(d.layer_column ? "%d 0 REFUSED 0 0 0 %s\n" : "%d 0 REFUSED 0 0 %s\n", rc, d.create_error()); }
// verify(pattern or NULL, its length, bind, bind2, proof, its length, &side, &layer, &result) is the library's verifier: its rc
template <class Result, class Verify>
int run_proofs(const Proofs& d, Verify&& verify) {
    uint32_t pattern_len, count;
    take(&pattern_len, 4);
    uint8_t* pattern = (uint8_t*)take_block(pattern_len);
    uint64_t* bind = d.n_bind ? (uint64_t*)take_block(32 * (size_t)d.n_bind) : nullptr;
    uint64_t* bind2 = d.n_bind2 ? (uint64_t*)take_block(32 * (size_t)d.n_bind2) : nullptr;
    take(&count, 4);
    for (uint32_t c = 0; c < count; c++) {
        uint64_t len;
        take(&len, 8);
        uint8_t* proof = (uint8_t*)take_block(len);
        Result r;
        int side = d.side;
        unsigned layer = 0;
        if (const int rc = verify(pattern_len ? pattern : nullptr, (size_t)pattern_len, bind, bind2, proof, (size_t)len, &side, &layer, &r))
            refused(d, rc);
        else if (d.layer_column)
            printf("0 %d %s %d %u %llu\n", r.accepted, d.check_name(r.check), side, layer, (unsigned long long)r.offset);
        else
            printf("0 %d %s %d %llu\n", r.accepted, d.check_name(r.check), side, (unsigned long long)r.offset);
        free(proof);
    }
    free(bind2), free(bind), free(pattern);
    return 0;
}

}  // namespace asan_case
