// asan_case.hpp -- the case-file reader of the sanitizer drivers (sumcheck/, lookup/, grandproduct/ asan_main.cpp): the file in one
// buffer, taken from front to back.  A case that ends early ends the program with status 2.  Host only.
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

}  // namespace asan_case
