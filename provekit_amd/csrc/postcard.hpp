// postcard.hpp -- reader of the postcard encoding the reference serialises with (provekit/common/src/file/bin.rs:22-71): usize / u32 =
// LEB128 varint, Vec<T> = varint length + items, bytes = varint length + raw.  Host only; the input is untrusted: a failed read sets
// `ok` to false for good, and a length is bounded by the bytes that remain before anything is sized from it.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "fe.hpp"

namespace pk {
namespace postcard {

struct Reader {
    const uint8_t* p;
    size_t n, off = 0;
    bool ok = true;
    uint64_t varint() {
        uint64_t v = 0;
        for (unsigned shift = 0; shift < 70; shift += 7) {
            if (off >= n) return ok = false, 0;
            const uint8_t b = p[off++];
            if (shift == 63 && b > 1) return ok = false, 0;
            v |= (uint64_t)(b & 0x7f) << shift;
            if (!(b & 0x80)) return v;
        }
        return ok = false, 0;
    }
    uint64_t below(uint64_t limit) {  // a usize / u32 that must stay under `limit`
        const uint64_t v = varint();
        if (v >= limit) ok = false;
        return v;
    }
    uint64_t vec_len() {  // of a Vec whose items take at least one byte each
        const uint64_t len = varint();
        if (len > n - off) ok = false;
        return ok ? len : 0;
    }
    bool vec_u32(std::vector<uint32_t>& out) {
        out.resize(vec_len());
        for (uint32_t& x : out) {
            x = (uint32_t)below(1ull << 32);
            if (!ok) return false;
        }
        return ok;
    }
    // serde_ark: bytes(32) = varint(32) | canonical little-endian (provekit/common/src/utils/serde_ark.rs:11-30)
    bool field(fe& out) {
        if (varint() != 32 || !ok || n - off < 32) return ok = false;
        memcpy(out.v, p + off, 32);
        off += 32;
        fe red = fe_reduce_any(out);
        if (memcmp(red.v, out.v, 32) != 0) return ok = false;  // Fp::deserialize_compressed rejects values >= p
        return true;
    }
};

}  // namespace postcard
}  // namespace pk
