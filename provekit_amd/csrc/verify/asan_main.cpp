// asan_main.cpp -- driver of the sanitizer build of the host core (make asan; CPU code only): reads one case file, verifies every
// proof in it with pkv_verify and prints "accepted check offset" per proof.  tests/test_verify_host.py writes the file:
//   u32 m, m_0, hash_version | pk_whir_config witness | pk_whir_config blinding | u32 pattern length | pattern |
//   u32 n_cases | n_cases x (u64 length | bytes)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../include/provekit_verify.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> buf;
    uint8_t chunk[1 << 16];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) buf.insert(buf.end(), chunk, chunk + n);
    fclose(f);
    size_t i = 0;
    auto take = [&](void* dst, size_t n) {
        if (buf.size() - i < n) exit(2);
        memcpy(dst, buf.data() + i, n);
        i += n;
    };
    uint32_t head[3], plen, n_cases;
    pk_whir_config cw, cb;
    take(head, sizeof head);
    take(&cw, sizeof cw);
    take(&cb, sizeof cb);
    take(&plen, 4);
    if (buf.size() - i < plen) return 2;
    const uint8_t* pattern = buf.data() + i;
    i += plen;
    pkv_verifier* v = nullptr;
    if (pkv_verifier_create(head[0], head[1], &cw, &cb, pattern, plen, (int)head[2], &v)) {
        fprintf(stderr, "create: %s\n", pkv_create_error());
        return 3;
    }
    take(&n_cases, 4);
    for (uint32_t c = 0; c < n_cases; c++) {
        uint64_t len;
        take(&len, 8);
        if (buf.size() - i < len) return 2;
        // an exact-size heap copy, so that a read past the proof's end is a report, not a read of the next case
        uint8_t* proof = (uint8_t*)malloc(len ? len : 1);
        memcpy(proof, buf.data() + i, len);
        i += len;
        pkv_result r;
        if (pkv_verify(v, proof, len, &r)) return 4;
        printf("%d %s %llu\n", r.accepted, pkv_check_name(r.check), (unsigned long long)r.offset);
        free(proof);
    }
    pkv_verifier_destroy(v);
    return 0;
}
