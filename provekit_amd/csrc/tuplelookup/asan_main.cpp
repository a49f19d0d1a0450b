// asan_main.cpp -- driver of the sanitizer build of this library's host verifier (make asan; CPU code only):
//   pkt_verify_asan verify <case file>
//       u32 n, k, w, c, n_bind | u32 pattern length | pattern | bind (n_bind elements) | u32 count | count x (u64 length | bytes)
//     verifies every proof with pkt_verify and prints "rc accepted check side layer offset" per proof.  A statement the library refuses
//     prints one REFUSED line and nothing of the rest is read: its counts size nothing.  Proofs and bind elements live in exact-size
//     heap blocks, so that a read past an end is a report, not a read of the next item.

#include "../../../include/provekit_tuplelookup.h"
#include "../asan_case.hpp"

namespace {

using asan_case::take;
using asan_case::take_block;

int run(const char* path) {
    if (!asan_case::read_file(path)) return 2;
    uint32_t head[5];
    take(head, sizeof head);
    const pkt_statement st{head[0], head[1], head[2], head[3], head[4]};
    size_t proof_len = 0;
    int rc = pkt_proof_bytes(&st, &proof_len);
    if (rc) {
        printf("%d 0 REFUSED 0 0 0 %s\n", rc, pkt_create_error());
        return 0;
    }
    uint32_t pattern_len, count;
    take(&pattern_len, 4);
    uint8_t* pattern = (uint8_t*)take_block(pattern_len);
    uint64_t* bind = st.n_bind ? (uint64_t*)take_block(32 * (size_t)st.n_bind) : nullptr;
    take(&count, 4);
    pkt_claims* claims = (pkt_claims*)malloc(sizeof(pkt_claims));
    for (uint32_t c = 0; c < count; c++) {
        uint64_t len;
        take(&len, 8);
        uint8_t* proof = (uint8_t*)take_block(len);
        pkv_result r;
        int side = 0;
        unsigned layer = 0;
        rc = pkt_verify(&st, pattern_len ? pattern : nullptr, pattern_len, bind, proof, len, claims, &side, &layer, &r);
        if (rc)
            printf("%d 0 REFUSED 0 0 0 %s\n", rc, pkt_create_error());
        else
            printf("0 %d %s %d %u %llu\n", r.accepted, pkt_check_name(r.check), side, layer, (unsigned long long)r.offset);
        free(proof);
    }
    free(claims), free(bind), free(pattern);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "verify")) return run(argv[2]);
    fprintf(stderr, "usage: pkt_verify_asan verify <case file>\n");
    return 2;
}
