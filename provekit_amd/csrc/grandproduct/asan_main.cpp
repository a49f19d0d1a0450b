// asan_main.cpp -- driver of the sanitizer build of this library's host verifiers (make asan; CPU code only):
//   pkg_verify_asan verify <case file>
//       u32 n, n_bind | u32 pattern length | pattern | bind (n_bind elements) | u32 count | count x (u64 length | bytes)
//   pkg_verify_asan multiset <case file>
//       u32 n, w, n_bind | the rest as above
//     verifies every proof with pkg_verify / pkg_multiset_verify and prints "rc accepted check side layer offset" per proof (side 0
//     for a grand product).  A statement the library refuses prints one REFUSED line and nothing of the rest is read: its counts size
//     nothing.  Proofs and bind elements live in exact-size heap blocks, so that a read past an end is a report, not a read of the
//     next item.

#include "../../../include/provekit_grandproduct.h"
#include "../asan_case.hpp"

namespace {

using asan_case::take;
using asan_case::take_block;

int run(const char* path, bool multiset) {
    if (!asan_case::read_file(path)) return 2;
    pkg_statement st{};
    pkg_multiset_statement ms{};
    size_t proof_len = 0;
    int rc;
    if (multiset) {
        uint32_t head[3];
        take(head, sizeof head);
        ms = pkg_multiset_statement{head[0], head[1], head[2]};
        rc = pkg_multiset_proof_bytes(&ms, &proof_len);
    } else {
        uint32_t head[2];
        take(head, sizeof head);
        st = pkg_statement{head[0], head[1]};
        rc = pkg_proof_bytes(&st, &proof_len);
    }
    if (rc) {
        printf("%d 0 REFUSED 0 0 0 %s\n", rc, pkg_create_error());
        return 0;
    }
    const unsigned n = multiset ? ms.n : st.n, n_bind = multiset ? ms.n_bind : st.n_bind;
    uint32_t pattern_len, count;
    take(&pattern_len, 4);
    uint8_t* pattern = (uint8_t*)take_block(pattern_len);
    uint64_t* bind = n_bind ? (uint64_t*)take_block(32 * (size_t)n_bind) : nullptr;
    take(&count, 4);
    pkg_multiset_claims* claims = (pkg_multiset_claims*)malloc(sizeof(pkg_multiset_claims));
    uint64_t* point = (uint64_t*)malloc(32 * (size_t)n);  // exactly n coordinates
    uint64_t* scalars = (uint64_t*)malloc(64);
    for (uint32_t c = 0; c < count; c++) {
        uint64_t len;
        take(&len, 8);
        uint8_t* proof = (uint8_t*)take_block(len);
        pkv_result r;
        int side = 0;
        unsigned layer = 0;
        if (multiset)
            rc = pkg_multiset_verify(&ms, pattern_len ? pattern : nullptr, pattern_len, bind, proof, len, claims, &side, &layer, &r);
        else
            rc = pkg_verify(&st, pattern_len ? pattern : nullptr, pattern_len, bind, nullptr, proof, len, scalars, point, scalars + 4, &layer, &r);
        if (rc)
            printf("%d 0 REFUSED 0 0 0 %s\n", rc, pkg_create_error());
        else
            printf("0 %d %s %d %u %llu\n", r.accepted, pkg_check_name(r.check), side, layer, (unsigned long long)r.offset);
        free(proof);
    }
    free(scalars), free(point), free(claims), free(bind), free(pattern);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "verify")) return run(argv[2], false);
    if (argc == 3 && !strcmp(argv[1], "multiset")) return run(argv[2], true);
    fprintf(stderr, "usage: pkg_verify_asan verify|multiset <case file>\n");
    return 2;
}
