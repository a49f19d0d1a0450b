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
    asan_case::Proofs d;
    d.n_bind = multiset ? ms.n_bind : st.n_bind, d.create_error = pkg_create_error, d.check_name = pkg_check_name;
    if (rc) return asan_case::refused(d, rc), 0;
    pkg_multiset_claims* claims = (pkg_multiset_claims*)malloc(sizeof(pkg_multiset_claims));
    uint64_t* point = (uint64_t*)malloc(32 * (size_t)(multiset ? ms.n : st.n));  // exactly n coordinates
    uint64_t* scalars = (uint64_t*)malloc(64);
    asan_case::run_proofs<pkv_result>(d, [&](const uint8_t* pattern, size_t pattern_len, const uint64_t* bind, const uint64_t*, const uint8_t* proof, size_t len,
                                             int* side, unsigned* layer, pkv_result* r) {
        if (multiset) return pkg_multiset_verify(&ms, pattern, pattern_len, bind, proof, len, claims, side, layer, r);
        return pkg_verify(&st, pattern, pattern_len, bind, nullptr, proof, len, scalars, point, scalars + 4, layer, r);
    });
    free(scalars), free(point), free(claims);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "verify")) return run(argv[2], false);
    if (argc == 3 && !strcmp(argv[1], "multiset")) return run(argv[2], true);
    fprintf(stderr, "usage: pkg_verify_asan verify|multiset <case file>\n");
    return 2;
}
