// asan_main.cpp -- driver of the sanitizer build of this library's host verifier (make asan; CPU code only):
//   pkl_verify_asan verify <case file>
//       u32 n, k, n_bind, n_bind2 | u32 pattern length | pattern | bind (n_bind elements) | bind2 (n_bind2 elements) |
//       u32 count | count x (u64 length | bytes)
//     verifies every proof with pkl_verify and prints "rc accepted check side offset" per proof.  A statement the library refuses
//     prints one REFUSED line and nothing of the rest is read: its counts size nothing.  Proofs and bind elements live in exact-size
//     heap blocks, so that a read past an end is a report, not a read of the next item.

#include "../../../include/provekit_lookup.h"
#include "../asan_case.hpp"

namespace {

int run_verify(const char* path) {
    if (!asan_case::read_file(path)) return 2;
    uint32_t head[4];
    asan_case::take(head, sizeof head);
    pkl_statement st{head[0], head[1], head[2], head[3]};
    size_t proof_len = 0;
    asan_case::Proofs d;
    d.n_bind = st.n_bind, d.n_bind2 = st.n_bind2, d.layer_column = false, d.side = -1, d.create_error = pkl_create_error, d.check_name = pks_check_name;
    if (int rc = pkl_proof_bytes(&st, &proof_len)) return asan_case::refused(d, rc), 0;
    pkl_claims* claims = (pkl_claims*)malloc(sizeof(pkl_claims));
    asan_case::run_proofs<pkv_result>(d, [&](const uint8_t* pattern, size_t pattern_len, const uint64_t* bind, const uint64_t* bind2, const uint8_t* proof,
                                             size_t len, int* side, unsigned*, pkv_result* r) {
        return pkl_verify(&st, pattern, pattern_len, bind, bind2, proof, len, claims, side, r);
    });
    free(claims);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "verify")) return run_verify(argv[2]);
    fprintf(stderr, "usage: pkl_verify_asan verify <case file>\n");
    return 2;
}
