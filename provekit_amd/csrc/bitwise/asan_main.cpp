// asan_main.cpp -- driver of the sanitizer build of this library's host verifier (make asan; CPU code only):
//   pkb_verify_asan verify <case file>
//       u32 n, op, d, L, n_bind | u32 pattern length | pattern | bind (n_bind elements) | u32 count | count x (u64 length | bytes)
//     verifies every proof with pkb_verify and prints "rc accepted check side layer offset" per proof.  A statement the library
//     refuses prints one REFUSED line and nothing of the rest is read: its counts size nothing.  Proofs and the bind elements live in
//     exact-size heap blocks, so that a read past an end is a report, not a read of the next item.

#include "../../../include/provekit_bitwise.h"
#include "../asan_case.hpp"

namespace {

int run(const char* path) {
    if (!asan_case::read_file(path)) return 2;
    uint32_t head[5];
    asan_case::take(head, sizeof head);
    const pkb_statement st{head[0], head[1], head[2], head[3], head[4]};
    size_t proof_len = 0;
    asan_case::Proofs d;
    d.create_error = pkb_create_error, d.check_name = pkb_check_name;
    if (int rc = pkb_proof_bytes(&st, &proof_len)) return asan_case::refused(d, rc), 0;
    d.n_bind = st.n_bind;  // only now: the statement's counts are inside their ranges
    pkb_claims* claims = (pkb_claims*)malloc(sizeof(pkb_claims));
    asan_case::run_proofs<pkv_result>(d, [&](const uint8_t* pattern, size_t pattern_len, const uint64_t* bind, const uint64_t*, const uint8_t* proof, size_t len, int* side,
                                             unsigned* layer, pkv_result* r) { return pkb_verify(&st, pattern, pattern_len, bind, proof, len, claims, side, layer, r); });
    free(claims);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "verify")) return run(argv[2]);
    fprintf(stderr, "usage: pkb_verify_asan verify <case file>\n");
    return 2;
}
