// asan_main.cpp -- driver of the sanitizer build of this library's host verifiers (make asan; CPU code only):
//   pkf_verify_asan verify <case file>
//       u32 n, n_bind, unit | u32 pattern length | pattern | bind (n_bind elements) | u32 count | count x (u64 length | bytes)
//   pkf_verify_asan lookup <case file>
//       u32 n, k, n_bind | the rest as above
//     verifies every proof with pkf_verify / pkf_lookup_verify and prints "rc accepted check side layer offset" per proof (side 0
//     for a fractional sum).  A statement the library refuses prints one REFUSED line and nothing of the rest is read: its counts size
//     nothing.  Proofs and bind elements live in exact-size heap blocks, so that a read past an end is a report, not a read of the
//     next item.

#include "../../../include/provekit_fracsum.h"
#include "../asan_case.hpp"

namespace {

using asan_case::take;

int run(const char* path, bool lookup) {
    if (!asan_case::read_file(path)) return 2;
    pkf_statement st{};
    pkf_lookup_statement ls{};
    size_t proof_len = 0;
    uint32_t head[3];
    take(head, sizeof head);
    int rc;
    if (lookup) {
        ls = pkf_lookup_statement{head[0], head[1], head[2]};
        rc = pkf_lookup_proof_bytes(&ls, &proof_len);
    } else {
        st = pkf_statement{head[0], head[1], head[2]};
        rc = pkf_proof_bytes(&st, &proof_len);
    }
    asan_case::Proofs d;
    d.n_bind = lookup ? ls.n_bind : st.n_bind, d.create_error = pkf_create_error, d.check_name = pkf_check_name;
    if (rc) return asan_case::refused(d, rc), 0;
    pkf_lookup_claims* claims = (pkf_lookup_claims*)malloc(sizeof(pkf_lookup_claims));
    uint64_t* point = (uint64_t*)malloc(32 * (size_t)(lookup ? ls.n : st.n));  // exactly n coordinates
    uint64_t* scalars = (uint64_t*)malloc(128);                                 // P, Q, cp, cq
    asan_case::run_proofs<pkv_result>(d, [&](const uint8_t* pattern, size_t pattern_len, const uint64_t* bind, const uint64_t*, const uint8_t* proof, size_t len,
                                             int* side, unsigned* layer, pkv_result* r) {
        if (lookup) return pkf_lookup_verify(&ls, pattern, pattern_len, bind, proof, len, claims, side, layer, r);
        return pkf_verify(&st, pattern, pattern_len, bind, nullptr, proof, len, scalars, point, scalars + 8, scalars + 12, layer, r);
    });
    free(scalars), free(point), free(claims);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "verify")) return run(argv[2], false);
    if (argc == 3 && !strcmp(argv[1], "lookup")) return run(argv[2], true);
    fprintf(stderr, "usage: pkf_verify_asan verify|lookup <case file>\n");
    return 2;
}
