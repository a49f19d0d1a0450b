// asan_main.cpp -- driver of the sanitizer build of this library's host verifier (make asan; CPU code only): reads one case file,
// verifies every proof in it with pkw_verify_linear and prints "accepted check offset unchecked" per proof.
// tests/test_whir_pcs_linear_host.py writes the file:
//   u32 hash_version, q, l, with_weights | pk_whir_config | u32 pattern length | pattern | q * n_vars points | l tags |
//   with_weights ? l tables of 2^n_vars elements | u32 n_cases | n_cases x (u64 length | bytes)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../include/provekit_whir.h"

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
    uint32_t head[4], plen, n_cases;
    pk_whir_config cfg;
    take(head, sizeof head);
    take(&cfg, sizeof cfg);
    const uint32_t q = head[1], l = head[2];
    if (cfg.n_vars > 16 || q > PKW_MAX_POINTS || l > PKW_MAX_WEIGHTS) return 2;
    take(&plen, 4);
    if (buf.size() - i < plen) return 2;
    const std::vector<uint8_t> pattern(buf.begin() + i, buf.begin() + i + plen);
    i += plen;
    const size_t N = (size_t)1 << cfg.n_vars;
    std::vector<uint64_t> points(4 * (size_t)q * cfg.n_vars + 4), tags(4 * (size_t)l + 4);
    take(points.data(), 32 * (size_t)q * cfg.n_vars);
    take(tags.data(), 32 * (size_t)l);
    std::vector<std::vector<uint64_t>> tables(head[3] ? l : 0, std::vector<uint64_t>(4 * N));  // exact-size heap blocks
    std::vector<const uint64_t*> weights;
    for (auto& t : tables) {
        take(t.data(), 32 * N);
        weights.push_back(t.data());
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
        std::vector<uint64_t> evals(4 * (size_t)q * cfg.batch_size + 4), sums(4 * (size_t)l * cfg.batch_size + 4), fold(4 * (size_t)cfg.n_vars + 4), def(4 * l + 4);
        unsigned unchecked = 0;
        pkv_result r;
        if (int rc = pkw_verify_linear(&cfg, pattern.data(), pattern.size(), (int)head[0], nullptr, points.data(), q, tags.data(),
                                       weights.empty() ? nullptr : weights.data(), l, proof, len, evals.data(), sums.data(), fold.data(), def.data(), &unchecked,
                                       &r)) {
            fprintf(stderr, "pkw_verify_linear: %d %s\n", rc, pkw_create_error());
            return 4;
        }
        printf("%d %s %llu %u\n", r.accepted, pkw_check_name(r.check), (unsigned long long)r.offset, unchecked);
        free(proof);
    }
    return 0;
}
