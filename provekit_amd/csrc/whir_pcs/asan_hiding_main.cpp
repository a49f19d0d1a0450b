// asan_hiding_main.cpp -- driver of the sanitizer build of pkw_verify_hiding (make asan; CPU code only): reads one case file, verifies
// every proof in it at the case's q points, then the first proof under every further point count, and prints
// "rc accepted check offset" per call.  tests/test_whir_pcs_hiding_host.py writes the file:
//   u32 hash_version, q, 0, 0 | pk_whir_config | u32 pattern length | pattern | q * (n_vars - 1) points |
//   u32 n_proofs | n_proofs x (u64 length | bytes) | u32 n_counts | n_counts x u32 q'
// Points, proofs and outputs live in exact-size heap blocks, so that a read or write past an end is a report; a count the library
// must refuse before it reads a point (0, above PKW_MAX_POINTS) comes with a block of ONE point.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../include/provekit_whir_hiding.h"

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
        if (n) memcpy(dst, buf.data() + i, n);
        i += n;
    };
    uint32_t head[4], plen, n_proofs, n_counts;
    pk_whir_config cfg;
    take(head, sizeof head);
    take(&cfg, sizeof cfg);
    const uint32_t q = head[1];
    if (cfg.n_vars < 2 || cfg.n_vars > 16 || cfg.batch_size < 1 || cfg.batch_size > 4 || q < 1 || q > PKW_MAX_POINTS) return 2;
    const size_t n = cfg.n_vars - 1, rows = cfg.batch_size - 1;
    take(&plen, 4);
    if (buf.size() - i < plen) return 2;
    const std::vector<uint8_t> pattern(buf.begin() + i, buf.begin() + i + plen);
    i += plen;
    std::vector<uint64_t> points(4 * (size_t)q * n);
    take(points.data(), 32 * (size_t)q * n);
    take(&n_proofs, 4);
    std::vector<std::pair<uint8_t*, uint64_t>> proofs;
    for (uint32_t c = 0; c < n_proofs; c++) {
        uint64_t len;
        take(&len, 8);
        if (buf.size() - i < len) return 2;
        uint8_t* p = (uint8_t*)malloc(len ? len : 1);
        take(p, len);
        proofs.push_back({p, len});
    }
    take(&n_counts, 4);
    std::vector<uint32_t> counts(n_counts);
    take(counts.data(), 4 * (size_t)n_counts);
    if (proofs.empty()) return 2;
    auto run = [&](uint32_t count, const std::pair<uint8_t*, uint64_t>& proof) {
        const size_t held = count >= 1 && count <= PKW_MAX_POINTS ? count : 1;  // what the library may read and write for this count
        uint64_t* pts = (uint64_t*)malloc(32 * held * n);
        for (size_t k = 0; k < 4 * held * n; k++) pts[k] = points[k % points.size()];
        uint64_t* evals = (uint64_t*)malloc(rows ? 32 * held * rows : 1);
        pkv_result r;
        memset(&r, 0, sizeof r);
        const int rc = pkw_verify_hiding(&cfg, pattern.data(), pattern.size(), (int)head[0], nullptr, pts, count, proof.first, proof.second, evals, &r);
        if (rc)
            printf("%d 0 REFUSED 0 %s\n", rc, pkw_create_error());
        else
            printf("0 %d %s %llu\n", r.accepted, pkw_check_name(r.check), (unsigned long long)r.offset);
        free(pts);
        free(evals);
    };
    for (const auto& p : proofs) run(q, p);
    for (uint32_t c : counts) run(c, proofs[0]);
    for (auto& p : proofs) free(p.first);
    return 0;
}
