// asan_sparse_main.cpp -- driver of the sanitizer build of pkw_verify_sparse (make asan; CPU code only): reads one case file, verifies
// every proof in it against the first weight lists, then the first proof against every further lists, and prints
// "rc accepted check offset" per call.  tests/test_whir_pcs_sparse_host.py writes the file:
//   u32 hash_version, q, l, 0 | pk_whir_config | u32 pattern length | pattern | q * n_vars points | l tags |
//   u32 n_proofs | n_proofs x (u64 length | bytes) |
//   u32 n_lists | n_lists x ((l + 1) u64 offsets | u64 n_index | n_index u32 | u64 n_value | n_value elements)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../include/provekit_whir_sparse.h"

struct Lists {  // exact-size heap blocks, so that a read past a list's end is a report
    std::vector<uint64_t> offsets;
    uint32_t* index;
    uint64_t* value;
};

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
    uint32_t head[4], plen, n_proofs, n_lists;
    pk_whir_config cfg;
    take(head, sizeof head);
    take(&cfg, sizeof cfg);
    const uint32_t q = head[1], l = head[2];
    if (cfg.n_vars > 16 || q > PKW_MAX_POINTS || l > PKW_MAX_WEIGHTS) return 2;
    take(&plen, 4);
    if (buf.size() - i < plen) return 2;
    const std::vector<uint8_t> pattern(buf.begin() + i, buf.begin() + i + plen);
    i += plen;
    std::vector<uint64_t> points(4 * (size_t)q * cfg.n_vars + 4), tags(4 * (size_t)l + 4);
    take(points.data(), 32 * (size_t)q * cfg.n_vars);
    take(tags.data(), 32 * (size_t)l);
    take(&n_proofs, 4);
    std::vector<std::pair<uint8_t*, uint64_t>> proofs;
    for (uint32_t c = 0; c < n_proofs; c++) {
        uint64_t len;
        take(&len, 8);
        if (buf.size() - i < len) return 2;
        uint8_t* p = (uint8_t*)malloc(len ? len : 1);  // an exact-size heap copy: a read past the proof's end is a report
        take(p, len);
        proofs.push_back({p, len});
    }
    take(&n_lists, 4);
    std::vector<Lists> lists(n_lists);
    for (Lists& w : lists) {
        uint64_t n_index, n_value;
        w.offsets.resize(l + 1);
        take(w.offsets.data(), 8 * (size_t)(l + 1));
        take(&n_index, 8);
        if (n_index > (1u << 24)) return 2;
        w.index = (uint32_t*)malloc(n_index ? 4 * n_index : 1);
        take(w.index, 4 * n_index);
        take(&n_value, 8);
        if (n_value > (1u << 24)) return 2;
        w.value = (uint64_t*)malloc(n_value ? 32 * n_value : 1);
        take(w.value, 32 * n_value);
    }
    if (proofs.empty() || lists.empty()) return 2;
    auto run = [&](const Lists& w, const std::pair<uint8_t*, uint64_t>& proof) {
        std::vector<uint64_t> evals(4 * (size_t)q * cfg.batch_size + 4), sums(4 * (size_t)l * cfg.batch_size + 4), fold(4 * (size_t)cfg.n_vars + 4), def(4 * l + 4);
        pkv_result r;
        memset(&r, 0, sizeof r);
        const int rc = pkw_verify_sparse(&cfg, pattern.data(), pattern.size(), (int)head[0], nullptr, points.data(), q, tags.data(), w.offsets.data(), w.index,
                                         w.value, l, proof.first, proof.second, evals.data(), sums.data(), fold.data(), def.data(), &r);
        if (rc)
            printf("%d 0 REFUSED 0 %s\n", rc, pkw_create_error());
        else
            printf("0 %d %s %llu\n", r.accepted, pkw_check_name(r.check), (unsigned long long)r.offset);
    };
    for (const auto& p : proofs) run(lists[0], p);
    for (size_t k = 1; k < lists.size(); k++) run(lists[k], proofs[0]);
    for (auto& p : proofs) free(p.first);
    for (Lists& w : lists) {
        free(w.index);
        free(w.value);
    }
    return 0;
}
