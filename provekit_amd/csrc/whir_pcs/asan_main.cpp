// asan_main.cpp -- driver of the sanitizer build of this library's host verifier (make asan; CPU code only):
//   pkw_verify_asan <linear|sparse|hiding> <case file>
// reads one case file and verifies the proofs in it with pkw_verify_linear, pkw_verify_sparse or pkw_verify_hiding.  Every file begins
//   u32 hash_version, q, l, with_weights | pk_whir_config | u32 pattern length | pattern
// and goes on as its mode says below; a list of proofs is u32 count | count x (u64 length | bytes).  Proofs, and whatever else a mode
// names, live in exact-size heap blocks, so that a read or write past an end is a report, not a read of the next item.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/provekit_whir.h"
#include "../../../include/provekit_whir_hiding.h"
#include "../../../include/provekit_whir_sparse.h"

namespace {

std::vector<uint8_t> buf;  // the case file
size_t at = 0;

void take(void* dst, size_t n) {
    if (buf.size() - at < n) exit(2);
    if (n) memcpy(dst, buf.data() + at, n);
    at += n;
}
void* take_block(size_t n) {  // the next n bytes in a heap block of exactly that size
    if (buf.size() - at < n) exit(2);
    void* p = malloc(n ? n : 1);
    take(p, n);
    return p;
}

struct Proof {
    uint8_t* bytes;
    uint64_t len;
};
std::vector<Proof> take_proofs() {
    uint32_t count;
    take(&count, 4);
    std::vector<Proof> proofs;
    for (uint32_t c = 0; c < count; c++) {
        uint64_t len;
        take(&len, 8);
        proofs.push_back({(uint8_t*)take_block(len), len});
    }
    return proofs;
}

// the head of every file
uint32_t head[4];
pk_whir_config cfg;
std::vector<uint8_t> pattern;

void print_verdict(int rc, const pkv_result& r) {  // "rc accepted check offset" per call
    if (rc)
        printf("%d 0 REFUSED 0 %s\n", rc, pkw_create_error());
    else
        printf("0 %d %s %llu\n", r.accepted, pkw_check_name(r.check), (unsigned long long)r.offset);
}

// what a linear or sparse verification writes
struct Outputs {
    std::vector<uint64_t> evals, sums, fold, def;
    Outputs(uint32_t q, uint32_t l)
        : evals(4 * (size_t)q * cfg.batch_size + 4), sums(4 * (size_t)l * cfg.batch_size + 4), fold(4 * (size_t)cfg.n_vars + 4), def(4 * l + 4) {}
};

// tests/test_whir_pcs_linear_host.py:  q * n_vars points | l tags | with_weights ? l tables of 2^n_vars elements | proofs.
// Prints "accepted check offset unchecked" per proof
int linear() {
    const uint32_t q = head[1], l = head[2];
    if (cfg.n_vars > 16 || q > PKW_MAX_POINTS || l > PKW_MAX_WEIGHTS) return 2;
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
    for (const Proof& p : take_proofs()) {
        Outputs o(q, l);
        unsigned unchecked = 0;
        pkv_result r;
        if (int rc = pkw_verify_linear(&cfg, pattern.data(), pattern.size(), (int)head[0], nullptr, points.data(), q, tags.data(),
                                       weights.empty() ? nullptr : weights.data(), l, p.bytes, p.len, o.evals.data(), o.sums.data(), o.fold.data(),
                                       o.def.data(), &unchecked, &r)) {
            fprintf(stderr, "pkw_verify_linear: %d %s\n", rc, pkw_create_error());
            return 4;
        }
        printf("%d %s %llu %u\n", r.accepted, pkw_check_name(r.check), (unsigned long long)r.offset, unchecked);
        free(p.bytes);
    }
    return 0;
}

// tests/test_whir_pcs_sparse_host.py:  q * n_vars points | l tags | proofs |
//   u32 n_lists | n_lists x ((l + 1) u64 offsets | u64 n_index | n_index u32 | u64 n_value | n_value elements)
// Every proof against the first weight lists, then the first proof against every further lists; index and value lists in exact-size
// blocks
int sparse() {
    struct Lists {
        std::vector<uint64_t> offsets;
        uint32_t* index;
        uint64_t* value;
    };
    const uint32_t q = head[1], l = head[2];
    if (cfg.n_vars > 16 || q > PKW_MAX_POINTS || l > PKW_MAX_WEIGHTS) return 2;
    std::vector<uint64_t> points(4 * (size_t)q * cfg.n_vars + 4), tags(4 * (size_t)l + 4);
    take(points.data(), 32 * (size_t)q * cfg.n_vars);
    take(tags.data(), 32 * (size_t)l);
    const std::vector<Proof> proofs = take_proofs();
    uint32_t n_lists;
    take(&n_lists, 4);
    std::vector<Lists> lists(n_lists);
    for (Lists& w : lists) {
        uint64_t n_index, n_value;
        w.offsets.resize(l + 1);
        take(w.offsets.data(), 8 * (size_t)(l + 1));
        take(&n_index, 8);
        if (n_index > (1u << 24)) return 2;
        w.index = (uint32_t*)take_block(4 * n_index);
        take(&n_value, 8);
        if (n_value > (1u << 24)) return 2;
        w.value = (uint64_t*)take_block(32 * n_value);
    }
    if (proofs.empty() || lists.empty()) return 2;
    auto run = [&](const Lists& w, const Proof& p) {
        Outputs o(q, l);
        pkv_result r;
        memset(&r, 0, sizeof r);
        print_verdict(pkw_verify_sparse(&cfg, pattern.data(), pattern.size(), (int)head[0], nullptr, points.data(), q, tags.data(), w.offsets.data(), w.index,
                                        w.value, l, p.bytes, p.len, o.evals.data(), o.sums.data(), o.fold.data(), o.def.data(), &r),
                      r);
    };
    for (const Proof& p : proofs) run(lists[0], p);
    for (size_t k = 1; k < lists.size(); k++) run(lists[k], proofs[0]);
    for (const Proof& p : proofs) free(p.bytes);
    for (Lists& w : lists) {
        free(w.index);
        free(w.value);
    }
    return 0;
}

// tests/test_whir_pcs_hiding_host.py:  q * (n_vars - 1) points | proofs | u32 n_counts | n_counts x u32 q'
// Every proof at the case's q points, then the first proof under every further point count.  Points and outputs in exact-size blocks
// too; a count the library must refuse before it reads a point (0, above PKW_MAX_POINTS) comes with a block of ONE point
int hiding() {
    const uint32_t q = head[1];
    if (cfg.n_vars < 2 || cfg.n_vars > 16 || cfg.batch_size < 1 || cfg.batch_size > 4 || q < 1 || q > PKW_MAX_POINTS) return 2;
    const size_t n = cfg.n_vars - 1, rows = cfg.batch_size - 1;
    std::vector<uint64_t> points(4 * (size_t)q * n);
    take(points.data(), 32 * (size_t)q * n);
    const std::vector<Proof> proofs = take_proofs();
    uint32_t n_counts;
    take(&n_counts, 4);
    std::vector<uint32_t> counts(n_counts);
    take(counts.data(), 4 * (size_t)n_counts);
    if (proofs.empty()) return 2;
    auto run = [&](uint32_t count, const Proof& p) {
        const size_t held = count >= 1 && count <= PKW_MAX_POINTS ? count : 1;  // what the library may read and write for this count
        uint64_t* pts = (uint64_t*)malloc(32 * held * n);
        for (size_t k = 0; k < 4 * held * n; k++) pts[k] = points[k % points.size()];
        uint64_t* evals = (uint64_t*)malloc(rows ? 32 * held * rows : 1);
        pkv_result r;
        memset(&r, 0, sizeof r);
        print_verdict(pkw_verify_hiding(&cfg, pattern.data(), pattern.size(), (int)head[0], nullptr, pts, count, p.bytes, p.len, evals, &r), r);
        free(pts);
        free(evals);
    };
    for (const Proof& p : proofs) run(q, p);
    for (uint32_t c : counts) run(c, proofs[0]);
    for (const Proof& p : proofs) free(p.bytes);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const std::string mode = argv[1];
    if (mode != "linear" && mode != "sparse" && mode != "hiding") return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    uint8_t chunk[1 << 16];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) buf.insert(buf.end(), chunk, chunk + n);
    fclose(f);
    uint32_t plen;
    take(head, sizeof head);
    take(&cfg, sizeof cfg);
    take(&plen, 4);
    if (buf.size() - at < plen) return 2;
    pattern.resize(plen);
    take(pattern.data(), plen);
    return mode == "linear" ? linear() : mode == "sparse" ? sparse() : hiding();
}
