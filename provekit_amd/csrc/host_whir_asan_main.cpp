// host_whir_asan_main.cpp -- driver of the sanitizer build of host_whir.hpp (make asan; CPU code only):
//   pk_host_whir_asan
//     checks every function of host_whir.hpp against a naive restatement -- the codeword as direct Horner evaluations at the domain
//     points the device layout prescribes, the tree by plain recursion, the opening by walking up from the leaf, the grinder against a
//     linear scan that also confirms no smaller nonce is valid, every product through the other host multiplier (h_mul, the 29-bit
//     one) -- at n = 4, 5, 6, 8 variables, fold 4, rate 1/2 (2, 4, 8, 32 leaves), batch 1 and
//     2, the round shape (n = 4, rate 1/16), both hash versions, entries drawn from 0, 1, p - 1 and random values, grinding at 0, 1, 4, 6
//     and 8 bits, and index lists with repeats and with every leaf opened.
//     Every table lives in a heap block of exactly its size, so that a read or write past an end is a report.
//     Prints one line per group of checks; exit 1 at the first group with a difference.
#include <cstdio>
#include <cstdlib>

#include "host_whir.hpp"

namespace {

using namespace pk;
namespace hw = pk::host_whir;

uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
uint64_t next_u64() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
fe p_minus_1() {
    fe r;
    for (int i = 0; i < 8; i++) r.v[i] = kPlimb(i);
    r.v[0] -= 1;
    return r;
}
fe random_fe() {
    fe r;
    for (int i = 0; i < 8; i += 2) {
        const uint64_t x = next_u64();
        r.v[i] = (u32)x;
        r.v[i + 1] = (u32)(x >> 32);
    }
    return fe_reduce_any(r);
}
// kind 0, 1, 2: every entry 0, 1, p - 1; 3: random; 4: a random mix of all four
fe draw(int kind) {
    if (kind == 4) kind = (int)(next_u64() & 3);
    return kind == 0 ? fe_zero() : kind == 1 ? fe_one() : kind == 2 ? p_minus_1() : random_fe();
}
std::vector<fe> table(size_t n, int kind) {
    std::vector<fe> t(n);
    for (auto& x : t) x = draw(kind);
    return t;
}

int failures = 0;
void expect(const fe& got, const fe& want, const char* what, size_t a, int b, int c) {
    if (fe_eq(got, want)) return;
    if (failures < 20) printf("MISMATCH %s %zu %d %d\n", what, a, b, c);
    failures++;
}

fe horner_naive(const fe* c, size_t n, const fe& z) {  // sum_i c[i] z^i with the powers multiplied up
    fe acc = fe_zero(), zp = fe_one();
    for (size_t i = 0; i < n; i++) {
        acc = h_add(acc, h_mul(c[i], zp));
        zp = h_mul(zp, z);
    }
    return acc;
}
fe root_naive(int version, const std::vector<fe>& digests, size_t lo, size_t n) {  // the tree over digests[lo, lo + n) by plain recursion
    if (n == 1) return digests[lo];
    return hw::compress(version, root_naive(version, digests, lo, n / 2), root_naive(version, digests, lo + n / 2, n / 2));
}

struct Shape {
    unsigned n_vars, log_inv_rate, fold, batch;
};
const Shape SHAPES[] = {{4, 1, 4, 1}, {4, 1, 4, 2}, {5, 1, 4, 1}, {5, 1, 4, 2}, {6, 1, 4, 1}, {6, 1, 4, 2}, {8, 1, 4, 1}, {8, 1, 4, 2}, {4, 4, 4, 1}};

void check_commit_and_open() {
    for (const Shape& s : SHAPES)
        for (int kind = 0; kind < 5; kind++)
            for (int version = 1; version <= 2; version++) {
                if (version == 1 && kind != 4) continue;  // the other hash once per shape
                const size_t N = (size_t)1 << s.n_vars, fw = (size_t)1 << s.fold, width = (size_t)s.batch << s.fold;
                const unsigned log_rows = s.n_vars + s.log_inv_rate - s.fold;
                const size_t rows = (size_t)1 << log_rows;
                std::vector<std::vector<fe>> polys;
                const fe* ptrs[2];
                for (unsigned b = 0; b < s.batch; b++) {
                    polys.push_back(table(N, kind));
                    ptrs[b] = polys[b].data();
                }
                std::vector<fe> leaves(rows * width), nodes(2 * rows);
                hw::commit(version, ptrs, s.batch, s.n_vars, s.log_inv_rate, s.fold, leaves.data(), nodes.data());
                // the codeword: leaf_i[b 2^k + j] = the stride-2^k sub-sequence j of polynomial b at w^i
                const fe w = domain_generator(log_rows);
                fe wi = fe_one();
                std::vector<fe> digests(rows);
                for (size_t i = 0; i < rows; i++, wi = h_mul(wi, w)) {
                    fe h = fe_zero();
                    for (size_t col = 0; col < width; col++) {
                        const size_t b = col / fw, j = col % fw;
                        std::vector<fe> sub(N / fw);
                        for (size_t t = 0; t < N / fw; t++) sub[t] = polys[b][fw * t + j];
                        const fe want = horner_naive(sub.data(), sub.size(), wi);
                        expect(leaves[col * rows + i], want, "codeword", rows, kind, (int)col);
                        h = col ? hw::compress(version, h, h_to_canon(want)) : h_to_canon(want);
                    }
                    digests[i] = h;
                    expect(nodes[rows + i], h, "leaf digest", rows, kind, (int)i);
                }
                expect(nodes[1], root_naive(version, digests, 0, rows), "root", rows, kind, version);
                expect(nodes[0], fe_zero(), "heap slot 0", rows, kind, version);
                for (size_t i = 1; i < rows; i++) expect(nodes[i], hw::compress(version, nodes[2 * i], nodes[2 * i + 1]), "inner node", rows, kind, (int)i);
                // openings: every leaf, and a list with repeats
                std::vector<uint64_t> all(rows), rep;
                for (size_t i = 0; i < rows; i++) all[i] = i;
                for (size_t q = 0; q < 7; q++) rep.push_back(next_u64() % rows), rep.push_back(rep.back());
                for (const std::vector<uint64_t>& idx : {all, rep}) {
                    const size_t k = idx.size(), plen = log_rows ? log_rows - 1 : 0;
                    std::vector<fe> ol(k * width), os(log_rows ? k : 0), op(k * plen);
                    hw::open(leaves.data(), nodes.data(), rows, width, idx.data(), k, ol.data(), os.data(), op.data());
                    for (size_t q = 0; q < k; q++) {
                        // the leaf, its sibling and its path lead to the root, as the verifier walks them
                        fe h = ol[q * width];
                        for (size_t j = 0; j < width; j++) expect(ol[q * width + j], h_to_canon(leaves[j * rows + idx[q]]), "opened leaf", rows, kind, (int)q);
                        for (size_t j = 1; j < width; j++) h = hw::compress(version, h, ol[q * width + j]);
                        uint64_t i = idx[q];
                        h = (i & 1) ? hw::compress(version, os[q], h) : hw::compress(version, h, os[q]);
                        i >>= 1;
                        for (size_t d = plen; d-- > 0;) {
                            const fe& node = op[q * plen + d];
                            h = (i & 1) ? hw::compress(version, node, h) : hw::compress(version, h, node);
                            i >>= 1;
                        }
                        expect(h, nodes[1], "opening reaches the root", rows, kind, (int)q);
                    }
                }
            }
    {  // a single leaf: the digest is the root
        const std::vector<fe> c = table(16, 3);
        const fe* ptrs[1] = {c.data()};
        std::vector<fe> leaves(16), nodes(2);
        hw::commit(2, ptrs, 1, 4, 0, 4, leaves.data(), nodes.data());
        fe h = h_to_canon(c[0]);
        for (size_t j = 1; j < 16; j++) h = hw::compress(2, h, h_to_canon(c[j]));
        expect(nodes[1], h, "one leaf", 1, 3, 0);
    }
    // compress against the transcript's permutation and the 29-bit path
    for (int kind = 0; kind < 4; kind++)
        for (int k2 = 0; k2 < 4; k2++) {
            const fe l = h_to_canon(draw(kind)), r = h_to_canon(draw(k2));
            expect(hw::compress(2, l, r), pack29(compress29<2, true>(unpack_reduce29(l), unpack_reduce29(r))), "compress v2", 0, kind, k2);
        }
    printf("commitments and openings ok\n");
}

void check_fold_and_horner() {
    for (unsigned n : {4u, 5u, 8u})
        for (unsigned k : {1u, 4u})
            for (int kind = 0; kind < 5; kind++) {
                const size_t N = (size_t)1 << n, fw = (size_t)1 << k;
                const std::vector<fe> c = table(N, kind), r = table(k, kind == 0 ? 3 : kind);
                std::vector<fe> out(N >> k);
                hw::fold_coeffs(c.data(), n, r.data(), k, out.data());
                for (size_t t = 0; t < (N >> k); t++) {
                    fe want = fe_zero();
                    for (size_t j = 0; j < fw; j++) {
                        fe w = fe_one();
                        for (unsigned b = 0; b < k; b++)
                            if ((j >> b) & 1) w = h_mul(w, r[b]);
                        want = h_add(want, h_mul(c[t * fw + j], w));
                    }
                    expect(out[t], want, "fold_coeffs", N, kind, (int)t);
                }
                const fe z = draw(kind);
                expect(hw::horner(c.data(), N, z), horner_naive(c.data(), N, z), "horner", N, kind, 0);
            }
    expect(hw::horner(nullptr, 0, fe_one()), fe_zero(), "horner of nothing", 0, 0, 0);
    printf("folds and evaluations ok\n");
}

void check_grinder() {
    for (double bits : {0.0, 1.0, 4.0, 6.0, 8.0})
        for (int c = 0; c < 3; c++) {
            uint8_t ch[32];
            for (int i = 0; i < 32; i += 8) {
                const uint64_t x = c == 0 && i == 24 ? ~0ull : next_u64();  // once a challenge above p
                memcpy(ch + i, &x, 8);
            }
            const uint64_t got = hw::pow_grind(ch, bits);
            if (bits == 0.0) {
                if (got != 0) printf("MISMATCH grinder at 0 bits\n"), failures++;
                continue;
            }
            // the linear scan, through the verifier's form of the check: no smaller nonce is valid, this one is
            uint64_t thr[4];
            pow_threshold(bits + 0.01, thr);
            fe t;
            memcpy(t.v, thr, 32);
            for (uint64_t nonce = 0; nonce <= got; nonce++) {
                fe nn = fe_zero();
                nn.v[0] = (u32)nonce;
                nn.v[1] = (u32)(nonce >> 32);
                const bool ok = fe_lt(hw::compress(2, load_raw(ch), nn), t);
                if (ok != (nonce == got)) {
                    printf("MISMATCH grinder bits %.0f nonce %llu of %llu\n", bits, (unsigned long long)nonce, (unsigned long long)got);
                    failures++;
                    break;
                }
            }
        }
    printf("grinder ok\n");
}

}  // namespace

int main() {
    check_commit_and_open();
    check_fold_and_horner();
    check_grinder();
    if (failures) {
        printf("%d differences\n", failures);
        return 1;
    }
    printf("host whir ok\n");
    return 0;
}
