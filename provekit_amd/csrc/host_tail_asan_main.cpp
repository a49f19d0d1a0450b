// host_tail_asan_main.cpp -- driver of the sanitizer build of host_tail.hpp (make asan; CPU code only):
//   pk_host_tail_asan
//     checks every function of host_tail.hpp against a naive restatement -- direct sums over the pairs, eq by its product formula, every
//     product through the other host multiplier (h_mul, the 29-bit one) -- at lengths 1, 2, 3 (where a length may be odd), 4, 256 and
//     2^11, entries drawn from 0, 1, p - 1 and random values, challenges 0, 1, p - 1 and random, and 0, 1 and 110 points for the weights.
//     Every table lives in a heap block of exactly its size, so that a read or write past an end is a report.
//     Prints one line per group of checks; exit 1 at the first difference.
#include <cstdio>
#include <cstdlib>

#include "host_tail.hpp"

namespace {

using namespace pk;
namespace ht = pk::host_tail;

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
void expect(const fe& got, const fe& want, const char* what, size_t len, int kind, int aux) {
    if (fe_eq(got, want)) return;
    printf("MISMATCH %s len %zu kind %d aux %d\n", what, len, kind, aux);
    failures++;
}
void expect(const uint64_t* got, const fe& want, const char* what, size_t len, int kind, int aux) { expect(h_load(got), want, what, len, kind, aux); }

// eq(x, i) by its product formula, x_0 <-> the most significant of the nv index bits
fe eq_naive(const fe* x, unsigned nv, size_t i) {
    fe acc = fe_one();
    for (unsigned t = 0; t < nv; t++) acc = h_mul(acc, ((i >> (nv - 1 - t)) & 1) ? x[t] : h_sub(fe_one(), x[t]));
    return acc;
}
fe fold_naive(const fe& x0, const fe& x1, const fe& r) { return h_add(h_mul(h_sub(fe_one(), r), x0), h_mul(r, x1)); }  // (1 - r) x0 + r x1
fe two(const fe& x) { return h_add(x, x); }

const size_t ROUND_LENS[] = {2, 4, 256, 2048};
const size_t DOT_LENS[] = {1, 2, 3, 4, 256, 2048};

void check_quadratic() {
    for (size_t len : ROUND_LENS)
        for (int kind = 0; kind < 5; kind++)
            for (int ch = -1; ch < 4; ch++)       // -1: no fold
                for (int nsums = 2; nsums <= 3; nsums++) {
                    if (ch >= 0 && len < 4) continue;  // a pair must be left after the fold
                    std::vector<fe> p = table(len, kind), w = table(len, kind == 4 ? 4 : 3);
                    const fe r = draw(ch < 0 ? 0 : ch);
                    std::vector<fe> fp = p, fw = w;
                    if (ch >= 0) {
                        fp.resize(len / 2), fw.resize(len / 2);
                        for (size_t i = 0; i < len / 2; i++) fp[i] = fold_naive(p[2 * i], p[2 * i + 1], r), fw[i] = fold_naive(w[2 * i], w[2 * i + 1], r);
                    }
                    fe h[3] = {fe_zero(), fe_zero(), fe_zero()};
                    for (size_t i = 0; i + 1 < fp.size(); i += 2) {
                        h[0] = h_add(h[0], h_mul(fp[i], fw[i]));
                        h[1] = h_add(h[1], h_mul(fp[i + 1], fw[i + 1]));
                        h[2] = h_add(h[2], h_mul(h_sub(two(fp[i + 1]), fp[i]), h_sub(two(fw[i + 1]), fw[i])));
                    }
                    uint64_t out[12];
                    const size_t after = ht::quadratic_round(p.data(), w.data(), len, ch < 0 ? nullptr : &r, nsums, out);
                    if (after != fp.size()) printf("MISMATCH quadratic length %zu\n", len), failures++;
                    expect(out, h[0], "quadratic h(0)", len, kind, ch);
                    if (nsums == 3) expect(out + 4, h[1], "quadratic h(1)", len, kind, ch);
                    expect(out + 4 * (nsums - 1), h[2], "quadratic h(2)", len, kind, ch);
                    for (size_t i = 0; i < after; i++) expect(p[i], fp[i], "quadratic p", len, kind, ch), expect(w[i], fw[i], "quadratic w", len, kind, ch);
                }
    {  // a single entry has no pair: the sums are zero
        std::vector<fe> p = table(1, 3), w = table(1, 3);
        uint64_t out[12];
        ht::quadratic_round(p.data(), w.data(), 1, nullptr, 3, out);
        for (int q = 0; q < 3; q++) expect(out + 4 * q, fe_zero(), "quadratic, one entry", 1, 3, q);
    }
    for (size_t len : ROUND_LENS)  // the closing fold
        for (int ch = 0; ch < 4; ch++) {
            std::vector<fe> v = table(len, 4);
            const std::vector<fe> v0 = v;
            const fe r = draw(ch);
            ht::fold_pairs(v.data(), len, r);
            for (size_t i = 0; i < len / 2; i++) expect(v[i], fold_naive(v0[2 * i], v0[2 * i + 1], r), "fold_pairs", len, 4, ch);
        }
    printf("quadratic rounds ok\n");
}

void check_cubic() {
    for (size_t len : ROUND_LENS)
        for (int kind = 0; kind < 5; kind++)
            for (int ch = -1; ch < 4; ch++) {
                if (ch >= 0 && len < 4) continue;
                std::vector<fe> a = table(len, kind), b = table(len, kind == 4 ? 4 : 3), c = table(len, kind);
                const size_t after = ch < 0 ? len : len / 2;
                const std::vector<fe> E = table(after / 2, kind == 0 ? 3 : kind);
                const fe r = draw(ch < 0 ? 0 : ch);
                std::vector<fe> fa = a, fb = b, fc = c;
                if (ch >= 0) {
                    fa.resize(after), fb.resize(after), fc.resize(after);
                    for (size_t i = 0; i < after; i++)
                        fa[i] = fold_naive(a[i], a[i + after], r), fb[i] = fold_naive(b[i], b[i + after], r), fc[i] = fold_naive(c[i], c[i + after], r);
                }
                fe q[3] = {fe_zero(), fe_zero(), fe_zero()};
                const size_t h = after / 2;
                for (size_t i = 0; i < h; i++) {
                    q[0] = h_add(q[0], h_mul(E[i], h_sub(h_mul(fa[i], fb[i]), fc[i])));
                    const fe ta = h_sub(two(fa[i]), fa[i + h]), tb = h_sub(two(fb[i]), fb[i + h]), tc = h_sub(two(fc[i]), fc[i + h]);
                    q[1] = h_add(q[1], h_mul(E[i], h_sub(h_mul(ta, tb), tc)));
                    q[2] = h_add(q[2], h_mul(E[i], h_mul(h_sub(fa[i + h], fa[i]), h_sub(fb[i + h], fb[i]))));
                }
                uint64_t out[12];
                const size_t got = ht::cubic_round(a.data(), b.data(), c.data(), E.data(), len, ch < 0 ? nullptr : &r, out);
                if (got != after) printf("MISMATCH cubic length %zu\n", len), failures++;
                for (int s = 0; s < 3; s++) expect(out + 4 * s, q[s], "cubic sum", len, kind, 10 * ch + s);
                for (size_t i = 0; i < after; i++) expect(a[i], fa[i], "cubic a", len, kind, ch), expect(b[i], fb[i], "cubic b", len, kind, ch), expect(c[i], fc[i], "cubic c", len, kind, ch);
            }
    printf("cubic rounds ok\n");
}

void check_weights() {
    const unsigned VARS[] = {0, 1, 2, 8, 11};
    const size_t QS[] = {0, 1, 110};
    for (unsigned nv : VARS)
        for (size_t q : QS)
            for (int kind = 0; kind < 5; kind++)
                for (int overwrite = 0; overwrite < 2; overwrite++) {
                    if (q == 110 && (kind != 4 || (nv == 11 && overwrite))) continue;  // the long cases once: the naive side is q * 2^nv * nv products
                    const size_t n = (size_t)1 << nv;
                    const std::vector<fe> pts = table(q * nv, kind), scales = table(q, kind == 0 ? 3 : kind);
                    std::vector<fe> w = table(n, 4);
                    const std::vector<fe> w0 = w;
                    ht::eq_accumulate(w.data(), nv, pts.data(), scales.data(), q, overwrite != 0);
                    for (size_t i = 0; i < n; i++) {
                        fe want = overwrite ? fe_zero() : w0[i];
                        for (size_t j = 0; j < q; j++) want = h_add(want, h_mul(scales[j], eq_naive(pts.data() + j * nv, nv, i)));
                        expect(w[i], want, "eq_accumulate", n, kind, (int)q);
                    }
                }
    printf("equality weights ok\n");
}

void check_dots() {
    for (size_t n : DOT_LENS)
        for (int kind = 0; kind < 5; kind++) {
            const std::vector<fe> w = table(n, kind), f = table(n, kind == 4 ? 4 : 3), g = table(n, kind);
            uint64_t out[8];
            ht::dot2(w.data(), f.data(), g.data(), n, out);
            fe sf = fe_zero(), sg = fe_zero();
            for (size_t i = 0; i < n; i++) sf = h_add(sf, h_mul(w[i], f[i])), sg = h_add(sg, h_mul(w[i], g[i]));
            expect(out, sf, "dot2 f", n, kind, 0);
            expect(out + 4, sg, "dot2 g", n, kind, 0);
            unsigned nv = 0;
            while (((size_t)1 << nv) < n) nv++;
            for (unsigned extra = 0; extra < 2; extra++)  // the rows fill the hypercube, or its leading part only
                for (unsigned nrows = 1; nrows <= 3; nrows += 2) {
                    const unsigned vars = nv + extra;
                    const std::vector<fe> point = table(vars, kind == 0 ? 3 : kind), rows = table(nrows * n, kind);
                    uint64_t o[12];
                    ht::dot_rows_eq(rows.data(), n, nrows, point.data(), vars, n, o);
                    for (unsigned k = 0; k < nrows; k++) {
                        fe want = fe_zero();
                        for (size_t i = 0; i < n; i++) want = h_add(want, h_mul(rows[k * n + i], eq_naive(point.data(), vars, i)));
                        expect(o + 4 * k, want, "dot_rows_eq", n, kind, (int)(10 * vars + k));
                    }
                }
            std::vector<fe> y = table(n, 4);
            const std::vector<fe> y0 = y;
            std::vector<fe> lc(n);
            const fe beta = draw(kind);
            ht::lincomb2(lc.data(), f.data(), beta, g.data(), n);
            ht::axpy(y.data(), beta, w.data(), n);
            for (size_t i = 0; i < n; i++) {
                expect(lc[i], h_add(f[i], h_mul(beta, g[i])), "lincomb2", n, kind, 0);
                expect(y[i], h_add(y0[i], h_mul(beta, w[i])), "axpy", n, kind, 0);
            }
        }
    printf("dot products ok\n");
}

void check_sum_groups() {  // the accumulator at its bound: p - 1 squared, through several groups and a partial one
    const fe m1 = p_minus_1();
    for (unsigned n : {1u, 15u, 16u, 17u, 32u, 100u}) {
        ht::Sum s;
        fe want = fe_zero();
        for (unsigned i = 0; i < n; i++) s.add(m1, m1), want = h_add(want, h_mul(m1, m1));
        expect(s.value(), want, "Sum", n, 2, 0);
    }
    for (int kind = 0; kind < 4; kind++)
        for (int k2 = 0; k2 < 4; k2++) {
            const fe a = draw(kind), b = draw(k2);
            expect(ht::mul(a, b), h_mul(a, b), "mul", 1, kind, k2);
        }
    printf("accumulator ok\n");
}

}  // namespace

int main() {
    check_sum_groups();
    check_quadratic();
    check_cubic();
    check_weights();
    check_dots();
    if (failures) {
        printf("%d differences\n", failures);
        return 1;
    }
    printf("host tail ok\n");
    return 0;
}
