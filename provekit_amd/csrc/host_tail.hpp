// host_tail.hpp -- the prover's sumchecks and weights over tables of a few hundred elements, on the host thread.
//
// A sumcheck round over 2^8 pairs is about a thousand field products; on the device it is a launch, a synchronisation and a transcript
// step, and every later round is half of the one before.  Once the tables are short (pk_selftest_set_host_tail) prover.hip brings them over
// once and finishes here: the rounds, the closing fold, the equality weights that join w between the rounds of a WHIR opening, and the
// dot products of a statement that small.  Every function restates a kernel of mle.hip over host memory and returns the canonical
// (fully reduced, Montgomery) values that kernel leaves -- field sums are exact, so the order in which they are taken does not show.
//
// Host only: the field layer of transcript.hpp / protocol.hpp and nothing of the runtime.  Products that are stored go through the
// 64-bit Montgomery multiplier (host64::mont_mul); products that are only summed are accumulated as 512-bit integers and reduced once
// per 16 terms (Sum), half the multiplications of a reduced product each.
#pragma once
#include <vector>

#include "protocol.hpp"

namespace pk {
namespace host_tail {

inline fe mul(const fe& a, const fe& b) {
    uint64_t x[4], y[4], r[4];
    memcpy(x, a.v, 32);
    memcpy(y, b.v, 32);
    host64::mont_mul(x, y, r);
    fe o;
    memcpy(o.v, r, 32);
    return o;
}
inline fe fold(const fe& x0, const fe& x1, const fe& r) { return h_add(x0, mul(r, h_sub(x1, x0))); }  // x0 + r (x1 - x0)

// sum_j a_j b_j of reduced operands: the raw products are added up in 8 limbs and Montgomery-reduced once per GROUP terms.
// 16 p^2 + 2^256 p < 2^512 (p < 0.19 * 2^256), so neither the sum nor the reduction's additions leave the 8 limbs, and the reduced
// group is below 16 p^2 / 2^256 + p < 4.1 p < 2^256: a few subtractions of p make it canonical.
class Sum {
  public:
    static constexpr unsigned GROUP = 16;
    void add(const fe& a, const fe& b) {
        using host64::u128;
        uint64_t x[4], y[4];
        memcpy(x, a.v, 32);
        memcpy(y, b.v, 32);
        for (int i = 0; i < 4; i++) {
            u128 c = 0;
            for (int j = 0; j < 4; j++) {
                c += (u128)x[j] * y[i] + t_[i + j];
                t_[i + j] = (uint64_t)c;
                c >>= 64;
            }
            for (int k = i + 4; k < 8 && c; k++) {
                c += t_[k];
                t_[k] = (uint64_t)c;
                c >>= 64;
            }
        }
        if (++n_ == GROUP) flush();
    }
    fe value() {
        flush();
        return total_;
    }

  private:
    uint64_t t_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned n_ = 0;
    fe total_ = fe_zero();
    void flush() {
        using namespace host64;
        if (!n_) return;
        for (int i = 0; i < 4; i++) {
            const uint64_t m = t_[i] * NP64;
            u128 c = 0;
            for (int j = 0; j < 4; j++) {
                c += (u128)m * P64[j] + t_[i + j];
                t_[i + j] = (uint64_t)c;
                c >>= 64;
            }
            for (int k = i + 4; k < 8 && c; k++) {
                c += t_[k];
                t_[k] = (uint64_t)c;
                c >>= 64;
            }
        }
        while (geq_p(t_ + 4)) sub_p(t_ + 4);
        fe r;
        memcpy(r.v, t_ + 4, 32);
        total_ = h_add(total_, r);
        memset(t_, 0, sizeof t_);
        n_ = 0;
    }
};

// ---- the folds ------------------------------------------------------------------------------------------------------------------
// adjacent pairs, the WHIR sumcheck's order (fold_pairs_kernel): v[i] = v[2i] + r (v[2i+1] - v[2i]), len -> len / 2 (len even)
inline void fold_pairs(fe* v, size_t len, const fe& r) {
    for (size_t i = 0; i < len / 2; i++) v[i] = fold(v[2 * i], v[2 * i + 1], r);
}
// halves, the Spartan sumcheck's order (sumcheck.rs:95-96): v[i] = v[i] + r (v[i + len/2] - v[i]), len -> len / 2 (len even)
inline void fold_halves(fe* v, size_t len, const fe& r) {
    for (size_t i = 0; i < len / 2; i++) v[i] = fold(v[i], v[i + len / 2], r);
}

// ---- quadratic round (sumcheck_quadratic_launch): p, w of `len` entries, a power of two.  r != null: first both are folded in place
// by r (adjacent pairs), len -> len / 2.  Then over the pairs (2i, 2i+1) of what stands: h(0) = sum p0 w0, h(1) = sum p1 w1,
// h(2) = sum (2 p1 - p0)(2 w1 - w0); out = h(0), h(1), h(2) (nsums 3) or h(0), h(2) (nsums 2).  Returns the length p, w have afterwards.
inline size_t quadratic_round(fe* p, fe* w, size_t len, const fe* r, int nsums, uint64_t out[12]) {
    if (r) {
        fold_pairs(p, len, *r);
        fold_pairs(w, len, *r);
        len /= 2;
    }
    Sum h0, h1, h2;
    for (size_t i = 0; i + 1 < len; i += 2) {
        const fe &p0 = p[i], &p1 = p[i + 1], &w0 = w[i], &w1 = w[i + 1];
        h0.add(p0, w0);
        if (nsums == 3) h1.add(p1, w1);
        h2.add(h_sub(h_add(p1, p1), p0), h_sub(h_add(w1, w1), w0));
    }
    h_store(out, h0.value());
    if (nsums == 3) h_store(out + 4, h1.value());
    h_store(out + 4 * (nsums - 1), h2.value());
    return len;
}

// ---- cubic round, CubicWeight::Level (sumcheck_cubic_launch): a, b, c of `len` entries, a power of two; E = the level of the suffix
// equality tables of the round evaluated, one entry per pair.  r != null: first a, b, c are folded in place by r (halves), len -> len / 2.
// Then over the pairs (i, i + len/2) of what stands: out = Q(0) = sum E (a0 b0 - c0), Q(-1) = sum E ((2a0-a1)(2b0-b1) - (2c0-c1)),
// Q_inf = sum E (a1-a0)(b1-b0).  Returns the length a, b, c have afterwards.
inline size_t cubic_round(fe* a, fe* b, fe* c, const fe* E, size_t len, const fe* r, uint64_t out[12]) {
    if (r) {
        fold_halves(a, len, *r);
        fold_halves(b, len, *r);
        fold_halves(c, len, *r);
        len /= 2;
    }
    Sum q0, qm, qi;
    const size_t h = len / 2;
    for (size_t i = 0; i < h; i++) {
        const fe &a0 = a[i], &a1 = a[i + h], &b0 = b[i], &b1 = b[i + h], &c0 = c[i], &c1 = c[i + h];
        q0.add(E[i], h_sub(mul(a0, b0), c0));
        const fe ta = h_sub(h_add(a0, a0), a1), tb = h_sub(h_add(b0, b0), b1), tc = h_sub(h_add(c0, c0), c1);
        qm.add(E[i], h_sub(mul(ta, tb), tc));
        qi.add(E[i], mul(h_sub(a1, a0), h_sub(b1, b0)));
    }
    h_store(out, q0.value());
    h_store(out + 4, qm.value());
    h_store(out + 8, qi.value());
    return len;
}

// ---- equality tables ------------------------------------------------------------------------------------------------------------
// T[i] = first * eq(x[0 .. nv), i), i < 2^nv, variable 0 <-> the most significant index bit (eval_eq's order, sumcheck.rs:146-171):
// level by level as eq_half_tables_kernel, the last variable first
inline void eq_table(const fe* x, unsigned nv, const fe& first, fe* T) {
    T[0] = first;
    for (unsigned l = 0; l < nv; l++) {
        const size_t h = (size_t)1 << l;
        const fe& xv = x[nv - 1 - l];
        for (size_t i = 0; i < h; i++) {
            const fe up = mul(T[i], xv);
            T[h + i] = up;
            T[i] = h_sub(T[i], up);
        }
    }
}
// eq(x, i) = hi[i >> nlo] * lo[i & (2^nlo - 1)]: the two half tables of a point, the scale in the high one
struct HalfTables {
    unsigned nhi, nlo;
    std::vector<fe> t;  // per point: 2^nhi high entries, then 2^nlo low entries
    size_t per_pt() const { return ((size_t)1 << nhi) + ((size_t)1 << nlo); }
    const fe* hi(size_t j) const { return t.data() + j * per_pt(); }
    const fe* lo(size_t j) const { return hi(j) + ((size_t)1 << nhi); }
    HalfTables(const fe* points, const fe* scales, unsigned n_vars, size_t q) : nhi(n_vars / 2), nlo(n_vars - n_vars / 2) {
        t.resize((q ? q : 1) * per_pt());
        for (size_t j = 0; j < q; j++) {
            const fe* x = points + j * n_vars;
            eq_table(x, nhi, scales ? scales[j] : fe_one(), t.data() + j * per_pt());
            eq_table(x + nhi, nlo, fe_one(), t.data() + j * per_pt() + ((size_t)1 << nhi));
        }
    }
};
// pk_eq_accumulate: w[i] = (overwrite ? 0 : w[i]) + sum_j scales[j] eq(points[j], i) over the 2^n_vars entries of w; points = q x n_vars
inline void eq_accumulate(fe* w, unsigned n_vars, const fe* points, const fe* scales, size_t q, bool overwrite) {
    const HalfTables H(points, scales, n_vars, q);
    const size_t n = (size_t)1 << n_vars, mask = ((size_t)1 << H.nlo) - 1;
    for (size_t i = 0; i < n; i++) {
        Sum s;
        for (size_t j = 0; j < q; j++) s.add(H.hi(j)[i >> H.nlo], H.lo(j)[i & mask]);
        w[i] = overwrite ? s.value() : h_add(w[i], s.value());
    }
}

// ---- dot products ---------------------------------------------------------------------------------------------------------------
// pk_dot2: out = <w, f>, <w, g> over n entries
inline void dot2(const fe* w, const fe* f, const fe* g, size_t n, uint64_t out[8]) {
    Sum sf, sg;
    for (size_t i = 0; i < n; i++) {
        sf.add(w[i], f[i]);
        sg.add(w[i], g[i]);
    }
    h_store(out, sf.value());
    h_store(out + 4, sg.value());
}
// dot_rows_eq: out[4 k] = <row k, eq(point, .)> over the rows' first n <= 2^n_vars entries, row k at rows + k * stride; the table's
// entries are formed from the point's half tables as they are met
inline void dot_rows_eq(const fe* rows, size_t stride, unsigned nrows, const fe* point, unsigned n_vars, size_t n, uint64_t* out) {
    const HalfTables H(point, nullptr, n_vars, 1);
    const size_t mask = ((size_t)1 << H.nlo) - 1;
    std::vector<Sum> s(nrows);
    for (size_t i = 0; i < n; i++) {
        const fe e = mul(H.hi(0)[i >> H.nlo], H.lo(0)[i & mask]);
        for (unsigned k = 0; k < nrows; k++) s[k].add(rows[k * stride + i], e);
    }
    for (unsigned k = 0; k < nrows; k++) h_store(out + 4 * k, s[k].value());
}

// ---- what forms the tables of an opening that starts here -------------------------------------------------------------------------
inline void lincomb2(fe* out, const fe* a, const fe& beta, const fe* b, size_t n) {  // out = a + beta b
    for (size_t i = 0; i < n; i++) out[i] = h_add(a[i], mul(beta, b[i]));
}
inline void axpy(fe* y, const fe& g, const fe* x, size_t n) {  // y += g x
    for (size_t i = 0; i < n; i++) y[i] = h_add(y[i], mul(g, x[i]));
}

}  // namespace host_tail
}  // namespace pk
