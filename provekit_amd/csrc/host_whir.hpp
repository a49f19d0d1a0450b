// host_whir.hpp -- the device work of a WHIR commitment and opening over tables of a few hundred elements, on the host thread.
//
// The blinding polynomial of a proof has 2^8 entries or fewer: its commitment is a 32-leaf tree whose leaf hash is one wavefront walking 31
// dependent compressions, and every other step of its opening is a launch that keeps a workgroup or less busy and a synchronisation on a
// queue shared with the other provers.  Once the tables are within the host tail's threshold (pk_selftest_set_host_tail) prover.hip draws
// them on the device, brings them over in one transfer and runs the rest here: the RS-encode, the leaf hashes and the tree, the
// openings, the coefficient fold, the Horner evaluations and the grinder.  Every function restates one device step over host memory and
// leaves the values that step leaves (fully reduced, Montgomery unless named canonical): field arithmetic is exact, so the order in which
// sums are taken does not show.
//
// Host only, like host_tail.hpp: the field layer of transcript.hpp / protocol.hpp / host_tail.hpp and nothing of the runtime.  The largest
// transform has 32 points: a radix-2 NTT is enough.
#pragma once
#include <vector>

#include "host_tail.hpp"

namespace pk {
namespace host_whir {

using host_tail::mul;

// ---- RS-encode (rs_encode_x; ntt.hip): rows = 2^(n_vars + log_inv_rate - fold) leaves of width = batch * 2^fold, column-major
// leaves[col * rows + i], col = b * 2^fold + j:  leaf_i[col] = sum_t c_b[2^fold t + j] w^(i t),  w = the generator of the `rows` points --
// per column one natural-order NTT of the zero-padded stride-2^fold sub-sequence
inline void ntt(fe* x, unsigned log_n) {  // in place, natural -> natural: X[i] = sum_t x[t] w^(i t)
    const size_t n = (size_t)1 << log_n;
    for (size_t i = 0; i < n; i++) {  // bit reversal, then decimation in time
        size_t r = 0;
        for (unsigned b = 0; b < log_n; b++) r |= ((i >> b) & 1) << (log_n - 1 - b);
        if (r > i) std::swap(x[i], x[r]);
    }
    std::vector<fe> w(n / 2 ? n / 2 : 1);
    w[0] = fe_one();
    const fe gen = domain_generator(log_n);
    for (size_t e = 1; e < n / 2; e++) w[e] = mul(w[e - 1], gen);
    for (size_t len = 2; len <= n; len <<= 1) {
        const size_t step = n / len;
        for (size_t base = 0; base < n; base += len)
            for (size_t t = 0; t < len / 2; t++) {
                const fe a = x[base + t], b = mul(x[base + t + len / 2], w[t * step]);
                x[base + t] = h_add(a, b);
                x[base + t + len / 2] = h_sub(a, b);
            }
    }
}
inline void rs_encode(const fe* const* polys, unsigned batch, unsigned n_vars, unsigned log_inv_rate, unsigned fold, fe* leaves) {
    const unsigned log_rows = n_vars + log_inv_rate - fold;
    const size_t rows = (size_t)1 << log_rows, fw = (size_t)1 << fold, L = (size_t)1 << (n_vars - fold);
    for (unsigned b = 0; b < batch; b++)
        for (size_t j = 0; j < fw; j++) {
            fe* col = leaves + (b * fw + j) * rows;
            for (size_t t = 0; t < rows; t++) col[t] = t < L ? polys[b][fw * t + j] : fe_zero();
            ntt(col, log_rows);
        }
}

// ---- the hash: compress on canonical values (the verifier's h_compress; any 256-bit input is taken mod p) -----------------------------
inline fe compress(int version, const fe& l, const fe& r) {
    if (version == 2) {
        fe a = fe_reduce_any(l), b = fe_reduce_any(r);
        const fe l0 = a;
        sky_permute_host(a, b);
        return fe_add(a, l0);
    }
    return pack29(compress29<1, true>(unpack_reduce29(l), unpack_reduce29(r)));
}
// leaf_hash_kernel over the column-major Montgomery leaves: digest_i = h, h = x_0, h = C(h, x_j) on canonical values; canonical digests
inline void leaf_hash(int version, const fe* leaves, size_t rows, size_t width, fe* digests) {
    for (size_t i = 0; i < rows; i++) {
        fe h = h_to_canon(leaves[i]);
        for (size_t j = 1; j < width; j++) h = compress(version, h, h_to_canon(leaves[j * rows + i]));
        digests[i] = h;
    }
}
// pk_merkle_inner: the heap of 2 * rows digests, leaf digest i at rows + i (already there), nodes[i] = C(nodes[2i], nodes[2i+1]),
// nodes[1] the root, slot 0 cleared
inline void merkle_inner(int version, fe* nodes, size_t rows) {
    for (size_t i = rows - 1; i >= 1; i--) nodes[i] = compress(version, nodes[2 * i], nodes[2 * i + 1]);
    nodes[0] = fe_zero();
}
// commit_into: encode, hash, tree.  leaves: rows * width, nodes: 2 * rows
inline void commit(int version, const fe* const* polys, unsigned batch, unsigned n_vars, unsigned log_inv_rate, unsigned fold, fe* leaves, fe* nodes) {
    const size_t rows = (size_t)1 << (n_vars + log_inv_rate - fold), width = (size_t)batch << fold;
    rs_encode(polys, batch, n_vars, log_inv_rate, fold, leaves);
    leaf_hash(version, leaves, rows, width, nodes + rows);
    merkle_inner(version, nodes, rows);
}

// ---- open_raw's three arrays for the leaves idx[0 .. k): out_leaves[q][width] canonical, out_sib[q] = nodes[(rows + i) ^ 1] (rows >= 2),
// out_path[q][d - 1] = the sibling of the depth-d ancestor, d = 1 .. log2(rows) - 1, root -> leaf (gather_opening_kernel)
inline void open(const fe* leaves, const fe* nodes, size_t rows, size_t width, const uint64_t* idx, size_t k, fe* out_leaves, fe* out_sib, fe* out_path) {
    unsigned logn = 0;
    while (((size_t)1 << logn) < rows) logn++;
    const unsigned plen = logn ? logn - 1 : 0;
    for (size_t q = 0; q < k; q++) {
        const size_t i = (size_t)idx[q], node = rows + i;
        for (size_t j = 0; j < width; j++) out_leaves[q * width + j] = h_to_canon(leaves[j * rows + i]);
        if (logn) out_sib[q] = nodes[node ^ 1];
        for (unsigned d = 0; d < plen; d++) out_path[q * plen + d] = nodes[(node >> (logn - (d + 1))) ^ 1];
    }
}

// ---- pk_fold_coeffs: out[t] = sum_j c[2^k t + j] prod_b r_b^bit_b(j), t < 2^(n_vars - k)  (r[0] <-> index bit 0) ---------------------
inline void fold_coeffs(const fe* c, unsigned n_vars, const fe* r, unsigned k, fe* out) {
    const size_t fw = (size_t)1 << k, n_out = (size_t)1 << (n_vars - k);
    std::vector<fe> w(fw);
    w[0] = fe_one();
    for (unsigned b = 0; b < k; b++)
        for (size_t j = 0; j < ((size_t)1 << b); j++) w[j | ((size_t)1 << b)] = mul(w[j], r[b]);
    for (size_t t = 0; t < n_out; t++) {
        fe acc = c[t * fw];
        for (size_t j = 1; j < fw; j++) acc = h_add(acc, mul(c[t * fw + j], w[j]));
        out[t] = acc;
    }
}

// ---- eval_univariate_multi: sum_i c[i] z^i ---------------------------------------------------------------------------------------------
inline fe horner(const fe* c, size_t n, const fe& z) {
    fe acc = fe_zero();
    for (size_t i = n; i-- > 0;) acc = h_add(mul(acc, z), c[i]);
    return acc;
}

// ---- the grinder (pow_solve_x): the SMALLEST nonce with C(challenge, nonce) < threshold(bits + 0.01), searched in ascending order --------
inline bool pow_valid(const fe& challenge_reduced, const uint64_t thr[4], uint64_t nonce) {
    fe a = challenge_reduced, b = fe_zero();
    b.v[0] = (u32)nonce;
    b.v[1] = (u32)(nonce >> 32);
    sky_permute_host(a, b);
    const fe h = fe_add(a, challenge_reduced);
    fe t;
    memcpy(t.v, thr, 32);
    return fe_lt(h, t);
}
inline uint64_t pow_grind(const uint8_t challenge[POW_CHALLENGE_BYTES], double bits) {
    if (bits <= 0.0) return 0;  // pow.rs:34-36
    uint64_t thr[4];
    pow_threshold(bits + 0.01, thr);  // PROVER_BIAS, pow.rs:6,37
    const fe ch = fe_reduce_any(load_raw(challenge));
    uint64_t nonce = 0;
    while (!pow_valid(ch, thr, nonce)) nonce++;
    return nonce;
}

}  // namespace host_whir
}  // namespace pk
