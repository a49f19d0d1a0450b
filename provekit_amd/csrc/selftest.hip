// selftest.hip -- host-side execution of the exact __host__ __device__ arithmetic the kernels use
// (fe29.hpp, skyscraper29.hpp), so the CPU test suite can check it against the oracle without a GPU; and the two host-only
// pieces of the transcript the parity tests pin (domain-separator tag, sponge permutation).  Measurement probes and rejected
// prototypes live in tools/probes (libpk_probes.so), not in the product.
#include "selftest_ops.hpp"
#include "ntt_regs.hpp"
#include "transcript.hpp"

using namespace pk;

// the NTT's register butterfly network on the host (ntt_regs.hpp dft_regs<le, d>): n_groups x 2^le values below 1.2p in, the network's
// outputs out.  tw (may be NULL): one multiplier below p per value, applied to the network's UNREDUCED outputs the way the pass kernel
// applies its inter-round / inter-pass twiddles (Shoup product with the table's quotient); without it the outputs are only reduced.
template <int LE, int D>
static int selftest_dft(const uint64_t* in, const uint64_t* tw, uint64_t* out, size_t n_groups) {
    constexpr int NX = 1 << LE;
    for (size_t g = 0; g < n_groups; g++) {
        fe29 x[NX];
        for (int i = 0; i < NX; i++) x[i] = unpack29<0>(load_host(in + 4 * (NX * g + i)));
        dft_regs<LE, D>(x);
        for (int i = 0; i < NX; i++) {
            fe29 y;
            if (tw) {
                tw29s t;
                t.w = unpack29<0>(load_host(tw + 4 * (NX * g + i)));
                t.wq = shoup_quotient29(t.w);
                y = mul_tw(x[i], t);
                for (int k = 0; k < 9; k++)
                    if (y.v[k] >> 29) return PK_ERR_BAD_ARG;  // a product leaves normalised limbs
            } else {
                y = (i >> (LE - D)) == 0 ? red29(x[i]) : red29w(x[i]);  // as the pass kernel: frequency digit 0 is the sum of sums
            }
            store_host(out + 4 * (NX * g + i), pack29(cond_sub_p29(y)));
        }
    }
    return PK_OK;
}
// ntt_regs.hpp pre_load_sum on the host: n outputs, each from `terms` inputs x (any value below 2^256) and `terms` multipliers
// below p (Shoup products with the quotient the twiddle tables hold); rows n1 >= live read as past the nonzero inputs.  out: the
// lazy result as it enters the network (not reduced further); a result with a limb not normalised is an error.
static int selftest_pre_load(const uint64_t* x, const uint64_t* tw, uint64_t* out, int terms, int live, size_t n) {
    for (size_t i = 0; i < n; i++) {
        const fe29 y = pre_load_sum(terms, [&](int n1, fe29& v) {
            if (n1 >= live) return false;
            tw29s t;
            t.w = unpack29<0>(load_host(tw + 4 * (terms * i + n1)));
            t.wq = shoup_quotient29(t.w);
            v = mul_tw(unpack29<0>(load_host(x + 4 * (terms * i + n1))), t);
            return true;
        });
        for (int k = 0; k < 9; k++)
            if (y.v[k] >> 29) return PK_ERR_BAD_ARG;
        store_host(out + 4 * i, pack29(y));
    }
    return PK_OK;
}
extern "C" {

// domain-separator tag (Keccak duplex, overwrite mode) and one Skyscraper sponge permutation, host only
int pk_selftest_keccak_tag(const uint8_t* data, size_t len, uint8_t tag[32]) {
    if (!tag || (len && !data)) return PK_ERR_BAD_ARG;
    keccak_tag(std::string((const char*)data, len), tag);
    return PK_OK;
}
int pk_selftest_permute(uint64_t l[4], uint64_t r[4]) {
    if (!l || !r) return PK_ERR_BAD_ARG;
    fe a = load_host(l), b = load_host(r);
    sky_permute_host(a, b);
    store_host(l, a);
    store_host(r, b);
    return PK_OK;
}

// op: 0 fe_mul29(a,b)  1 compress v2  2 compress v1  3 from_mont  4 a*b*2^-256 via mont256_29  5 a^2*2^-256 via sqr256_29
// 6..26: the rest of the table in selftest_ops.hpp (conversions, lazy reductions, wide_reduce, the scaled path, dot29, the inverse,
// the Shoup product, the NTT's constants)
// the carry chains of fe.hpp: 27 fe_add(a,b)  28 fe_sub(a,b)  29 fe_neg(a)  30 fe_dbl(a)  31 {a < b, a == b, b < a} in words 0..2
// 32/33/34 cond_sub_kp<1/2/4>(a)  35 fe_reduce_any(a)  36 fe_fold(a, b, one) == b  37 fe_fold(a, b, a)  38 pack_canon29(unpack29(a))
// the consumers of a stored hash-ready codeword element (a, b < SCALED32_BOUND, skyscraper29s.hpp): 39 / 40 compress v2 / v1 as the leaf
// fold enters it  41 a fold of three  42 / 43 the canonical / Montgomery opening (opened_element)
// a, b, out: n field elements (4 x u64 each); b may be NULL for the one-operand ops.  Host only; no device needed.
int pk_selftest_arith(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
    const bool two = op == 0 || op == 1 || op == 2 || op == 4 || op == 15 || op == 16 || op == 19 || op == 20 || op == 24 || op == 25 ||
                     op == 27 || op == 28 || op == 31 || op == 36 || op == 37 || op == 39 || op == 40 || op == 41;
    if (!a || !out || (!b && two)) return PK_ERR_BAD_ARG;
    for (size_t i = 0; i < n; i++) {
        fe x = load_host(a + 4 * i), y = b ? load_host(b + 4 * i) : x;
        if (op < 0 || op > 43) return PK_ERR_BAD_ARG;
        fe r = selftest_op(op, x, y);
        store_host(out + 4 * i, r);
    }
    return PK_OK;
}

// the parts of the safegcd inverse (feinv.hpp: divsteps30, divsteps30_var, update_de, update_fg, normalize, to_s30, from_s30 = part 0..6) on
// n records of 32 words in, 32 words out; the packing of a record is stated at selftest_inv30 (selftest_inv30.hpp).  Host only.
int pk_selftest_inv30(int part, const int32_t* in, int32_t* out, size_t n) {
    if (!in || !out || part < 0 || part > 6) return PK_ERR_BAD_ARG;
    for (size_t i = 0; i < n; i++)
        if (!selftest_inv30(part, in + 32 * i, out + 32 * i)) return PK_ERR_BAD_ARG;
    return PK_OK;
}

int pk_selftest_pre_load(const uint64_t* x, const uint64_t* tw, uint64_t* out, int terms, int live, size_t n) {
    if (!x || !tw || !out || terms < 1 || terms > 4 || live < 0 || live > terms) return PK_ERR_BAD_ARG;
    return selftest_pre_load(x, tw, out, terms, live, n);
}
int pk_selftest_dft(const uint64_t* in, const uint64_t* tw, uint64_t* out, int le, int d, size_t n_groups) {
    if (!in || !out) return PK_ERR_BAD_ARG;
    if (le == 3 && d == 1) return selftest_dft<3, 1>(in, tw, out, n_groups);
    if (le == 3 && d == 2) return selftest_dft<3, 2>(in, tw, out, n_groups);
    if (le == 2 && d == 1) return selftest_dft<2, 1>(in, tw, out, n_groups);
    if (le == 2 && d == 2) return selftest_dft<2, 2>(in, tw, out, n_groups);
    return PK_ERR_BAD_ARG;
}

}  // extern "C"
