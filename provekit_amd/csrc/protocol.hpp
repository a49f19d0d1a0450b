// protocol.hpp -- the wire rules on which the prover (prover.hip, pow.hip, whir_config.hip) and the verifier (verify/core.hpp) must
// agree bit for bit, each stated once.  Host only, on top of transcript.hpp's field layer; nothing here throws or needs a device.
//
// spongefish is an un-pinned, un-vendored git dependency of the reference (Cargo.toml:130-131), so the byte framing follows what the
// in-tree Go verifier consumes (recursive-verifier/app/circuit/common.go:30-105, utilities/utilities.go:84-101): scalars = 32-byte
// canonical little-endian, absorbed as field elements; hints = u32-LE length + payload, not absorbed; PoW nonce = 8 bytes big-endian,
// absorbed byte-wise; challenge bytes are taken 15 at a time from squeezed elements (spongefish's bytes_uniform_modp for a 254-bit
// modulus).
#pragma once
#include <algorithm>
#include <cmath>

#include "transcript.hpp"

namespace pk {

inline fe load_raw(const uint8_t* p) {
    fe r;
    memcpy(r.v, p, 32);
    return r;
}
inline bool is_canonical(const fe& raw) {
    fe p;
    for (int i = 0; i < 8; i++) p.v[i] = kPlimb(i);
    return fe_lt(raw, p);
}

// ---- the duplex sponge (provekit/common/src/skyscraper/sponge.rs:42-60): state = 2 field elements, rate 1, IV in the capacity
// element, overwrite mode: absorbing replaces the rate element.  At rate 1 spongefish's squeeze position always stands at the end of
// the rate, so every squeeze permutes; its absorb position says whether the rate element is fresh, and then an absorb permutes first.
constexpr size_t SQUEEZE_BYTES = 15;  // uniform bytes one squeezed element yields
inline size_t units_for_bytes(size_t n) { return (n + SQUEEZE_BYTES - 1) / SQUEEZE_BYTES; }

class DuplexSponge {
  public:
    unsigned permutes = 0;  // permutation calls so far
    explicit DuplexSponge(const std::string& io_pattern) {
        uint8_t iv[32];
        keccak_tag(io_pattern, iv);  // HashStateWithInstructions::generate_tag
        st_[0] = fe_zero();
        st_[1] = fe_reduce_any(load_raw(iv));  // FieldElement::new(bigint_from_bytes_le(iv)), sponge.rs:46-49
    }
    void absorb(const fe& canon) {
        if (absorb_pos_ == 1) permute();
        st_[0] = canon;
        absorb_pos_ = 1;
    }
    void absorb_bytes(const uint8_t* b, size_t n) {  // one element per byte
        for (size_t i = 0; i < n; i++) {
            fe c = fe_zero();
            c.v[0] = b[i];
            absorb(c);
        }
    }
    fe squeeze() {  // canonical
        permute();
        absorb_pos_ = 0;
        return st_[0];
    }
    void squeeze_bytes(uint8_t* out, size_t n) {  // units_for_bytes(n) squeezes
        while (n) {
            const fe c = squeeze();
            const size_t take = n < SQUEEZE_BYTES ? n : SQUEEZE_BYTES;
            memcpy(out, c.v, take);
            out += take;
            n -= take;
        }
    }

  private:
    fe st_[2];
    int absorb_pos_ = 0;
    void permute() {
        sky_permute_host(st_[0], st_[1]);
        permutes++;
    }
};

// ---- position in a parsed IO pattern: spongefish's HashStateWithInstructions checks every absorb / squeeze / hint against the
// declared stack; neighbouring operations of one kind were merged by the parser, so one declared operation may be taken in pieces ----
class IoCursor {
  public:
    explicit IoCursor(const std::vector<IoOp>& ops) : ops_(ops) {}
    // `n` units of `kind`: false, and nothing taken, unless the current operation is of that kind and has that many left
    bool take(char kind, size_t n) {
        if (!n) return true;
        if (at_end() || ops_[op_].kind != kind || remaining() < n) return false;
        used_ += n;
        if (used_ == ops_[op_].count) {
            op_++;
            used_ = 0;
        }
        return true;
    }
    size_t op_index() const { return op_; }
    bool at_end() const { return op_ >= ops_.size(); }
    char kind() const { return ops_[op_].kind; }                  // of the current operation: not at_end()
    size_t remaining() const { return ops_[op_].count - used_; }  // ditto

  private:
    const std::vector<IoOp>& ops_;
    size_t op_ = 0, used_ = 0;  // units of ops_[op_] already taken
};

// ---- hints: the length as a little-endian hint_len_t, then the payload; neither is absorbed -------------------------------------
typedef uint32_t hint_len_t;
// the payloads are ark-serialize uncompressed (common.go:36-73): a u64 little-endian, and a Vec<F> = its u64 length, then every
// element's canonical 32 bytes.  The writer (`montgomery`: the elements are still in Montgomery form) ...
inline void put_u64(std::vector<uint8_t>& buf, uint64_t v) {
    for (int i = 0; i < 8; i++) buf.push_back((uint8_t)(v >> (8 * i)));
}
inline void put_vec(std::vector<uint8_t>& buf, const fe* v, size_t n, bool montgomery = true) {
    put_u64(buf, n);
    for (size_t j = 0; j < n; j++) {
        const fe c = montgomery ? h_to_canon(v[j]) : v[j];
        buf.insert(buf.end(), (const uint8_t*)c.v, (const uint8_t*)c.v + 32);
    }
}
// ... and the bounded reader: every count is checked against the bytes that remain before anything is reserved for it
struct Rd {
    const uint8_t* b;
    size_t n, i = 0;
    size_t left() const { return n - i; }
    bool u64(uint64_t& v) {
        if (left() < 8) return false;
        memcpy(&v, b + i, 8);
        i += 8;
        return true;
    }
    // a count of items of at least `item_bytes` each: refused unless the payload can hold them
    bool count(uint64_t& v, size_t item_bytes) { return u64(v) && v <= left() / item_bytes; }
    bool skip(size_t bytes, const uint8_t*& p) {
        if (left() < bytes) return false;
        p = b + i;
        i += bytes;
        return true;
    }
    bool end() const { return i == n; }
};
struct HintFe {
    fe mont;
    bool canonical;
};
inline bool parse_vec(Rd& rd, std::vector<HintFe>& out) {  // Vec<F>
    uint64_t c;
    if (!rd.count(c, 32)) return false;
    out.resize((size_t)c);
    for (auto& x : out) {
        const uint8_t* p;
        rd.skip(32, p);
        const fe raw = load_raw(p);
        x.canonical = is_canonical(raw);
        x.mont = h_from_canon(raw);
    }
    return true;
}

// ---- STIR query indexes (recursive-verifier/app/circuit/whir_utilities.go:48-77): per query ceil(log2(folded)/8) challenge bytes,
// big-endian, low bits kept; then sorted + deduplicated as whir does.  Each side squeezes the bytes between the two calls. -----------
inline size_t stir_query_bytes(uint64_t domain, unsigned fold) {
    const uint64_t folded = domain >> fold;
    unsigned bits = 0;
    while ((folded >> (bits + 1)) != 0) bits++;
    return (bits + 7) / 8;
}
inline std::vector<uint64_t> stir_indexes(const uint8_t* raw, uint64_t domain, unsigned fold, unsigned n_queries) {
    const uint64_t folded = domain >> fold;
    const size_t nbytes = stir_query_bytes(domain, fold);
    std::vector<uint64_t> idx(n_queries);
    for (unsigned q = 0; q < n_queries; q++) {
        uint64_t v = 0;
        for (size_t j = 0; j < nbytes; j++) v = (v << 8) | raw[q * nbytes + j];
        idx[q] = v & (folded - 1);
    }
    std::sort(idx.begin(), idx.end());
    idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
    return idx;
}

// ---- evaluation domains: ark-bn254 Fr's two-adic root of unity 5^((p-1) >> 28), Montgomery --------------------------------------
namespace host64 {
constexpr uint64_t ROOT28[4] = {0x9bd61b6e725b19f0ULL, 0x402d111e41112ed4ULL, 0x00e0a7eb8ef62abcULL, 0x2a3c09f0a58a7e85ULL};  // canonical
// the literal against the definition, in the compiler: Montgomery images by 256 doublings, a square-and-multiply ladder, and back
constexpr bool root28_is_5_to_the_odd_part() {
    uint64_t e[4] = {P64[0] - 1, P64[1], P64[2], P64[3]};
    for (int i = 0; i < 4; i++) e[i] = (e[i] >> 28) | (i < 3 ? e[i + 1] << 36 : 0);
    const uint64_t one[4] = {1, 0, 0, 0};
    uint64_t acc[4] = {1, 0, 0, 0}, base[4] = {5, 0, 0, 0};
    for (int i = 0; i < 256; i++) add_mod(acc, acc), add_mod(base, base);
    for (int bit = 0; bit < 256; bit++) {
        if ((e[bit >> 6] >> (bit & 63)) & 1) mont_mul(acc, base, acc);
        mont_mul(base, base, base);
    }
    mont_mul(acc, one, acc);
    return acc[0] == ROOT28[0] && acc[1] == ROOT28[1] && acc[2] == ROOT28[2] && acc[3] == ROOT28[3];
}
static_assert(root28_is_5_to_the_odd_part(), "ROOT28 is not 5^((p-1) >> 28)");
}  // namespace host64

// generator of the domain of 2^log_size points: root28^(2^(28 - log_size))
inline fe domain_generator(unsigned log_size) {
    fe gen = h_from_canon(h_load(host64::ROOT28));
    for (unsigned i = log_size; i < 28; i++) gen = h_mul(gen, gen);
    return gen;
}
// ... raised to the 2^fold-th power (whir.go:99): root28^(2^(28 - log_size + fold)).  Whether a caller thinks of it as one run of
// 28 + fold - log_size squarings or as the domain's generator squared `fold` more times, it is this one function of (log_size, fold).
inline fe folded_domain_generator(unsigned log_size, unsigned fold) {
    fe gen = domain_generator(log_size);
    for (unsigned i = 0; i < fold; i++) gen = h_mul(gen, gen);
    return gen;
}

// ---- algebra both sides evaluate -------------------------------------------------------------------------------------------------
// ExpandFromUnivariate (recursive-verifier/app/utilities/utilities.go:182-190): out[n-1-i] = z^(2^i)
inline void expand_from_univariate(fe z, size_t n, fe* out) {
    for (size_t i = 0; i < n; i++) {
        out[n - 1 - i] = z;
        z = h_mul(z, z);
    }
}
inline fe eval_cubic(const fe c[4], const fe& x) {  // provekit/common/src/utils/sumcheck.rs:174-176
    return h_add(c[0], h_mul(x, h_add(c[1], h_mul(x, h_add(c[2], h_mul(x, c[3]))))));
}

// the quadratic through h(0), h(1), h(2) = h[0..3) at x: the WHIR sumcheck's next claim (whir_utilities.go:102-125)
inline fe eval_quadratic_012(const fe h[3], const fe& x) {
    const fe c2 = h_mul(h_half(), h_add(h_sub(h_sub(h[2], h[1]), h[1]), h[0]));  // h(2) = 2 h(1) - h(0) + 2 c2
    const fe c1 = h_sub(h_sub(h[1], h[0]), c2);
    return h_add(h[0], h_mul(x, h_add(c1, h_mul(x, c2))));
}

// ---- proof of work (utilities.go:84-101): POW_CHALLENGE_BYTES challenge bytes are squeezed, the nonce is absorbed as 8 big-endian
// bytes; compress(challenge, nonce) must lie below the threshold ----------------------------------------------------------------------
constexpr size_t POW_CHALLENGE_BYTES = 32, POW_NONCE_BYTES = 8;
inline void nonce_to_bytes(uint64_t nonce, uint8_t out[POW_NONCE_BYTES]) {
    for (int i = 0; i < 8; i++) out[i] = (uint8_t)(nonce >> (56 - 8 * i));
}
inline uint64_t nonce_from_bytes(const uint8_t in[POW_NONCE_BYTES]) {
    uint64_t nonce = 0;
    for (int i = 0; i < 8; i++) nonce = (nonce << 8) | in[i];
    return nonce;
}
// skyscraper/core/src/pow.rs:44-82
inline void f64_to_u256(double f, uint64_t out[4]) {
    uint64_t bits;
    memcpy(&bits, &f, 8);
    const bool sign = bits >> 63;
    const int exp_bits = (int)((bits >> 52) & 0x7ff);
    const uint64_t frac = bits & ((1ull << 52) - 1);
    const int exp = exp_bits == 0 ? -1022 : exp_bits - 1023;
    const uint64_t significand = exp_bits == 0 ? frac : frac + (1ull << 52);
    memset(out, 0, 32);
    if (sign) return;
    if (exp > 256) {
        memset(out, 0xff, 32);
        return;
    }
    const int shift = exp - 52;
    if (shift < 0) {
        const double r = std::round(f);
        out[0] = r >= 18446744073709551616.0 ? UINT64_MAX : (r > 0 ? (uint64_t)r : 0);
    } else {
        const unsigned limb = (unsigned)shift / 64, sh = (unsigned)shift % 64;
        if (limb > 3) return;
        out[limb] = significand << sh;
        if (sh != 0 && limb < 3) out[limb + 1] = significand >> (64 - sh);
    }
}
// pow.rs:14-22: 2^-difficulty times the modulus, taken as its top limb x 2^192.  The arithmetic alone: the callers bound `difficulty`.
inline void pow_threshold(double difficulty, uint64_t out[4]) {
    const double modulus = (double)host64::P64[3] * std::ldexp(1.0, 192);
    f64_to_u256(std::exp2(-difficulty) * modulus, out);
}

}  // namespace pk
