// statement.hpp -- what the sources of libprovekit_rangecheck.so share: the plan (one __host__ __device__ rule that prover, verifier,
// kernels and claims read), which statements the library takes, the outer IO pattern, the inner lookup's statement and the claims.
// Of other libraries only what provekit_tuplelookup.h declares.
#pragma once
#include <string>

#include "../../../include/provekit_rangecheck.h"
#include "../argument.hpp"

namespace pkr {

using pk::fe;

// THE PLAN.  L = ceil(bits / k) limbs; r = bits - (L - 1) k bits in the top limb; groups 0 .. L - 1 the limbs; when r < k group L the
// top check, 2^(k-r) limb_{L-1}; G = L + (r < k); c the smallest of {1, 2, 4} with c >= G, the spare group of G = 3 being limb 0 again.
// G > 4 leaves c = 0: the statement is refused.  Valid for 1 <= bits <= 64, 1 <= k <= 28.
struct Plan {
    unsigned L, r, G, c;
    unsigned limb_of[PKR_MAX_GROUPS], shift_of[PKR_MAX_GROUPS];
};
__host__ __device__ inline Plan plan_of(unsigned bits, unsigned k) {
    Plan P{};
    P.L = (bits + k - 1) / k;
    P.r = bits - (P.L - 1) * k;
    P.G = P.L + (P.r < k ? 1 : 0);
    P.c = P.G > PKR_MAX_GROUPS ? 0 : P.G == 3 ? 4 : P.G;
    for (unsigned g = 0; g < PKR_MAX_GROUPS; g++) {
        const bool limb = g < P.L, top = !limb && g < P.G;
        P.limb_of[g] = limb ? g : top ? P.L - 1 : 0;  // the spare group: limb 0 again
        P.shift_of[g] = top ? k - P.r : 0;
    }
    return P;
}
// the smallest limb width with at most four groups: ceil(bits / 3) leaves three limbs and a top check at most
__host__ __device__ inline unsigned width_that_works(unsigned bits) { return (bits + 2) / 3; }

extern thread_local std::string g_error;  // pkr_create_error
inline int refuse(const std::string& why) { return pk::refuse(g_error, why); }

using pk::elements_below_p;
using pk::pattern_op;
using pk::put_fe;

inline unsigned log2_groups(unsigned c) { return c == 4 ? 2 : c == 2 ? 1 : 0; }

inline bool statement_ok(const pkr_statement* s, std::string& why) {
    if (!s) return why = "null statement", false;
    if (s->n < 1 || s->n > PKR_MAX_VARS) return why = "n must be 1..28", false;
    if (s->bits < 1 || s->bits > PKR_MAX_BITS) return why = "bits must be 1..64", false;
    if (s->k < 1 || s->k > PKR_MAX_LIMB_BITS) return why = "k must be 1..28", false;
    if (s->n_bind > PKR_MAX_BIND) return why = "n_bind must be 0..16", false;
    const Plan P = plan_of(s->bits, s->k);
    if (!P.c)
        return why = "bits = " + std::to_string(s->bits) + " in limbs of k = " + std::to_string(s->k) + " bits needs " + std::to_string(P.G) +
                     " groups, at most 4 are looked up in one proof: k = " + std::to_string(width_that_works(s->bits)) + " works, as every k >= ceil(bits / 3)",
               false;
    if (s->n + log2_groups(P.c) > PKR_MAX_VARS) return why = "n + log2 c must be at most 28 (c = " + std::to_string(P.c) + " groups)", false;
    return true;
}

inline std::string io_pattern(const pkr_statement& s) {
    std::string d = "provekit-hip/range/v1/n" + std::to_string(s.n) + "/b" + std::to_string(s.bits) + "/k" + std::to_string(s.k);
    pattern_op(d, 'A', s.n_bind, "bind");
    pattern_op(d, 'S', 1, "seed");
    return d;
}

// the one inner proof: c groups of one column in the table I_k, binding the seed
inline pkt_statement lookup_of(const pkr_statement& s) { return pkt_statement{s.n, s.k, 1, plan_of(s.bits, s.k).c, 1}; }

// 2^e as an element, e < 64
inline fe pow2(unsigned e) { return pk::h_from_u64((uint64_t)1 << e); }

// The claims of an accepted proof from the lookup's: coeff_i = sum over the groups g of limb i of eq(z_hi, g) 2^shift_g
inline void fill_claims(const pkr_statement& s, const pkt_claims& look, pkr_claims* out) {
    memset(out, 0, sizeof *out);
    const Plan P = plan_of(s.bits, s.k);
    memcpy(out->z_lo, look.z_lo, 32 * (size_t)s.n);
    memcpy(out->z_t, look.z_t, 32 * (size_t)s.k);
    fe coeff[PKR_MAX_GROUPS];
    for (fe& c : coeff) c = pk::fe_zero();
    for (unsigned g = 0; g < P.c; g++) {
        const fe eq = pk::h_load(look.f_coeff[g][0]);
        coeff[P.limb_of[g]] = pk::h_add(coeff[P.limb_of[g]], P.shift_of[g] ? pk::h_mul(eq, pow2(P.shift_of[g])) : eq);
    }
    for (unsigned i = 0; i < P.L; i++) put_fe(out->limb_coeff[i], coeff[i]), put_fe(out->pow2[i], pow2(s.k * i));
    memcpy(out->limbs_value, look.f_value, 32);
    memcpy(out->m_value, look.m_value, 32);
}

// the library's overload sets, for argument.hpp's templates (the proof's length comes from the tuple-lookup library's C ABI)
struct Lib {
    static std::string& error() { return g_error; }
    static bool ok(const pkr_statement* s, std::string& why) { return statement_ok(s, why); }
    static std::string pattern(const pkr_statement& s) { return io_pattern(s); }
};

}  // namespace pkr
