// statement.hpp -- what the sources of libprovekit_spark.so share on the host: which statements the library takes, the outer IO
// pattern, the three sides' inner statements, the table's extension the verifier evaluates itself and the claims.  Host only; no
// device, and of other libraries only what provekit_sumcheck.h and provekit_tuplelookup.h declare.
#pragma once
#include <string>

#include "../../../include/provekit_spark.h"
#include "../argument.hpp"

namespace pkx {

using pk::fe;

extern thread_local std::string g_error;  // pkx_create_error
inline int refuse(const std::string& why) { return pk::refuse(g_error, why); }

using pk::elements_below_p;
using pk::pattern_op;
using pk::put_fe;

inline bool statement_ok(const pkx_statement* st, std::string& why) {
    if (!st) return why = "null statement", false;
    if (st->n < 1 || st->n > PKX_MAX_VARS) return why = "n must be 1..28", false;
    if (st->s < 1 || st->s > PKX_MAX_VARS) return why = "s must be 1..28", false;
    if (st->t < 1 || st->t > PKX_MAX_VARS) return why = "t must be 1..28", false;
    if (st->n_bind > PKX_MAX_BIND) return why = "n_bind must be 0..16", false;
    return true;
}

inline std::string io_pattern(const pkx_statement& st) {
    std::string d = "provekit-hip/spark/v1/n" + std::to_string(st.n) + "/s" + std::to_string(st.s) + "/t" + std::to_string(st.t);
    pattern_op(d, 'A', st.n_bind, "bind");
    pattern_op(d, 'A', st.s, "rx");
    pattern_op(d, 'A', st.t, "ry");
    pattern_op(d, 'S', 3, "seeds");
    return d;
}

// the three sides of a proof; each binds its seed.  VAL: sum_x val e_row e_col, one term of three tables
inline pks_statement side_val(const pkx_statement& st) {
    pks_statement v{};
    v.n = st.n, v.m = 3, v.T = 1, v.has_tau = 0, v.n_bind = 1, v.masks[0] = 7;
    put_fe(v.coeffs[0], pk::fe_one());
    return v;
}
// ROW, COL: rows (index, e) in the table (I, eq(point, .)): a ROM read
inline unsigned side_bits(const pkx_statement& st, int side) { return side == PKX_SIDE_ROW ? st.s : st.t; }
inline pkt_statement side_lookup(const pkx_statement& st, int side) { return pkt_statement{st.n, side_bits(st, side), 2, 1, 1}; }

// eq(r, y) = prod_i (r_i y_i + (1 - r_i)(1 - y_i)): the extension of pk_eq_table's table of r at y
inline fe eq_at(const fe* r, const fe* y, unsigned v) {
    fe acc = pk::fe_one();
    for (unsigned i = 0; i < v; i++) {
        const fe both = pk::h_mul(r[i], y[i]);  // r y + (1 - r)(1 - y) = 1 - r - y + 2 r y
        acc = pk::h_mul(acc, pk::h_add(pk::h_sub(pk::h_sub(pk::fe_one(), r[i]), y[i]), pk::h_add(both, both)));
    }
    return acc;
}
// PKX_CHECK_TABLE: the extension of the table (I, eq(r, .)) compressed by beta, at y
inline fe table_at(const fe* r, const fe& beta, const fe* y, unsigned v) { return pk::h_add(pk::index_at(y, v), pk::h_mul(beta, eq_at(r, y, v))); }

// The claims of an accepted proof from the three sides' ends
inline void fill_claims(const pkx_statement& st, const fe& value, const fe* z_val, const fe* finals, const pkt_claims look[2], pkx_claims* out) {
    memset(out, 0, sizeof *out);
    put_fe(out->value, value);
    for (unsigned i = 0; i < st.n; i++) put_fe(out->z_val[i], z_val[i]);
    for (unsigned j = 0; j < 3; j++) put_fe(out->val_values[j], finals[j]);
    for (int side = 0; side < 2; side++) {
        const pkt_claims& c = look[side];
        memcpy(out->beta[side], c.beta, 32);
        memcpy(out->z_f[side], c.z_lo, 32 * (size_t)st.n);
        memcpy(out->f_coeff[side][0], c.f_coeff[0][0], 32), memcpy(out->f_coeff[side][1], c.f_coeff[0][1], 32);
        memcpy(out->f_value[side], c.f_value, 32);
        memcpy(out->z_m[side], c.z_t, 32 * (size_t)side_bits(st, PKX_SIDE_ROW + side));
        memcpy(out->m_value[side], c.m_value, 32);
    }
}

// the library's overload sets, for argument.hpp's templates (the proof's length comes from the inner libraries' C ABI)
struct Lib {
    static std::string& error() { return g_error; }
    static bool ok(const pkx_statement* st, std::string& why) { return statement_ok(st, why); }
    static std::string pattern(const pkx_statement& st) { return io_pattern(st); }
};

}  // namespace pkx
