// selftest_inv30.hpp -- the second table of arithmetic self-tests, next to selftest_op (selftest_ops.hpp, which includes this file): the
// parts of the safegcd inverse, whose operands (two 257-bit signed values and a matrix) do not fit the two field elements of that table.
// A header of its own because it needs feinv.hpp alone, so that the sanitizer build (feinv_asan_main.cpp, plain C++) can compile it.
#pragma once
#include "feinv.hpp"

namespace pk {

// The parts of feinv.hpp one at a time: the functions of pk::inv30 themselves on one record of 32 words in, 32 words out (words the
// part does not name are ignored on the way in and zero on the way out).  Two users again: pk_selftest_inv30 (selftest.hip, host) and
// pk_probe_inv30_device (tools/probes, one lane per record); tests/feinv_refs.py holds the operands and what each part must return.
// An s30 travels as its nine limbs, a trans as u, v, q, r, a word of f or g as its 32 bits.
//   part 0 divsteps30      in: zeta, f0, g0                        out: u, v, q, r, zeta'
//   part 1 divsteps30_var  in: eta, f0, g0                         out: u, v, q, r, eta'
//   part 2 update_de       in: d[0..9), e[9..18), u, v, q, r       out: d'[0..9), e'[9..18)
//   part 3 update_fg       in: f[0..9), g[9..18), u, v, q, r       out: f'[0..9), g'[9..18)
//   part 4 normalize       in: r[0..9), sign                       out: r'[0..9)
//   part 5 to_s30          in: the 8 words of a 256-bit value      out: its nine limbs
//   part 6 from_s30        in: nine limbs                          out: the 8 words
// false: no such part (out is all zero).
PK_HD bool selftest_inv30(int part, const int32_t in[32], int32_t out[32]) {
    using namespace inv30;
    for (int i = 0; i < 32; i++) out[i] = 0;
    s30 a, b;
    for (int i = 0; i < 9; i++) {
        a.v[i] = in[i];
        b.v[i] = in[9 + i];
    }
    trans t;
    t.u = in[18];
    t.v = in[19];
    t.q = in[20];
    t.r = in[21];
    switch (part) {
        case 0:
        case 1:
            out[4] = part == 0 ? divsteps30(in[0], (u32)in[1], (u32)in[2], t) : divsteps30_var(in[0], (u32)in[1], (u32)in[2], t);
            out[0] = t.u;
            out[1] = t.v;
            out[2] = t.q;
            out[3] = t.r;
            return true;
        case 2:
        case 3:
            if (part == 2) update_de(a, b, t);
            else update_fg(a, b, t);
            for (int i = 0; i < 9; i++) {
                out[i] = a.v[i];
                out[9 + i] = b.v[i];
            }
            return true;
        case 4:
            normalize(a, in[9]);
            for (int i = 0; i < 9; i++) out[i] = a.v[i];
            return true;
        case 5: {
            fe x;
            for (int i = 0; i < 8; i++) x.v[i] = (u32)in[i];
            a = to_s30(x);
            for (int i = 0; i < 9; i++) out[i] = a.v[i];
            return true;
        }
        case 6: {
            const fe x = from_s30(a);
            for (int i = 0; i < 8; i++) out[i] = (i32)x.v[i];
            return true;
        }
        default: return false;
    }
}

}  // namespace pk
