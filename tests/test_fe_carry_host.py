"""CPU: the host build of the field's carry chains (csrc/fe.hpp: fe_add, fe_sub, fe_neg, fe_dbl, fe_lt, fe_eq, cond_sub_kp,
fe_reduce_any; fe_fold and pack_canon29 on top of them; wide_reduce and the products' final subtractions) through pk_selftest_arith,
against Python ints, on the operands of tests/fe_carry_cases.py: carries riding through all-ones words, borrows riding through equal
words, results and operands one off the modulus at every limb.  Bit-exact; tests/test_gpu_fe_carry.py runs the same on the device."""
import numpy as np
import pytest

import fe_carry_cases as fc

P = fc.P


def run(op, xs, ys=None):
    from provekit_amd._lib import lib

    a = fc.to_limbs(xs)
    b = fc.to_limbs(ys) if ys is not None else None
    out = np.empty_like(a)
    assert lib.pk_selftest_arith(op, a.ctypes.data, b.ctypes.data if b is not None else None, out.ctypes.data, a.shape[0]) == 0
    return fc.from_limbs(out)


def mismatches(got, want, xs, ys):
    return [(hex(x), hex(y), hex(g), hex(w)) for x, y, g, w in zip(xs, ys, got, want) if g != w][:4]


@pytest.mark.parametrize("op", sorted(fc.NEW_OPS))
def test_chain_op_equals_its_definition(op):
    xs, ys, want = fc.new_op_cases(op)
    assert len(xs) > 100
    assert mismatches(run(op, xs, ys), want, xs, ys) == [], fc.NEW_OPS[op][0]
    if op in fc.ONE_OPERAND:  # the second operand may be absent
        assert run(op, xs) == want


def test_two_operand_ops_refuse_a_missing_operand():
    """(where the table ends is asserted with its last ops, in tests/test_scaled_codeword_host.py)"""
    from provekit_amd._lib import lib

    a = fc.to_limbs([1, 2])
    out = np.empty_like(a)
    for op in sorted(fc.NEW_OPS):
        rc = lib.pk_selftest_arith(op, a.ctypes.data, None, out.ctypes.data, 2)
        assert (rc == 0) == (op in fc.ONE_OPERAND), op
    assert max(fc.NEW_OPS) == 38 and lib.pk_selftest_arith(-1, a.ctypes.data, a.ctypes.data, out.ctypes.data, 2) != 0


@pytest.mark.parametrize("op", sorted(fc.OLD_UNARY))
def test_single_operand_ops_on_the_structured_values(oracle, op):
    """ops 3, 6, 7, 9, 12, 17, 18 (Montgomery conversions, lazy and exact reductions, the scaled domain's conversions) over the
    structured values of both limb widths, as far up as each op's contract reaches (2^256 - 1 for ops 9 and 17)"""
    bound, define = fc.OLD_UNARY[op]
    xs = fc.old_unary_cases(op)
    assert max(xs) == min(bound, fc.R) - 1 and len(xs) > 200
    got = run(op, xs)
    if define is None:  # op 9: almost reduced
        for x, r in zip(xs, got):
            assert r % P == x % P and r < P + (P >> 10), hex(x)
    else:
        assert mismatches(got, [define(x) for x in xs], xs, xs) == []
    if op in (3, 18):  # and the oracle's into_bigint(), as tests/test_fe29_host.py
        assert got == oracle.limbs_to_ints(oracle.from_mont(oracle.ints_to_limbs(xs)))


def test_wide_reduce_on_both_sides_of_every_multiple_of_p():
    cases = fc.wide_pairs()
    xs, ys = [c[0] for c in cases], [c[1] for c in cases]
    want = [d % P for _, _, _, d in cases]  # 700 x + 324 y == k p + d
    assert mismatches(run(14, xs, ys), want, xs, ys) == []


def test_products_that_land_on_the_structured_values():
    cases = fc.mont_products()
    xs, ys, ts = ([c[i] for c in cases] for i in range(3))
    assert all(x * y * fc.RINV % P == t for x, y, t in cases)
    assert mismatches(run(0, xs, ys), ts, xs, ys) == []  # fe_mul29
    cases = fc.shoup_products()
    xs, ys, ts = ([c[i] for c in cases] for i in range(3))
    assert all(x * w % P == t for x, w, t in cases)
    assert mismatches(run(24, xs, ys), ts, xs, ys) == []  # shoup261_29


def test_the_cases_cover_what_they_claim():
    """on the ints alone: every carry run, every borrow run, the sums and differences at the modulus, every reachable multiple of p"""
    cov = fc.coverage()
    assert cov["add_runs"] >= fc.ADD_RUNS and len(fc.ADD_RUNS) == 28
    assert cov["sub_runs"] >= fc.SUB_RUNS and fc.SUB_RUNS >= fc.ADD_RUNS
    assert all(cov["sums"].values()) and len(cov["sums"]) == 4, cov["sums"]
    assert all(cov["diffs"].values()) and len(cov["diffs"]) == 5, cov["diffs"]
    assert cov["wide_k"] == set(range(1024))
    assert cov["wide_d"] == {(0, 0), (1, -1), (2, -2), (2, 2), (3, 1)}  # d == -k mod 4: d == 0 exactly for the multiples of 4
    # the structured sets hold what the chains' edges need
    for c in (P, 2 * P, 4 * P):
        s = fc.structured(32, c)
        assert {0, 1, c - 1, c, c + 1, (1 << 224) - 1, (((c >> 192) - 1) << 192) | ((1 << 192) - 1), ((c >> 192) + 1) << 192} <= set(s)
    assert {(1 << 232) - 1, 1 << 232, P - 1, P, P + 1} <= set(fc.structured(29, P))
    assert max(fc.structured_below()) == P - 1 and max(fc.structured_below(2 * P)) == 2 * P - 1 and max(fc.structured_any()) == fc.TOP
    # the fold pairs hand fe_fold's inner sub and add exactly the targeted pairs
    n_add = len(fc.add_pairs())
    assert all(x == a and (y - x) % P == b for (x, y), (a, b) in zip(fc.fold_pairs()[:n_add], fc.add_pairs()))
    assert all((y, x) == ab for (x, y), ab in zip(fc.fold_pairs()[n_add:], fc.sub_pairs()))


def test_random_operands_never_reach_a_riding_carry():
    """why the case module exists: 5000 random pairs below p (what tests/test_gpu_hash.py gives pk_fe_add / pk_fe_sub) hold no carry
    or borrow that rides through even one word"""
    from provekit_amd.field import random_field

    a, b = fc.from_limbs(random_field(5000, 1)), fc.from_limbs(random_field(5000, 2))
    assert all(x < P for x in a + b)
    assert not any(ln >= 1 for x, y in zip(a, b) for _, ln in fc.add_runs(x, y) | fc.sub_runs(x, y))
    sums, diffs = {x + y for x, y in zip(a, b)}, {x - y for x, y in zip(a, b)}
    assert not sums & {P - 1, P, P + 1} and not diffs & {0, 1, -1}
