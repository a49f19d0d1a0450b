"""CPU: the references of tests/test_gpu_mle_edges.py (tests/mle_edge_refs.py) against the C oracle and against plain Python sums at
small sizes -- a closed form or a grouped definition that is wrong would otherwise only show as a GPU test failing for no reason
in the kernel."""
import numpy as np
import pytest

import mle_edge_refs as E
from provekit_amd.field import random_field

P = E.P


def test_constants_and_stored_arithmetic(oracle):
    one = oracle.to_mont(oracle.ints_to_limbs([1]))[0]
    assert E.ints(one) == [E.ONE] and (E.ONE + E.MINUS_ONE) % P == 0 and E.TOP == P - 1
    a, b = random_field(50, 1), random_field(50, 2)
    assert [E.mul(x, y) for x, y in zip(E.ints(a), E.ints(b))] == E.ints(oracle.binop("pko_fe_mul", a, b))
    assert np.array_equal(E.limbs(E.ints(a)), a)
    assert np.array_equal(E.periodic(7, [1, 2, 3]), E.limbs([1, 2, 3, 1, 2, 3, 1])) and np.array_equal(E.const(3, 5), E.limbs([5, 5, 5]))


@pytest.mark.parametrize("n", [1, 2, 255, 1000])
def test_stored_sum_and_the_dot_products_of_constants(oracle, n):
    a = random_field(n, 3 + n)
    a[0] = E.limbs([P - 1])[0]
    assert E.stored_sum(a) == sum(E.ints(a)) % P
    assert E.stored_sum(E.const(n, P - 1)) == (P - n) % P
    # w = p - 1, f = the field's one: every product is the stored value p - 1, the sum (p - n) mod p; g = two doubles it
    for w, f in ((E.TOP, E.ONE), (E.TOP, 2 * E.ONE % P), (P - 3, E.ONE), (P - 2, 2 * E.ONE % P)):
        want = sum(E.mul(w, f) for _ in range(n)) % P
        assert E.dot_of_constants(n, w, f) == want == E.ints(oracle.dot(E.const(n, w), E.const(n, f)))[0]
    assert E.dot_of_constants(n, E.TOP, E.ONE) == (P - n) % P and E.dot_of_constants(n, E.TOP, 2 * E.ONE % P) == (P - 2 * n) % P


@pytest.mark.parametrize("n", [1, 2, 9, 300])
def test_horner_closed_forms(oracle, n):
    c = random_field(n, 40 + n)
    ci = E.ints(c)
    closed = E.horner_closed_forms(c)
    for name, want in closed.items():
        z = E.CHALLENGES[name]
        assert want == E.horner(ci, z) == E.ints(oracle.eval_univariate(c, E.limbs([z])[0]))[0], (n, name)
    assert closed["zero"] == ci[0] and closed["one"] == sum(ci) % P
    assert closed["minus_one"] == sum(v if i % 2 == 0 else -v for i, v in enumerate(ci)) % P


def test_product_form_table_has_product_form_coefficients(oracle):
    """the identity the full-array to_coeffs checks rest on, at 4 variables: against the oracle's transform and a Python one"""
    xs = E.ints(random_field(4, 77))
    xs[1], xs[2] = 0, E.MINUS_ONE
    table = E.product_table_ints(xs)
    assert table[0b0101] == E.mul(xs[0], xs[2]) and table[0] == E.ONE
    want = E.product_table_coeffs_ints(xs)
    assert E.to_coeffs_ints(table) == want == E.ints(oracle.to_coeffs(E.limbs(table), 4))
    assert E.to_coeffs_ints([E.ONE] * 16) == [E.ONE] + [0] * 15


def test_grid_rule():
    for latency in (False, True):
        for items, blocks in E.geometry_items(latency).items():
            assert E.reduction_blocks(items, latency, 256) == blocks
    assert E.reduction_blocks(0, False, 256) == 1 and E.reduction_blocks(1 << 30, True, 8) == 32


@pytest.mark.parametrize("log_len", [1, 2, 3, 6])
@pytest.mark.parametrize("challenge", [None, "zero", "one", "top", "random"])
def test_grouped_sumcheck_definitions_equal_the_oracle(oracle, log_len, challenge):
    n = 1 << log_len
    arrs = [random_field(n, 10 * log_len + k) for k in range(4)]
    arrs[1][: n // 2] = arrs[1][n // 2:]  # repeated operands: groups of more than one item
    r = None if challenge is None else (E.ints(random_field(1, 5))[0] if challenge == "random" else E.CHALLENGES[challenge])
    rl = None if r is None else E.limbs([r])[0]
    if r is None or n >= 4:
        sums, folded = E.cubic_round(*arrs, r)
        want = oracle.sumcheck_cubic_round(*arrs, rl)
        assert sums == E.ints(want[0])
        if r is not None:
            for k in range(4):
                assert np.array_equal(folded[k], want[1 + k][: n // 2])
    if r is None or n >= 4:
        sums, folded = E.quadratic_round(arrs[0], arrs[1], r)
        want = oracle.sumcheck_quadratic_round(arrs[0], arrs[1], rl)
        assert sums == E.ints(want[0])
        if r is not None:
            assert np.array_equal(folded[0], want[1][: n // 2]) and np.array_equal(folded[1], want[2][: n // 2])


def test_grouped_folds_axpy_and_eq_equal_the_oracle(oracle):
    c = random_field(1 << 9, 8)
    c[:64] = E.const(64, P - 1)
    for k in (0, 1, 4, 8):
        r = random_field(max(k, 1), 9)[:k]
        assert np.array_equal(E.fold_coeffs(c, k, E.ints(r)), oracle.fold_coeffs(c, 9, r)), k
    r = E.ints(random_field(1, 3))[0]
    want = [E.fold(x0, x1, r) for x0, x1 in zip(E.ints(c[0::2]), E.ints(c[1::2]))]
    assert E.ints(E.fold_pairs(c, r)) == want
    assert E.fold(5, 9, 0) == 5 and E.fold(5, 9, E.ONE) == 9 and E.fold(5, 9, E.MINUS_ONE) == 1
    y, x = random_field(100, 1), random_field(100, 2)
    assert np.array_equal(E.axpy(y, r, x), oracle.vec_axpy(y, E.limbs([r])[0], x))
    pts, scales, w = random_field(3 * 5, 4).reshape(3, 5, 4), random_field(3, 5), random_field(32, 6)
    want = w.copy()
    for t in range(3):
        want = oracle.eq_accumulate_point(want, 5, pts[t], scales[t])
    assert E.eq_accumulate(E.ints(w), [E.ints(p) for p in pts], E.ints(scales)) == E.ints(want)
    assert E.eq_table_ints([E.ONE, 0, E.ONE]) == [E.ONE if i == 0b101 else 0 for i in range(8)]  # variable 0 is the top bit
