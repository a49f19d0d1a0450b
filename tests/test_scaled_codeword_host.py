"""CPU: every consumer of a stored hash-ready codeword element (PK_LEAVES_SCALED32: the leaf fold's compress29s, from_scaled_canon,
the two routes of opened_element -- csrc/skyscraper29s.hpp) as the HOST build of the exact device source, through pk_selftest_arith
ops 39 .. 43, against Python integers and the oracle's compress_many, on the stored values of tests/scaled_codeword_cases.py: the
whole range [0, 8p/5) the encoding allows, with the edges at p, at the producer's bound and at every exact division by 32.
Bit-exact; tests/test_gpu_scaled_codeword.py runs the same ops over the same operands on the device."""
import numpy as np
import pytest

import scaled_codeword_cases as sc

P = sc.P


def run(op, xs, ys=None):
    from provekit_amd._lib import lib

    a = sc.to_limbs(xs)
    b = sc.to_limbs(ys) if ys is not None else None
    out = np.empty_like(a)
    assert lib.pk_selftest_arith(op, a.ctypes.data, b.ctypes.data if b is not None else None, out.ctypes.data, a.shape[0]) == 0
    return sc.from_limbs(out)


def mismatches(got, want, xs, ys):
    return [(hex(x), hex(y), hex(g), hex(w)) for x, y, g, w in zip(xs, ys, got, want) if g != w][:4]


def fold_of_three(oracle, xs, ys):
    """op 41: the digest of the width-4 leaf (x, y, x, y)"""
    return sc.leaf_digests(oracle, [(x, y, x, y) for x, y in zip(xs, ys)], 2)


def test_the_cases_cover_the_range_the_encoding_states():
    """on the ints alone, and against the one statement of the range in csrc/skyscraper29s.hpp (read through the lab)"""
    from tools.pk_probes import lib as probes

    cov = sc.coverage()
    assert cov["{p}"] == 1 and cov["not below B"] == 0
    assert cov["[0, p)"] > sc.N_RANDOM and cov["(p, p + (p >> 10))"] > sc.N_RANDOM and cov["[p + (p >> 10), B)"] > sc.N_RANDOM // 2
    bound, most = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    assert probes.pk_probe_scaled32_bounds(bound.ctypes.data, most.ctypes.data) == 0
    assert sc.from_limbs(bound) == [sc.B] and sc.from_limbs(most) == [sc.PRODUCER_MAX]
    assert sc.B == 8 * P // 5 and P < sc.PRODUCER_MAX < 105 * P // 100 < 6 * P // 5 < sc.B < sc.R
    must = {0, 1, 31, 32, 33, P - 1, P, P + 1, P + 31, P + 32, P + 33, sc.ALMOST - 1, sc.ALMOST, sc.B - 1,
            105 * P // 100 - 1, 105 * P // 100 + 1, 6 * P // 5 - 1, 6 * P // 5 + 1}
    assert must <= set(sc.NAMED) and len(sc.NAMED) == len(must) + 2
    ones, zeros = sc.NAMED[-2:]  # limbs 0..7 all ones / all zero under the largest top limb
    assert ones & ((1 << 232) - 1) == (1 << 232) - 1 and ones < sc.B <= ones + (1 << 232)
    assert zeros & ((1 << 232) - 1) == 0 and zeros < sc.B <= zeros + (1 << 232)
    # the exact-division edges: a value on either side of every k p / 32, each stored below p and (where that stays below B) above
    values = {sc.value(x) for x in sc.EDGES}
    for k in range(1, 32):
        assert {k * P // 32, k * P // 32 + 1} <= values, k
        assert 32 * (k * P // 32 + 1) % P + P in sc.EDGES, k
    assert {0, 1, P - 1} <= values
    # the constructed leaves put every edge value at a fold's seed and at a later element
    seeds, later = sc.leaf_coverage()
    assert set(sc.EDGES) <= seeds and set(sc.EDGES) <= later
    assert len(sc.EDGES) <= 255  # so that the opening tests' 256-leaf buffers hold all of them in every column


@pytest.mark.parametrize("op,define", [(42, sc.canonical_opening), (43, sc.montgomery_opening)], ids=["canonical", "montgomery"])
def test_openings_of_every_case(op, define):
    xs = list(sc.CASES)
    want = [define(x) for x in xs]
    assert mismatches(run(op, xs), want, xs, xs) == []
    assert run(op, xs, xs[::-1]) == want  # a one-operand op: the second operand is ignored


@pytest.mark.parametrize("op,version", [(39, 2), (40, 1)], ids=["v2", "v1"])
def test_raw_compress_of_every_pair_and_every_case(oracle, op, version):
    """compress29s as the leaf fold enters it: unpack29<0> of the stored words on both sides, no to_scaled29"""
    xs, ys = sc.pair_operands()
    assert len(xs) == 40 * 40 + len(sc.CASES)
    want = sc.compress(oracle, [sc.value(x) for x in xs], [sc.value(y) for y in ys], version)
    assert mismatches(run(op, xs, ys), want, xs, ys) == []


def test_raw_fold_of_three(oracle):
    """three compressions without leaving the scaled domain: the stored element is the seed, then the right input twice over"""
    xs, ys = sc.pair_operands()
    assert mismatches(run(41, xs, ys), fold_of_three(oracle, xs, ys), xs, ys) == []


def test_the_new_ops_end_the_table_and_the_folds_need_both_operands():
    from provekit_amd._lib import lib

    a = sc.to_limbs([1, P])
    out = np.empty_like(a)
    for op in (39, 40, 41, 42, 43):
        assert (lib.pk_selftest_arith(op, a.ctypes.data, None, out.ctypes.data, 2) == 0) == (op in (42, 43)), op
    assert lib.pk_selftest_arith(44, a.ctypes.data, a.ctypes.data, out.ctypes.data, 2) != 0


def test_the_stored_form_is_not_the_to_scaled29_form():
    """why ops 39 .. 43 exist: ops 15 .. 19 enter through to_scaled29, which multiplies by 32 and reduces -- run on the same stored
    words they compute the hash of 32 times the value, and their input never reaches compress29s at or above 1.04p"""
    xs, ys = list(sc.PAIR_SAMPLE), list(sc.PAIR_SAMPLE[1:] + sc.PAIR_SAMPLE[:1])
    assert run(15, xs, ys) != run(39, xs, ys)
    assert run(17, xs) == [x % P for x in xs] != [sc.value(x) for x in xs]
