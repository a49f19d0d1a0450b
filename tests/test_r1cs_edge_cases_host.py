"""CPU: the systems of tests/r1cs_edge_cases.py are what tests/test_gpu_r1cs_edges.py assumes -- every case has exactly the heavy
lines it claims, in the line sets it claims (lengths, lines per set, chunks per line, all from the arrays alone), and its heavy
lines' sums differ pairwise in the oracle, so that a sum read from a wrong slot cannot pass.  The C oracle's sparse products, the
reference of every device comparison, are pinned against Python integers on the largest values, and so is the grouped dot product
every line goes through (csrc/fe29.hpp dot29), run on the host by the lab's pk_probe_dot29_host."""
import numpy as np
import pytest

import r1cs_edge_cases as E

P, RINV = E.P, E.RINV


def test_the_thresholds_are_the_ones_the_cases_straddle():
    from tools.pk_probes import r1cs_thresholds

    th = r1cs_thresholds()
    assert (th["HEAVY_DEGREE"], th["HEAVY_CHUNK"], th["DOT29_GROUP"]) == (64, 2048, 4) and th == E.THRESHOLDS
    assert th["RED_THREADS"] >= 64 and th["RED_THREADS"] % 64 == 0  # whole wavefronts; its value is csrc/reduce.hpp's to choose
    # the lengths of the all-(p-1) lines: both sides of every switch, every phase of a reduction group, a lane more or less per chunk
    T = E.RED_THREADS
    for t in list(range(10)) + [63, 64, 65, 2047, 2048, 2049, 4097, T - 1, T + 1, 2 * T - 1, 2 * T + 1]:
        assert t in E.PM1_LENGTHS
    assert {t % E.DOT29_GROUP for t in E.PM1_LENGTHS if t <= 9} == set(range(E.DOT29_GROUP))


def _all_cases():
    gens = [(f"pm1-{k}", g) for k, g in E.PM1_CASES.items()] + [(f"slot-{k}", g) for k, g in E.SLOT_CASES.items()]
    gens += [(f"strided-{nc}", (lambda nc=nc: E.strided_case(nc))) for nc in E.STRIDED_NCS]
    gens += [("ranges", E.range_case), ("satisfiable", E.satisfiable_case)] + [(f"degenerate-{k}", g) for k, g in E.DEGENERATE_CASES.items()]
    return gens


def _line_sums(oracle, case, s):
    m = case.mats[s % 3]
    x = case.z if s < 3 else case.eq[: case.nc]
    return oracle.spmv(case.nc, case.nw, m.new_row_indices, m.col_indices, m.values, case.interner, x, transpose=s >= 3)


@pytest.mark.parametrize("name,gen", _all_cases(), ids=[n for n, _ in _all_cases()])
def test_a_case_has_the_heavy_lines_it_claims_and_their_sums_differ(oracle, name, gen):
    from tools.pk_probes import r1cs_thresholds

    th = r1cs_thresholds()
    case = gen()
    assert len(case.mats) == 3 and case.z.shape == (case.nw, 4) and case.eq.shape == (max(case.nc, 1), 4)
    assert all(x < P for x in E.ints(case.interner) + E.ints(case.z) + E.ints(case.eq))
    sums = []
    for s in range(6):
        m = case.mats[s % 3]
        assert (m.num_rows, m.num_cols) == (case.nc, case.nw)
        assert m.nnz == 0 or (int(m.col_indices.max()) < case.nw and int(m.values.max()) < len(case.interner))
        lengths = E.line_lengths(case, s)
        assert len(lengths) == (case.nc if s < 3 else case.nw) and int(lengths.sum()) == m.nnz
        found = {int(i): int(lengths[i]) for i in np.nonzero(lengths > th["HEAVY_DEGREE"])[0]}
        assert found == case.heavy.get(s, {}), f"line set {s}"
        assert s not in case.heavy or case.heavy[s], "a set is listed only if it has heavy lines"
        for line, n in found.items():  # chunks per line, as pk_r1cs_create cuts them
            assert E.chunks_of(n) == len(range(0, n, th["HEAVY_CHUNK"])) >= 1
        if found:
            y = E.ints(_line_sums(oracle, case, s))
            sums += [y[i] for i in sorted(found)]
    assert len(set(sums)) == len(sums), "two heavy lines of the case have the same sum: a wrong slot could hide"
    for s, lines in case.expect.get("light", {}).items():  # lines right AT the threshold are not heavy
        lengths = E.line_lengths(case, s)
        assert all(int(lengths[i]) == n == th["HEAVY_DEGREE"] for i, n in lines.items())


def test_the_cases_cover_what_they_are_for():
    """one heavy line in all; only the first row; only the last row and column; every row; one set only, for each set that a case is
    named for; a set that is not the first with empty sets before it; chunk counts 1, 2 and 3"""
    c = {k: g() for k, g in E.SLOT_CASES.items()}
    assert c["one_heavy_line"].heavy == {0: {5: 65}}
    assert all(set(c["heavy_first_row"].heavy[s]) == {0} for s in range(3)) and set(c["heavy_first_row"].heavy) == {0, 1, 2}
    last = c["heavy_last_row_and_col"]
    assert set(last.heavy) == set(range(6)) and all(set(last.heavy[s]) == {last.nc - 1} for s in range(3)) and all(set(last.heavy[s]) == {last.nw - 1} for s in (3, 4, 5))
    assert all(set(c["every_row_heavy"].heavy[s]) == set(range(300)) for s in range(3)) and set(c["every_row_heavy"].heavy) == {0, 1, 2}
    for k, s in (("heavy_rows_A_only", 0), ("heavy_rows_B_only", 1), ("heavy_rows_C_only", 2), ("heavy_cols_C_only", 5)):
        assert set(c[k].heavy) == {s} and len(c[k].heavy[s]) >= 3
    assert set(c["heavy_rows_A_cols_C"].heavy) == {0, 5}
    assert c["len64_next_to_len65"].heavy == {0: {11: 65}, 4: {21: 65}}
    assert {E.chunks_of(n) for n in c["heavy_rows_A_only"].heavy[0].values()} == {1, 2}
    assert sorted(E.chunks_of(t) for t in E.PM1_LENGTHS if t > 64) == [1, 1, 1, 1, 1, 1, 1, 2, 3]
    for k, g in E.PM1_CASES.items():
        case = g()
        assert set(case.heavy) == {case.expect["set"]} and len(case.heavy[case.expect["set"]]) == 9
    assert sorted(g().expect["set"] for g in E.PM1_CASES.values()) == list(range(6))
    sat = E.satisfiable_case()
    assert {s: sorted(v) for s, v in sat.heavy.items()} == {0: [7, 256, 599], 1: [256, 300], 2: [300, 599]}
    for nc in E.STRIDED_NCS:
        assert set(E.strided_case(nc).heavy) == {0, 1}
    assert set(E.range_case().heavy) == {3, 4, 5}


def _py_spmv(m, nc, nw, interner, x, transpose):
    """the sparse product as the device forms it, in Python integers: y = sum value * x / 2^256 mod p"""
    y = [0] * (nw if transpose else nc)
    nri = [int(v) for v in m.new_row_indices] + [m.nnz]
    for i in range(nc):
        for k in range(nri[i], nri[i + 1]):
            c, v = int(m.col_indices[k]), interner[int(m.values[k])]
            if transpose:
                y[c] = (y[c] + v * x[i]) % P
            else:
                y[i] = (y[i] + v * x[c]) % P
    return [v * RINV % P for v in y]


@pytest.mark.parametrize("name", ["A_rows", "B_cols"])
def test_the_oracle_products_on_the_largest_values(oracle, name):
    """oracle.spmv, both directions, on matrices whose every entry is p - 1 against vectors of p - 1: the C oracle has only ever seen
    random values, and everything on the device is compared with it"""
    case = E.PM1_CASES[name]()
    it, z, eq = E.ints(case.interner), E.ints(case.z), E.ints(case.eq)
    s = case.expect["set"]
    for k, m in enumerate(case.mats):
        rows = E.ints(oracle.spmv(case.nc, case.nw, m.new_row_indices, m.col_indices, m.values, case.interner, case.z))
        assert rows == _py_spmv(m, case.nc, case.nw, it, z, False)
        cols = E.ints(oracle.spmv(case.nc, case.nw, m.new_row_indices, m.col_indices, m.values, case.interner, case.eq, transpose=True))
        assert cols == _py_spmv(m, case.nc, case.nw, it, eq, True)
        if k == s % 3:  # the lines of every length: t (p-1)^2 / 2^256
            got = cols if s >= 3 else rows
            assert all(got[i] == E.pm1_value(t) for i, t in case.expect["lengths"].items())
            assert all(v == 0 for i, v in enumerate(got) if i not in case.expect["lengths"])
    a, b = (oracle.spmv(case.nc, case.nw, m.new_row_indices, m.col_indices, m.values, case.interner, case.z) for m in case.mats[:2])
    assert E.ints(oracle.hadamard(a, b)) == [x * y * RINV % P for x, y in zip(E.ints(a), E.ints(b))]


# ---- fe29.hpp dot29 on the host -----------------------------------------------------------------------------------------------------
TERM_COUNTS = list(range(14)) + [63, 64, 65, 2049]


def _dot(a, b):
    from tools.pk_probes import dot29_host

    assert len(a) == len(b)
    got = E.ints(dot29_host(E.limbs(a) if a else np.zeros((0, 4), np.uint64), E.limbs(b) if b else np.zeros((0, 4), np.uint64)))[0]
    assert got == sum(x * y for x, y in zip(a, b)) * RINV % P, f"{len(a)} terms"


@pytest.mark.parametrize("terms", TERM_COUNTS)
def test_dot29_of_the_largest_operands(terms):
    """every product the largest a line can hold, the count ending in every phase of a reduction group and past the heavy threshold
    and a chunk: the running sum's bound (fe29.hpp dot29_flush) is derived by hand and holds here or nowhere"""
    _dot([P - 1] * terms, [P - 1] * terms)


@pytest.mark.parametrize("terms", TERM_COUNTS)
def test_dot29_of_random_operands(terms):
    rng = np.random.default_rng(700 + terms)
    a, b = ([int.from_bytes(rng.bytes(32), "little") % P for _ in range(terms)] for _ in range(2))
    _dot(a, b)


def test_dot29_of_zeros_and_ones():
    for terms in (1, 3, 4, 5, 8, 9):
        for x, y in ((0, 0), (0, 1), (1, 0), (1, 1), (0, P - 1), (P - 1, 0), (1, P - 1), (P - 1, 1), (E.R, E.R)):
            _dot([x] * terms, [y] * terms)
    _dot([0, 1, P - 1, 1, 0, E.R, P - 1], [P - 1, 1, 0, 0, 1, E.R, P - 1])


@pytest.mark.parametrize("at", range(9))
def test_dot29_takes_one_unreduced_first_factor_among_reduced_ones(at):
    """fe29.hpp: "single such terms among reduced ones stay inside the bound" -- one first factor of 2^256 - 1 at each position of a
    run of nine p - 1 (two full groups and a term) still gives the exact sum.  (pk_r1cs_create refuses such interned values; this
    pins the comment's claim, not a supported input.)"""
    a = [P - 1] * 9
    a[at] = (1 << 256) - 1
    _dot(a, [P - 1] * 9)
