"""R1CS systems aimed at the places where csrc/r1cs.hip changes path: the line length above which a line is summed by workgroups
(HEAVY_DEGREE), the entries per workgroup of such a line (HEAVY_CHUNK), the phases of a reduction group of its dot product
(DOT29_GROUP), the lanes a chunk is strided by (RED_THREADS), the slot numbering of the heavy lines through the six line sets
(0..2: rows of A, B, C; 3..5: their columns), the shards of the sharded prover, and the largest values a line can hold.

Every generator returns a Case: three SparseMatrix, the interner, z (num_witnesses elements) and eq (num_constraints elements, at
least one), all Montgomery images as (n, 4) u64 arrays, and `heavy`: for each line set that has heavy lines, {line: length}.
tests/test_r1cs_edge_cases_host.py checks that claim from the arrays alone, and that the heavy lines' sums differ pairwise;
tests/test_gpu_r1cs_edges.py runs the cases on the device.  Nothing here touches a GPU."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from tools.pk_probes import r1cs_thresholds

# the values the cases are aimed at (csrc/r1cs_shape.hpp, fe29.hpp); both test files compare them with the library's before they run a
# case.  RED_THREADS is taken as it is: csrc/reduce.hpp is its one source, and the lengths below follow it
HEAVY_DEGREE, HEAVY_CHUNK, DOT29_GROUP = 64, 2048, 4
RED_THREADS = r1cs_thresholds()["RED_THREADS"]
THRESHOLDS = {"HEAVY_DEGREE": HEAVY_DEGREE, "HEAVY_CHUNK": HEAVY_CHUNK, "DOT29_GROUP": DOT29_GROUP, "RED_THREADS": RED_THREADS}
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R = (1 << 256) % P  # the Montgomery image of one
RINV = pow(1 << 256, -1, P)


def limbs(xs) -> np.ndarray:
    xs = [int(x) for x in xs]
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype="<u8").reshape(len(xs), 4).astype(np.uint64)


def ints(a) -> list:
    b = np.ascontiguousarray(a, dtype="<u8").reshape(-1, 4).tobytes()
    return [int.from_bytes(b[32 * i : 32 * i + 32], "little") for i in range(len(b) // 32)]


@dataclass
class Case:
    name: str
    nc: int
    nw: int
    mats: tuple  # (A, B, C)
    interner: np.ndarray
    z: np.ndarray
    eq: np.ndarray
    heavy: dict  # line set -> {line: length}, only the sets that have heavy lines
    expect: dict = field(default_factory=dict)

    @property
    def m0(self) -> int:
        return (self.nc - 1).bit_length() if self.nc else 0


def line_lengths(case: Case, s: int) -> np.ndarray:
    """the lengths of the lines of set s, from the arrays alone"""
    m = case.mats[s % 3]
    if s < 3:
        return np.diff(np.concatenate([m.new_row_indices.astype(np.int64), [m.nnz]]))
    return np.bincount(m.col_indices.astype(np.int64), minlength=case.nw)[: case.nw]


def chunks_of(length: int) -> int:
    return -(-length // HEAVY_CHUNK)


def _matrix(nc, nw, rows):
    """rows[i] = [(column, interner index)], any order -> SparseMatrix with the columns of a row ascending"""
    from provekit_amd.sparse_matrix import SparseMatrix

    nri, ci, vv = [], [], []
    for r in rows:
        nri.append(len(ci))
        for c, v in sorted(r):
            ci.append(c)
            vv.append(v)
    return SparseMatrix(nc, nw, np.array(nri, np.uint32), np.array(ci, np.uint32), np.array(vv, np.uint32))


def _claim(rows, cols):
    heavy = {}
    for m, i, n in rows:
        if n > HEAVY_DEGREE:
            heavy.setdefault(m, {})[i] = n
    for m, j, n in cols:
        if n > HEAVY_DEGREE:
            heavy.setdefault(3 + m, {})[j] = n
    return heavy


def _entries(rng, nc, nw, rows, cols, fill, n_interned):
    """three matrices as entry lists: row i of matrix m has n entries for (m, i, n) in rows, column j of matrix m has n for (m, j, n)
    in cols; the other rows get fill[0] .. fill[1] - 1 entries, in columns no entry of cols names (so those columns hold exactly
    what was asked for); a column's entries avoid the rows that rows names (so do those rows)"""
    out = []
    for m in range(3):
        asked_rows = {i: n for mm, i, n in rows if mm == m}
        asked_cols = [(j, n) for mm, j, n in cols if mm == m]
        free = np.array(sorted(set(range(nw)) - {j for j, _ in asked_cols}), dtype=np.int64)
        ent = []
        for i in range(nc):
            n = asked_rows.get(i)
            if n is None:
                n = int(rng.integers(fill[0], fill[1]))
            assert n <= len(free)
            ent.append({int(c) for c in rng.choice(free, size=n, replace=False)})
        plain = np.array([i for i in range(nc) if i not in asked_rows], dtype=np.int64)
        for j, n in asked_cols:
            assert n <= len(plain)
            for i in rng.choice(plain, size=n, replace=False):
                ent[int(i)].add(j)
        out.append([[(c, int(rng.integers(0, n_interned))) for c in sorted(r)] for r in ent])
    return out


def _system(name, nc, nw, seed, rows=(), cols=(), fill=(0, 5), n_interned=17, expect=None) -> Case:
    from provekit_amd.field import random_field

    rng = np.random.default_rng(seed)
    ent = _entries(rng, nc, nw, rows, cols, fill, n_interned)
    mats = tuple(_matrix(nc, nw, e) for e in ent)
    return Case(name, nc, nw, mats, random_field(n_interned, seed + 1), random_field(nw, seed + 2), random_field(max(nc, 1), seed + 3),
                _claim(rows, cols), dict(expect or {}))


# ---- 1. the largest addends ---------------------------------------------------------------------------------------------------------
# one line of each length: 0 .. 9 end in every phase of a reduction group twice over; 63, 64, 65 straddle HEAVY_DEGREE; 2047, 2048, 2049
# and 4097 straddle one and two chunks; RED_THREADS -+ 1 and 2 RED_THREADS -+ 1 give the lanes of a chunk one term more or less
PM1_LENGTHS = sorted(set(list(range(10)) + [63, 64, 65, 2047, 2048, 2049, 4097] + [RED_THREADS - 1, RED_THREADS + 1, 2 * RED_THREADS - 1, 2 * RED_THREADS + 1]))


def pm1_case(matrix: int, transposed: bool) -> Case:
    """interner {p - 1, 0, R}; every entry, every element of z and of eq is p - 1.  Matrix `matrix` has one row (transposed: one
    column) of every length of PM1_LENGTHS, line i of length PM1_LENGTHS[i] over the first columns (rows); the two other matrices
    hold the same lines as far as they have at most 9 entries.  So only line set matrix + 3 * transposed has heavy lines, their
    lengths differ, and with them their sums t (p-1)^2 / 2^256"""
    n = max(PM1_LENGTHS)
    full = {i: t for i, t in enumerate(PM1_LENGTHS)}
    short = {i: t for i, t in full.items() if t <= 9}

    def build(lengths):
        if not transposed:
            rows = [[(c, 0) for c in range(lengths.get(i, 0))] for i in range(n)]
        else:
            rows = [[(j, 0) for j, t in lengths.items() if t > i] for i in range(n)]
        return _matrix(n, n, rows)

    mats = tuple(build(full if m == matrix else short) for m in range(3))
    pm1 = limbs([P - 1] * n)
    s = matrix + 3 * int(transposed)
    return Case(f"pm1_{'ABC'[matrix]}{'_cols' if transposed else '_rows'}", n, n, mats, limbs([P - 1, 0, R]), pm1, pm1.copy(),
                {s: {i: t for i, t in full.items() if t > HEAVY_DEGREE}}, {"set": s, "lengths": dict(full), "short": dict(short)})


PM1_CASES = {f"{'ABC'[m]}{'_cols' if t else '_rows'}": (lambda m=m, t=t: pm1_case(m, t)) for t in (False, True) for m in range(3)}


def pm1_value(t: int) -> int:
    """a line of t entries p - 1 against p - 1, as the device forms it: the sum of t Montgomery products"""
    return t * (P - 1) * (P - 1) * RINV % P


# ---- 2. the heavy-slot lookup -----------------------------------------------------------------------------------------------------
def _abc(i, base):
    return [(m, i, base + 7 * m) for m in range(3)]


SLOT_CASES = {
    "one_heavy_line": lambda: _system("one_heavy_line", 40, 100, 101, rows=[(0, 5, 65)]),
    "heavy_first_row": lambda: _system("heavy_first_row", 300, 320, 102, rows=_abc(0, 65)),
    "heavy_last_row_and_col": lambda: _system("heavy_last_row_and_col", 300, 310, 103, rows=_abc(299, 66), cols=_abc(309, 80)),
    "every_row_heavy": lambda: _system("every_row_heavy", 300, 2000, 104, rows=[(m, i, 65) for m in range(3) for i in range(300)]),
    "heavy_rows_A_only": lambda: _system("heavy_rows_A_only", 300, 2100, 105, rows=[(0, 3, 65), (0, 100, 100), (0, 257, 2049), (0, 299, 70)]),
    "heavy_rows_B_only": lambda: _system("heavy_rows_B_only", 300, 2100, 106, rows=[(1, 0, 66), (1, 255, 2048), (1, 256, 90), (1, 298, 71)]),
    "heavy_rows_C_only": lambda: _system("heavy_rows_C_only", 300, 2100, 107, rows=[(2, 1, 67), (2, 2, 2050), (2, 200, 65), (2, 299, 72)]),
    "heavy_cols_C_only": lambda: _system("heavy_cols_C_only", 300, 320, 108, cols=[(2, 0, 65), (2, 7, 300), (2, 319, 100)]),
    # sets 1, 2, 3, 4 empty between two that are not: slot0 of set 5 is the number of heavy rows of A
    "heavy_rows_A_cols_C": lambda: _system("heavy_rows_A_cols_C", 300, 320, 109, rows=[(0, 4, 65), (0, 150, 200), (0, 299, 80)],
                                            cols=[(2, 3, 66), (2, 160, 120)]),
    "len64_next_to_len65": lambda: _system("len64_next_to_len65", 300, 320, 110, rows=[(0, 10, 64), (0, 11, 65)], cols=[(1, 20, 64), (1, 21, 65)],
                                            expect={"light": {0: {10: 64}, 4: {20: 64}}}),
}


# ---- 3. strided witness bounds ------------------------------------------------------------------------------------------------------
STRIDES = (1, 2, 4, 8, 16)
# nc = 2^m, 2^m - 1, 2^(m-1) + 1 for m = 9 (more than one workgroup of outputs at stride 1) and m = 4 (stride 16: one output), and 1
STRIDED_NCS = (512, 511, 257, 16, 15, 9, 1)


def strided_case(nc: int) -> Case:
    """heavy rows of A and B at the first rows, on both sides of the first workgroup's end and at the last row"""
    at = sorted({i for i in (0, 1, 255, 256, nc - 1) if 0 <= i < nc})
    rows = [(0, i, 65 + 3 * k) for k, i in enumerate(at)] + [(1, i, 150 + 5 * k) for k, i in enumerate(at) if i != 1]
    return _system(f"strided_{nc}", nc, 320, 300 + nc, rows=rows, fill=(1, 5))


# ---- 4. ranges of the external rows -----------------------------------------------------------------------------------------------
def range_case() -> Case:
    """heavy columns at the first and last column, on both sides of 256 and 512 and of the four blocks' seams (150, 300, 450)"""
    cols = [(0, 0, 65), (0, 255, 100), (0, 256, 70), (0, 599, 300), (1, 1, 66), (1, 257, 90), (1, 511, 75), (1, 512, 80), (2, 149, 67),
            (2, 150, 68), (2, 449, 76), (2, 450, 85)]
    return _system("ranges", 300, 600, 400, cols=cols)


def ranges(nw: int, k: int = 77):
    return [(0, 0), (k, k), (0, nw), (1, nw), (255, 257), (256, 512), (nw - 1, nw + 1000), (nw, nw + 5)]


# ---- 5. satisfaction ----------------------------------------------------------------------------------------------------------------
def satisfiable_case() -> Case:
    """600 constraints over 400 inputs and 600 outputs.  A and B read inputs only.  Row i of C reads a few inputs and, with
    coefficient one, output i, which no other entry reads: output i = (A z)_i (B z)_i - (the rest of row i of C) . z makes the system
    satisfied, and adding one to output i breaks row i alone.  Heavy rows: A 7, 256, 599; B 256, 300; C 300, 599.  Input 399 is read
    only by row 7 of A (the one heavy matrix of that row), input 398 only by row 300 of C: changing either breaks that row alone, and
    the change reaches the check only through the heavy line's sum"""
    import oracle_lib as oracle

    from provekit_amd.field import random_field

    nc, n_in, seed = 600, 400, 500
    nw = n_in + nc
    rng = np.random.default_rng(seed)
    rows = [(0, 7, 80), (0, 256, 70), (0, 599, 300), (1, 256, 65), (1, 300, 100), (2, 300, 90), (2, 599, 120)]
    ent = _entries(rng, nc, n_in - 2, rows, (), (1, 4), 17)  # inputs 0 .. 397; interner index 0 is kept for the coefficient one
    ent = [[[(c, 1 + v % 16) for c, v in r] for r in e] for e in ent]
    priv_a, priv_c = n_in - 1, n_in - 2
    ent[0][7].append((priv_a, 3))
    ent[2][300].append((priv_c, 5))
    c_inputs = _matrix(nc, nw, ent[2])
    for i in range(nc):
        ent[2][i].append((n_in + i, 0))
    mats = tuple(_matrix(nc, nw, e) for e in ent)
    interner = random_field(17, seed + 1)
    interner[0] = limbs([R])[0]
    z = np.zeros((nw, 4), np.uint64)
    z[:n_in] = random_field(n_in, seed + 2)
    a, b = (oracle.spmv(nc, nw, m.new_row_indices, m.col_indices, m.values, interner, z) for m in mats[:2])
    rest = oracle.spmv(nc, nw, c_inputs.new_row_indices, c_inputs.col_indices, c_inputs.values, interner, z)
    z[n_in:] = limbs([(x - y) % P for x, y in zip(ints(oracle.hadamard(a, b)), ints(rest))])
    heavy = _claim([(m, i, n + (1 if (m, i) in ((0, 7), (2, 300)) else 0) + (1 if m == 2 else 0)) for m, i, n in rows], ())
    return Case("satisfiable", nc, nw, mats, interner, z, random_field(nc, seed + 3), heavy,
                {"n_in": n_in, "priv_a": (priv_a, 7), "priv_c": (priv_c, 300), "heavy_c_row": 599, "only_a_heavy_row": 7})


def corrupt(z: np.ndarray, column: int) -> np.ndarray:
    """z with one added to element `column`"""
    out = z.copy()
    out[column] = limbs([(ints(z[column])[0] + 1) % P])[0]
    return out


# ---- 6. degenerate shapes -----------------------------------------------------------------------------------------------------------
def _bare(name, nc, nw, n_interned) -> Case:
    from provekit_amd.field import random_field

    mats = tuple(_matrix(nc, nw, [[] for _ in range(nc)]) for _ in range(3))
    it = random_field(n_interned, 601) if n_interned else np.zeros((0, 4), np.uint64)
    return Case(name, nc, nw, mats, it, random_field(max(nw, 1), 602), random_field(max(nc, 1), 603), {})


DEGENERATE_CASES = {
    "no_entries": lambda: _bare("no_entries", 5, 7, 3),
    "no_constraints": lambda: _bare("no_constraints", 0, 6, 2),
    "no_interned_values": lambda: _bare("no_interned_values", 3, 4, 0),
    "one_row_m0_zero": lambda: _system("one_row_m0_zero", 1, 80, 604, rows=[(0, 0, 3), (1, 0, 65), (2, 0, 1)]),
}
