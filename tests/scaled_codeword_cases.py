"""Stored elements of the hash-ready codeword (PK_LEAVES_SCALED32, csrc/skyscraper29s.hpp "the hash-ready codeword") and what every
consumer must make of them.  A stored x is the plain integer 32 v mod p, lazily reduced: any x below B = floor(8 p / 5) is legal, the
commit's own NTT stays at or below PRODUCER_MAX = p + (p >> 10).  Random codewords put an element at or above p in front of a consumer
about once in a thousand elements and never at an edge; the cases here put every edge there.

The reference is Python integers: the value v = x / 32 mod p; the canonical opening v; the Montgomery opening v 2^256 mod p; the
leaf digest h = v_0, h = C(h, v_j) with C the oracle's compress_many on canonical bytes (the digest of a width-1 leaf is v_0).

Plain ints, seeded, no import of the library: tests/test_scaled_codeword_host.py (CPU) and tests/test_gpu_scaled_codeword.py (device)
take the same operands and the same expected values from here."""
import random

import numpy as np

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R = 1 << 256
INV32 = pow(32, -1, P)
B = 8 * P // 5                # what every consumer takes (exclusive): skyscraper29s.hpp SCALED32_BOUND_NUM / _DEN
PRODUCER_MAX = P + (P >> 10)  # what the commit stores (inclusive): reduce_almost29's p (1 + 2^-10), SCALED32_PRODUCER_SHIFT
ALMOST = PRODUCER_MAX         # the edge between the band the producer reaches and the band only a caller's buffer can hold
M29 = (1 << 29) - 1
N_RANDOM = 2000


def to_limbs(xs):
    xs = list(xs)
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u8").reshape(len(xs), 4).copy()


def from_limbs(a):
    b = np.ascontiguousarray(a, dtype="<u8").reshape(-1, 4).tobytes()
    return [int.from_bytes(b[32 * i: 32 * i + 32], "little") for i in range(len(b) // 32)]


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def value(x):
    return x * INV32 % P


def canonical_opening(x):
    return value(x)


def montgomery_opening(x):
    return value(x) * R % P


def compress(oracle, ls, rs, version):
    """C(l, r) of canonical values, element by element, through the oracle's compress_many"""
    msgs = b"".join(int(l).to_bytes(32, "little") + int(r).to_bytes(32, "little") for l, r in zip(ls, rs))
    out = oracle.compress_many(msgs, version)
    return [int.from_bytes(out[32 * i: 32 * i + 32], "little") for i in range(len(out) // 32)]


def leaf_digests(oracle, rows, version):
    """rows: n leaves of w stored elements each -> the n digests (ints): h = v_0; h = C(h, v_j)"""
    h = [value(row[0]) for row in rows]
    for j in range(1, len(rows[0])):
        h = compress(oracle, h, [value(row[j]) for row in rows], version)
    return h


# ---- the stored values -----------------------------------------------------------------------------------------------------------
def _named():
    top_ones = B >> 232  # limbs 0..7 all ones, the largest top limb that stays below B
    if (top_ones << 232) | ((1 << 232) - 1) >= B:
        top_ones -= 1
    return [0, 1, 31, 32, 33, P - 1, P, P + 1, P + 31, P + 32, P + 33,
            ALMOST - 1, ALMOST, 105 * P // 100 - 1, 105 * P // 100 + 1, 6 * P // 5 - 1, 6 * P // 5 + 1, B - 1,
            (top_ones << 232) | ((1 << 232) - 1), ((B - 1) >> 232) << 232]


def _division_edges():
    """32 v mod p and 32 v mod p + p where from_scaled_canon's division by 32 is at an edge: v in {0, 1, p - 1} and on either side of
    every k p / 32 (the stored value wraps there: 32 floor(k p / 32) mod p is just below p, 32 ceil(k p / 32) mod p just above 0)"""
    vs = [0, 1, P - 1]
    for k in range(1, 32):
        vs += [k * P // 32, -(-k * P // 32)]
    out = []
    for v in vs:
        out += [32 * v % P, 32 * v % P + P]
    return out


def _keep(xs):
    seen, out = set(), []
    for x in xs:
        if 0 <= x < B and x < R and x not in seen:
            seen.add(x)
            out.append(x)
    return tuple(out)


NAMED = _keep(_named())
EDGES = _keep(list(NAMED) + _division_edges())
_rnd = random.Random(0x5CA1ED32)
RANDOM = tuple([_rnd.randrange(P) for _ in range(N_RANDOM)] + [_rnd.randrange(P, ALMOST) for _ in range(N_RANDOM)]
               + [_rnd.randrange(P, B) for _ in range(N_RANDOM)])
CASES = EDGES + RANDOM

# the sample the two-operand ops take every pair of: the named values and twenty of the division edges
PAIR_SAMPLE = tuple(list(NAMED) + random.Random(40).sample([x for x in EDGES if x not in NAMED], 40 - len(NAMED)))


def coverage(xs=CASES):
    return {"[0, p)": sum(x < P for x in xs), "{p}": sum(x == P for x in xs), "(p, p + (p >> 10))": sum(P < x < ALMOST for x in xs),
            "[p + (p >> 10), B)": sum(ALMOST <= x < B for x in xs), "not below B": sum(not 0 <= x < B for x in xs)}


_cov = coverage()
assert all(_cov[band] >= 1 for band in ("[0, p)", "{p}", "(p, p + (p >> 10))", "[p + (p >> 10), B)")), _cov
assert _cov["not below B"] == 0 and B < R and PRODUCER_MAX < B, _cov
assert len(PAIR_SAMPLE) == 40 and len(set(PAIR_SAMPLE)) == 40 and set(PAIR_SAMPLE) <= set(EDGES)


def pair_operands():
    """xs, ys: every pair of PAIR_SAMPLE, then every case against a neighbour of the list (each case once on either side)"""
    xs = [x for x in PAIR_SAMPLE for _ in PAIR_SAMPLE] + list(CASES)
    ys = [y for _ in PAIR_SAMPLE for y in PAIR_SAMPLE] + list(CASES[7:] + CASES[:7])
    return xs, ys


# ---- constructed codewords -------------------------------------------------------------------------------------------------------
def leaf_matrix(n, w, salt=0):
    """n leaves of w stored elements (a list of rows).  The first len(EDGES) leaves walk the edge list in every column, each column
    from its own start, so from len(EDGES) leaves up every edge value is some leaf's element 0 (the fold's seed) and, from width 2, some
    leaf's later element; the leaves behind them take the random values."""
    E, Q = len(EDGES), len(RANDOM)
    return [[EDGES[(i + 7 * j + salt) % E] if i < E else RANDOM[(i * w + j + salt) % Q] for j in range(w)] for i in range(n)]


def column_major(rows):
    """rows (n x w ints) -> the (w, n, 4) u64 array a column-major codeword buffer holds"""
    n, w = len(rows), len(rows[0])
    return to_limbs(rows[i][j] for j in range(w) for i in range(n)).reshape(w, n, 4)


def leaf_major(rows):
    n, w = len(rows), len(rows[0])
    return to_limbs(x for row in rows for x in row).reshape(n, w, 4)


# the shapes of the constructed leaf-hash test, and what they must reach between them
LEAF_WIDTHS = (1, 2, 3, 32, 33)
LEAF_COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)


def leaf_coverage():
    seeds, later = set(), set()
    for w in LEAF_WIDTHS:
        for n in LEAF_COUNTS:
            for row in leaf_matrix(n, w, salt=w):
                seeds.add(row[0])
                later.update(row[1:])
    return seeds, later
