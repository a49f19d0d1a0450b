"""Operands that drive the field's carry chains (csrc/fe.hpp and the final subtractions written with the same add-/subtract-with-
carry builtins in fe29.hpp, skyscraper29s.hpp, reduce.hpp) into the cases random values reach with probability 2^-32 per word: a
carry riding through words whose sums are all ones, a borrow riding through equal words, results at 0, p - 1, p, p + 1, and values
that agree with the subtrahend in their upper limbs and differ by one further down (where the deciding borrow is made).

Plain Python ints, seeded, no import of the library: tests/test_fe_carry_host.py (CPU) and tests/test_gpu_fe_carry.py (device) take
the same operands and the same expected values from here.  Every case set is built once and returned as a tuple."""
import functools
import random

import numpy as np

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R = 1 << 256
RINV = pow(R, -1, P)
TOP = R - 1
M32 = (1 << 32) - 1
P7 = P >> 224  # p's top word: a value whose word 7 is below it is below p whatever its other words hold


def to_limbs(xs):
    xs = list(xs)
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u8").reshape(len(xs), 4).copy()


def from_limbs(a):
    b = np.ascontiguousarray(a, dtype="<u8").reshape(-1, 4).tobytes()
    return [int.from_bytes(b[32 * i: 32 * i + 32], "little") for i in range(len(b) // 32)]


def words(v):
    return [(v >> (32 * i)) & M32 for i in range(8)]


def value(ws):
    return sum(w << (32 * i) for i, w in enumerate(ws))


# ---- structured values ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def structured(w, c):
    """the values below 2^256 at which a chain over w-bit limbs that subtracts or compares against c can go wrong"""
    n = 8 if w == 32 else 9
    mask = (1 << w) - 1
    top = w * (n - 1)
    vals = {0, 1, 2, c - 1, c - 2, c, c + 1, (c - 1) // 2, (c - 1) // 2 + 1}
    for k in range(n):
        vals.update((1 << (w * k)) + d for d in (-1, 0, 1))
    under = ((c >> top) - 1) << top  # a top limb one below c's: the value stays below c whatever the lower limbs hold
    low = (1 << top) - 1
    for i in range(n):
        for ln in range(1, n - i + 1):
            run = ((1 << (w * ln)) - 1) << (w * i)
            vals.add(run & TOP)
            if i + ln <= n - 1:
                vals.add(under | run)
                vals.add(under | (low ^ run))
    for k in range(1, n):  # equal to c from limb k up, one off in limb k - 1, all zeros or all ones below
        hi = (c >> (w * k)) << (w * k)
        lk = (c >> (w * (k - 1))) & mask
        for d in (-1, 1):
            if 0 <= lk + d <= mask:
                for below in (0, (1 << (w * (k - 1))) - 1):
                    vals.add(hi | ((lk + d) << (w * (k - 1))) | below)
    return tuple(sorted(v for v in vals if 0 <= v <= TOP))


@functools.lru_cache(maxsize=None)
def structured_any():
    """every structured value of both limb widths and of the constants p, 2p, 4p, with the multiples of p between and above them"""
    vals = set(structured(32, P)) | set(structured(32, 2 * P)) | set(structured(32, 4 * P)) | set(structured(29, P))
    vals.update(k * P + d for k in (3, 5) for d in (-1, 0, 1))
    vals.add(TOP)
    return tuple(sorted(vals))


@functools.lru_cache(maxsize=None)
def structured_below(bound=P):
    return tuple(v for v in structured_any() if v < bound)


# ---- carry and borrow runs -----------------------------------------------------------------------------------------------------
def add_runs(a, b):
    """the (lo, ln) of a + b: word lo generates a carry that then rides through ln words whose sums are 0xffffffff"""
    aw, bw = words(a), words(b)
    runs, i = set(), 0
    while i < 8:
        if aw[i] + bw[i] > M32:
            ln = 0
            while i + ln + 1 < 8 and aw[i + ln + 1] + bw[i + ln + 1] == M32:
                ln += 1
            runs.add((i, ln))
            i += ln + 1
        else:
            i += 1
    return runs


def sub_runs(a, b):
    """the (lo, ln) of a - b: word lo generates a borrow that then rides through ln words with a == b"""
    aw, bw = words(a), words(b)
    runs, i = set(), 0
    while i < 8:
        if aw[i] < bw[i]:
            ln = 0
            while i + ln + 1 < 8 and aw[i + ln + 1] == bw[i + ln + 1]:
                ln += 1
            runs.add((i, ln))
            i += ln + 1
        else:
            i += 1
    return runs


ADD_RUNS = frozenset((lo, ln) for lo in range(7) for ln in range(7 - lo))  # word 7 of a value below p cannot take part in a sum run
SUB_RUNS = frozenset((lo, ln) for lo in range(8) for ln in range(8 - lo))  # equal top words can: the borrow then leaves the chain


def _rand_words(rnd, full):
    ws = [rnd.getrandbits(32) for _ in range(8)]
    if not full:
        ws[7] = rnd.randrange(P7)
    return ws


def _run_word(rnd, kind):
    return (0, M32, rnd.getrandbits(32))[kind % 3]


def _add_run_pair(rnd, lo, ln, kind):
    a, b = _rand_words(rnd, False), _rand_words(rnd, False)
    if kind % 2:  # no carry comes in from below
        for i in range(lo):
            a[i], b[i] = rnd.getrandbits(31), rnd.getrandbits(31)
    if kind % 3 == 0:  # the smallest generating sum: the word becomes 0 (or 1 with a carry in)
        a[lo] = rnd.randrange(1, 1 << 32)
        b[lo] = (1 << 32) - a[lo]
    elif kind % 3 == 1:  # the largest
        a[lo] = b[lo] = M32
    else:
        a[lo] = rnd.randrange(1, 1 << 32)
        b[lo] = rnd.randrange((1 << 32) - a[lo], 1 << 32)
    for i in range(lo + 1, lo + ln + 1):
        a[i] = _run_word(rnd, kind + i)
        b[i] = M32 ^ a[i]
    j = lo + ln + 1
    if j < 7:  # the word that takes the carry in without passing it on (word 7's sum is below 2^31 anyway)
        a[j] = rnd.randrange(M32)
        b[j] = (M32 - 1 - a[j]) if kind % 4 == 0 else rnd.randrange(M32 - a[j])
    return value(a), value(b)


def _sub_run_pair(rnd, lo, ln, kind, full):
    a, b = _rand_words(rnd, full), _rand_words(rnd, full)
    if kind % 2:  # no borrow comes in from below
        for i in range(lo):
            a[i], b[i] = max(a[i], b[i]), min(a[i], b[i])
    if kind % 3 == 0:  # the smallest generating difference: the word becomes 0xffffffff
        a[lo] = rnd.randrange(M32 if lo < 7 or full else P7 - 1)
        b[lo] = a[lo] + 1
    elif kind % 3 == 1 and (lo < 7 or full):  # the largest
        a[lo], b[lo] = 0, M32
    else:
        b[lo] = rnd.randrange(1, 1 << 32 if lo < 7 or full else P7)
        a[lo] = rnd.randrange(b[lo])
    for i in range(lo + 1, lo + ln + 1):
        a[i] = b[i] = _run_word(rnd, kind + i) if i < 7 or full else rnd.randrange(P7)
    j = lo + ln + 1
    if j < 8:  # the word that takes the borrow without passing it on
        hi = (1 << 32) if j < 7 or full else P7
        a[j] = rnd.randrange(1, hi)
        b[j] = (a[j] - 1) if kind % 4 == 0 else rnd.randrange(a[j])
        if kind % 4 == 2:  # or the other way round: the word generates a borrow of its own and a - b ends negative
            a[j], b[j] = b[j], a[j]
    return value(a), value(b)


VARIANTS = 12  # a multiple of 2, 3 and 4: every combination of the choices above


@functools.lru_cache(maxsize=None)
def limb_add_pairs():
    rnd = random.Random(0xADD)
    out = [(a, b) for a in (0, 1, P - 1) for b in (0, 1, P - 1)]
    out += [_add_run_pair(rnd, lo, ln, kind) for lo, ln in sorted(ADD_RUNS) for kind in range(VARIANTS)]
    assert all(a < P and b < P for a, b in out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def limb_sub_pairs(full=False):
    """full: any 256-bit operands (for the comparisons); otherwise both below p.  Both operand orders of every pair."""
    rnd = random.Random(0x5B + full)
    out = [(a, b) for a in (0, 1, P - 1) for b in (0, 1, P - 1)]
    for lo, ln in sorted(SUB_RUNS):
        for kind in range(VARIANTS):
            a, b = _sub_run_pair(rnd, lo, ln, kind, full)
            out += [(a, b), (b, a)]
    assert all(a <= TOP and b <= TOP for a, b in out) and (full or all(a < P and b < P for a, b in out))
    return tuple(out)


# ---- result-targeted pairs -----------------------------------------------------------------------------------------------------
DRAWS = 2


@functools.lru_cache(maxsize=None)
def targeted_add_pairs():
    """a, b < p with a + b == t (no subtraction) and a + b == t + p (the subtraction lands on t), t every structured value below p"""
    rnd = random.Random(0x7ADD)
    out = []
    for t in structured_below():
        for _ in range(DRAWS):
            a = rnd.randrange(0, t + 1)
            out.append((a, t - a))
            if t + 1 <= P - 1:  # a, b in [t + 1, p - 1]; t == p - 1 has no such pair (a + b <= 2p - 2)
                a = rnd.randrange(t + 1, P)
                out.append((a, t + P - a))
    assert all(0 <= a < P and 0 <= b < P for a, b in out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def targeted_sub_pairs():
    """a, b < p with a - b == t (no borrow) and a - b == t - p (the add-back of p lands on t)"""
    rnd = random.Random(0x75B)
    out = []
    for t in structured_below():
        for _ in range(DRAWS):
            a = rnd.randrange(t, P)
            out.append((a, a - t))
            if t >= 1:  # a in [0, t - 1]; t == 0 has no borrowing pair
                a = rnd.randrange(0, t)
                out.append((a, a + P - t))
    assert all(0 <= a < P and 0 <= b < P for a, b in out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def add_pairs():
    return limb_add_pairs() + targeted_add_pairs()


@functools.lru_cache(maxsize=None)
def sub_pairs():
    return limb_sub_pairs() + targeted_sub_pairs()


@functools.lru_cache(maxsize=None)
def cmp_pairs():
    """any 256-bit x, y: the borrow runs (top words free), equal values, neighbours, and values that differ in one bit of one word"""
    rnd = random.Random(0xC3)
    s = structured_any()
    out = list(limb_sub_pairs(True)) + list(limb_sub_pairs(False))
    out += [(v, v) for v in s]
    out += [(u, v) for u, v in zip(s, s[1:])] + [(v, u) for u, v in zip(s, s[1:])]
    for i in range(8):
        for bit in (0, 31):
            x = rnd.getrandbits(256)
            out += [(x, x ^ (1 << (32 * i + bit))), (x ^ (1 << (32 * i + bit)), x)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fold_pairs():
    """(x, y) for fe_fold(x, y, r) = fe_add(x, r * fe_sub(y, x)): with r = one the sub and the add see exactly the pairs above --
    x = a, y = a + b makes the add fe_add(a, b); y = a, x = b makes the sub fe_sub(a, b)"""
    return tuple((a, (a + b) % P) for a, b in add_pairs()) + tuple((b, a) for a, b in sub_pairs())


# ---- wide_reduce: 700 x + 324 y on both sides of every multiple of p ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_pairs():
    """(x, y, k, d): x, y < p with 700 x + 324 y == k p + d, |d| <= 2, every k in 0..1023 that has a solution.  gcd(700, 324) = 4
    and p == 1 mod 4, so d == -k mod 4: d == 0 exactly for the multiples of 4, d == +-2 for k == 2 mod 4."""
    rnd = random.Random(0x14)
    inv = pow(175, -1, 81)
    out = []
    for k in range(1024):
        for d in (-2, -1, 0, 1, 2):
            n = k * P + d
            if n < 0 or n % 4:
                continue
            n //= 4  # 175 x + 81 y == n: x == n / 175 mod 81, y = (n - 175 x) / 81 in [0, p - 1]
            x0 = n * inv % 81
            lo = max(0, -((81 * (P - 1) - n) // 175))  # ceil((n - 81 (p - 1)) / 175)
            hi = min(P - 1, n // 175)
            j_lo, j_hi = -((x0 - lo) // 81), (hi - x0) // 81  # x = x0 + 81 j in [lo, hi]
            if j_lo > j_hi:
                continue
            for _ in range(DRAWS):
                x = x0 + 81 * rnd.randrange(j_lo, j_hi + 1)
                y = (n - 175 * x) // 81
                assert 0 <= x < P and 0 <= y < P and 700 * x + 324 * y == k * P + d
                out.append((x, y, k, d))
    return tuple(out)


# ---- products whose result is a structured value ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mont_products():
    """(x, y, t): x, y < p with x y 2^-256 == t mod p, so the Montgomery product's final subtraction must land on t"""
    rnd = random.Random(0x0)
    out = []
    for t in structured_below():
        for _ in range(DRAWS):
            x = rnd.randrange(1, P)
            out.append((x, t * R * pow(x, -1, P) % P, t))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def shoup_products():
    """(x, w, t): x, w < p with x w == t mod p (the Shoup product by a constant)"""
    rnd = random.Random(0x24)
    out = []
    for t in structured_below():
        for _ in range(DRAWS):
            w = rnd.randrange(1, P)
            out.append((t * pow(w, -1, P) % P, w, t))
    return tuple(out)


# ---- the new self-test ops: operands and definitions -----------------------------------------------------------------------------
def _cond_sub(k):
    return lambda x, y: x - k * P if x >= k * P else x


def _pairs_of(values):
    return tuple((v, v) for v in values)


# op -> (what it runs, the case set as (x, y) pairs, the definition on ints); one-operand ops ignore y
NEW_OPS = {
    27: ("fe_add", add_pairs, lambda x, y: (x + y) % P),
    28: ("fe_sub", sub_pairs, lambda x, y: (x - y) % P),
    29: ("fe_neg", lambda: _pairs_of(structured_below()), lambda x, y: (-x) % P),
    30: ("fe_dbl", lambda: _pairs_of(structured_below()), lambda x, y: 2 * x % P),
    31: ("fe_lt | fe_eq", cmp_pairs, lambda x, y: int(x < y) | (int(x == y) << 32) | (int(y < x) << 64)),
    32: ("cond_sub_kp<1>", lambda: _pairs_of(structured_any()), _cond_sub(1)),
    33: ("cond_sub_kp<2>", lambda: _pairs_of(structured_any()), _cond_sub(2)),
    34: ("cond_sub_kp<4>", lambda: _pairs_of(structured_any()), _cond_sub(4)),
    35: ("fe_reduce_any", lambda: _pairs_of(structured_any()), lambda x, y: x % P),
    36: ("fe_fold(x, y, one)", fold_pairs, lambda x, y: y),
    37: ("fe_fold(x, y, x)", fold_pairs, lambda x, y: (x + x * (y - x) * RINV) % P),
    38: ("pack_canon29", lambda: _pairs_of(structured_below(2 * P)), lambda x, y: x % P),
}
ONE_OPERAND = (29, 30, 32, 33, 34, 35, 38)


def new_op_cases(op):
    """-> xs, ys (ints), the expected results (ints)"""
    _, cases, define = NEW_OPS[op]
    pairs = cases()
    xs, ys = [x for x, _ in pairs], [y for _, y in pairs]
    return xs, ys, [define(x, y) for x, y in pairs]


# the single-operand ops the table already had: op -> (largest operand it accepts, exclusive; the definition, or None where the
# result is only almost reduced: op 9)
OLD_UNARY = {
    3: (P, lambda x: x * RINV % P),      # pack29(from_mont29(x))
    6: (P, lambda x: x * RINV % P),      # fe_from_montx
    7: (P, lambda x: x * R % P),         # fe_to_montx
    9: (R, None),                        # pack29(unpack_reduce29(x)): congruent, below p (1 + 2^-10)
    12: (2 * P, lambda x: x % P),        # cond_sub_p29
    17: (R, lambda x: x % P),            # to_scaled29 and back
    18: (P, lambda x: x * RINV % P),     # a Montgomery image to the scaled domain and back to canonical
}


def old_unary_cases(op):
    return [v for v in structured_any() if v < OLD_UNARY[op][0]]


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def coverage():
    """what the pairs above contain, computed on the ints alone"""
    adds, subs = add_pairs(), sub_pairs()
    sums, diffs = {a + b for a, b in adds}, {a - b for a, b in subs}
    return {
        "add_runs": set().union(*(add_runs(a, b) for a, b in adds)),
        "sub_runs": set().union(*(sub_runs(a, b) for a, b in subs)),
        "sums": {name: v in sums for name, v in (("p-1", P - 1), ("p", P), ("p+1", P + 1), ("2p-2", 2 * P - 2))},
        "diffs": {name: v in diffs for name, v in (("0", 0), ("1", 1), ("-1", -1), ("p-1", P - 1), ("-(p-1)", 1 - P))},
        "wide_k": {k for _, _, k, _ in wide_pairs()},
        "wide_d": {(k % 4, d) for _, _, k, d in wide_pairs()},
    }
