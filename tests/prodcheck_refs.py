"""The product sumcheck of include/provekit_sumcheck.h on Python ints: statement shapes, the IO pattern, a prover that writes whole
proof bytes and a verifier that names the check it fails.  Written from the header's protocol text over the oracle's sponge
(oracle/verifier.py's Arthur and keccak tag, oracle/pyref.py's permutation).  TEST INFRASTRUCTURE ONLY; small sizes (pure Python).

Values are canonical ints throughout; Montgomery form exists only at the library's boundary (mont / unmont below)."""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle")]

import pyref as pr  # noqa: E402
import verifier as V  # noqa: E402

P = pr.P
R = (1 << 256) % P
R_INV = pow(R, -1, P)
LABEL = b"provekit-hip/sumcheck/v1"

# name -> (m, [(coefficient, mask)], has_tau): the shapes the header names, plus m = 4 with T = 4
SHAPES = {
    "inner": (2, [(1, 0b11)], False),                                        # <a, b>
    "r1cs": (3, [(1, 0b011), (P - 1, 0b100)], True),                         # eq (a b - c)
    "eval": (1, [(1, 0b1)], True),                                           # eq f
    "triple": (3, [(1, 0b111)], False),                                      # a b c
    "mixed": (4, [(1, 0b0011), (2, 0b1100), (1, 0b0001)], True),             # a b + 2 c d + a
    "four": (4, [(3, 0b0111), (P - 5, 0b1110), (1, 0b1001), (7, 0b0100)], True),
}

# The forms of the round kernel that the shapes above do not reach (csrc/sumcheck/round.hip dispatches on (D, m); lane.hpp on the
# coefficient's kind): linear statements over several tables, coefficients 1, -1, 0 and others with and without tau, a mask in two
# terms.  Kept apart: the suites over SHAPES run those six; these run where a test names FORMS
FORMS = {
    "lin2": (2, [(1, 0b01), (5, 0b10)], True),                                             # eq (f0 + 5 f1)
    "lin3": (3, [(1, 0b001), (P - 1, 0b010), (7, 0b100)], False),                          # f0 - f1 + 7 f2
    "lin4": (4, [(3, 0b0001), (1, 0b0010), (P - 1, 0b0100), (P - 2, 0b1000)], True),       # eq (3 f0 + f1 - f2 - 2 f3)
    "lin2rep": (2, [(1, 0b01), (0, 0b10), (P - 1, 0b01), (9, 0b10)], False),               # f0 + 0 f1 - f0 + 9 f1
    "deg3low": (3, [(P - 1, 0b111), (1, 0b011), (4, 0b100)], True),                        # eq (-a b c + a b + 4 c)
    "pair2": (2, [(P - 1, 0b11), (1, 0b01), (1, 0b10)], False),                            # -a b + a + b
}


class Shape:
    def __init__(self, name, n, n_bind=0):
        self.name, self.n, self.n_bind = name, n, n_bind
        self.m, self.terms, self.has_tau = SHAPES[name] if name in SHAPES else FORMS[name]
        self.D = max(bin(mask).count("1") for _, mask in self.terms)

    def statement(self):
        from provekit_amd import prodcheck

        return prodcheck.Statement(self.n, self.m, self.terms, self.has_tau, self.n_bind)

    def pattern(self) -> bytes:
        d = LABEL + b"/n%d/m%d/T%d/tau%d/masks" % (self.n, self.m, len(self.terms), int(self.has_tau))
        d += b".".join(b"%d" % mask for _, mask in self.terms)
        ops = []
        if self.n_bind:
            ops.append(b"A%dbind" % self.n_bind)
        if self.has_tau:
            ops.append(b"A%dtau" % self.n)
        ops += [b"A%dcoefficients" % len(self.terms), b"A1sum"]
        for _ in range(self.n):
            ops += [b"A%dround_values" % (self.D + 1), b"S1challenge"]
        ops.append(b"A%dfinal_values" % self.m)
        return d + b"".join(b"\0" + op for op in ops)

    def proof_bytes(self) -> int:
        return 32 * (1 + self.n * (self.D + 1) + self.m)

    def terms_at(self, v):
        total = 0
        for c, mask in self.terms:
            prod = c
            for j in range(self.m):
                if (mask >> j) & 1:
                    prod = prod * v[j] % P
            total += prod
        return total % P


def random_tables(m, n, seed):
    rng = random.Random(seed)
    return [[rng.randrange(P) for _ in range(1 << n)] for _ in range(m)]


def random_elements(k, seed):
    rng = random.Random(seed)
    return [rng.randrange(P) for _ in range(k)]


def mont(values) -> np.ndarray:
    """canonical ints -> [k, 4] uint64 Montgomery limbs"""
    buf = b"".join((v % P * R % P).to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype="<u8").reshape(-1, 4).copy()


def unmont(limbs) -> list:
    b = np.ascontiguousarray(limbs, dtype="<u8").reshape(-1, 4).tobytes()
    return [int.from_bytes(b[32 * i : 32 * i + 32], "little") * R_INV % P for i in range(len(b) // 32)]


def eq1(t, r):
    return (t * r + (1 - t) * (1 - r)) % P


def poly_at(h, x):
    """the polynomial of degree <= len(h) - 1 through (k, h[k]) at x"""
    total = 0
    for k, hk in enumerate(h):
        num, den = 1, 1
        for j in range(len(h)):
            if j != k:
                num = num * (x - j) % P
                den = den * (k - j) % P
        total += hk * num * pow(den, -1, P)
    return total % P


class Merlin:
    """the prover side of the sponge: public values are absorbed, proof values absorbed and written"""

    def __init__(self, pattern: bytes):
        self.a = V.Arthur(pattern, b"")
        self.out = b""

    def public(self, values):
        self.a._expect("A", len(values))
        for v in values:
            self.a._absorb(v % P)

    def add(self, values):
        self.public(values)
        self.out += b"".join((v % P).to_bytes(32, "little") for v in values)

    def challenge(self):
        return self.a.challenge_scalars(1)[0]


def prove(shape: Shape, tables, tau=None, bind=(), pattern=None):
    """-> (proof bytes, point, finals, s)"""
    n, m, D = shape.n, shape.m, shape.D
    assert (tau is not None) == shape.has_tau and len(bind) == shape.n_bind
    M = Merlin(pattern or shape.pattern())
    M.public(list(bind))
    if tau is not None:
        M.public(list(tau))
    M.public([c for c, _ in shape.terms])
    f = [list(t) for t in tables]
    point = []
    for i in range(n):
        half = len(f[0]) // 2
        w = pr.eq_table(list(tau[i + 1 :])) if tau is not None else None
        h = [0] * (D + 1)
        picks = [(c, [j for j in range(m) if (mask >> j) & 1]) for c, mask in shape.terms]
        for x in range(half):
            lo = [t[x] for t in f]
            step = [t[x + half] - t[x] for t in f]
            for X in range(D + 1):
                v = [a + X * b for a, b in zip(lo, step)]  # reduced once per (x, X) below: Python ints do not overflow
                g = 0
                for c, js in picks:
                    for j in js:
                        c = c * v[j]
                    g += c
                h[X] += g % P * w[x] if w is not None else g % P
        h = [v % P for v in h]
        if i == 0:
            s = ((1 - tau[0]) * h[0] + tau[0] * h[1]) % P if tau is not None else (h[0] + h[1]) % P
            M.add([s])
        M.add(h)
        r = M.challenge()
        point.append(r)
        f = [[(t[x] + r * (t[x + half] - t[x])) % P for x in range(half)] for t in f]
    finals = [t[0] for t in f]
    M.add(finals)
    assert M.a.done()
    return M.out, point, finals, s


def round_values(shape: Shape, tables, tau_rest=None, fold=None):
    """ONE round by the header's definition (pks_round): h(0) .. h(D) of the tables as they stand, or with a fold challenge
    (h, folded tables) of the tables folded by it first.  The weight of pair x' is eq(tau_rest, x'), 1 where tau_rest is None --
    whatever shape.has_tau says, as pks_round takes tau_rest_or_null on its own terms"""
    f = [list(t) for t in tables]
    if fold is not None:
        half = len(f[0]) // 2
        f = [[(t[x] + fold * (t[x + half] - t[x])) % P for x in range(half)] for t in f]
    half = len(f[0]) // 2
    assert half >= 1 and all(len(t) == 2 * half for t in f) and len(f) == shape.m
    w = pr.eq_table(list(tau_rest)) if tau_rest is not None else [1] * half
    assert len(w) == half
    h = [0] * (shape.D + 1)
    for x in range(half):
        for X in range(shape.D + 1):
            h[X] += w[x] * shape.terms_at([t[x] + X * (t[x + half] - t[x]) for t in f])
    h = [v % P for v in h]
    return h if fold is None else (h, f)


class Rejected(Exception):
    def __init__(self, check):
        super().__init__(check)
        self.check = check


def verify(shape: Shape, proof: bytes, tau=None, bind=(), expected_sum=None, pattern=None):
    """-> ("NONE", point, finals) or (the failed check's name, None, None): the names of pks_check_name"""
    public = list(bind) + (list(tau) if tau is not None else []) + [c for c, _ in shape.terms]
    prefix = b"".join((v % P).to_bytes(32, "little") for v in public)
    try:
        try:
            A = V.Arthur(pattern or shape.pattern(), prefix + proof)
            A.next_scalars(len(public))
            (claim,) = A.next_scalars(1)
            if expected_sum is not None and claim != expected_sum % P:
                raise Rejected("SUM")
            e, point = 1, []
            for i in range(shape.n):
                h = A.next_scalars(shape.D + 1)
                lhs = e * ((1 - tau[i]) * h[0] + tau[i] * h[1]) % P if tau is not None else (h[0] + h[1]) % P
                if lhs != claim:
                    raise Rejected("ROUND")
                (r,) = A.challenge_scalars(1)
                point.append(r)
                claim = poly_at(h, r)
                if tau is not None:
                    e = e * eq1(tau[i], r) % P
                    claim = e * claim % P
            finals = A.next_scalars(shape.m)
            g = shape.terms_at(finals)
            if tau is not None:
                g = e * g % P
            if g != claim:
                raise Rejected("FINAL")
            if not A.done():
                raise Rejected("TRAILING_BYTES")
            return "NONE", point, finals
        except V.VerifyError as err:
            msg = str(err)
            raise Rejected("TRANSCRIPT_SHORT" if "too short" in msg else "NON_CANONICAL" if "non-canonical" in msg else "IO_PATTERN")
    except Rejected as rej:
        return rej.check, None, None
