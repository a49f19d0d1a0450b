"""The wide product sumcheck of include/provekit_sumcheck_wide.h on Python ints: a catalogue of statements, the IO pattern, a prover
that writes whole proof bytes, one round by itself and a verifier that names the check it fails.  Written from the header's protocol
text in the style of tests/prodcheck_refs.py, whose sponge (Merlin), Montgomery helpers and eq1 it reuses; the round and the verifier are
prodcheck_refs' own, which read a statement only through its terms_at, pattern and counts.  TEST INFRASTRUCTURE ONLY; small sizes.

Values are canonical ints throughout; Montgomery form exists only at the library's boundary (mont / unmont)."""
import prodcheck_refs as K

P = K.P
LABEL = b"provekit-hip/sumcheck-wide/v1"
Merlin, mont, unmont, eq1, poly_at = K.Merlin, K.mont, K.unmont, K.eq1, K.poly_at
random_tables, random_elements, pr = K.random_tables, K.random_elements, K.pr


def _indices(mask):
    return [j for j in range(4) if (mask >> j) & 1]


# name -> (m, [(coefficient, [table, ...])], has_tau).  A repeated table is a power; every list is non-decreasing
CATALOGUE = {
    # the vanilla Plonk gate eq (qL a + qR b + qM a b + qO c + qC): tables qL qR qM qO qC a b c
    "plonk": (8, [(1, [0, 5]), (1, [1, 6]), (1, [2, 5, 6]), (1, [3, 7]), (1, [4])], True),
    "pow5": (1, [(1, [0, 0, 0, 0, 0])], False),                                         # x^5
    "a2b3c": (3, [(1, [0, 0, 1, 1, 1]), (P - 1, [2])], True),                           # eq (a^2 b^3 - c)
    # 16 tables, 16 terms, table 0 in every one
    "wide16": (16, [(3, [0])] + [((1, P - 1, 5)[t % 3], [0, t]) for t in range(1, 16)], True),
    "lin16": (16, [((1, P - 1, t + 2)[t % 3], [t]) for t in range(16)], False),         # a linear statement over 16 tables
    "coeffs": (4, [(1, [0, 1]), (P - 1, [1, 2]), (0, [2, 3]), (7, [0, 3, 3]), (P - 2, [1])], True),  # 1, -1, 0 and others
    "twice": (2, [(3, [0, 1]), (P - 4, [0, 1]), (1, [1])], False),                      # the same list in two terms
}
# one statement for each D = 1 .. 5, with and without tau
_PER_DEGREE = {
    1: (3, [(1, [0]), (5, [1]), (P - 1, [2]), (2, [0])]),
    2: (2, [(1, [0, 1]), (2, [0, 0])]),
    3: (3, [(1, [0, 1, 2]), (P - 1, [1, 1])]),
    4: (3, [(1, [0, 0, 1, 2]), (3, [2])]),
    5: (2, [(2, [0, 1, 1, 1, 1]), (P - 1, [0, 0])]),
}
for _d, (_m, _terms) in _PER_DEGREE.items():
    CATALOGUE["d%d" % _d] = (_m, _terms, False)
    CATALOGUE["d%dt" % _d] = (_m, _terms, True)
# the twelve statements of prodcheck_refs, mask by mask: what both interfaces can state
TRANSLATED = {"pks_" + name: name for name in list(K.SHAPES) + list(K.FORMS)}
for _wide, _name in TRANSLATED.items():
    _m, _terms, _tau = K.SHAPES[_name] if _name in K.SHAPES else K.FORMS[_name]
    CATALOGUE[_wide] = (_m, [(c, _indices(mask)) for c, mask in _terms], _tau)

ONE_PER_DEGREE = ["d1t", "d2", "d3t", "d4", "d5t"]


class Shape:
    def __init__(self, name, n, n_bind=0):
        self.name, self.n, self.n_bind = name, n, n_bind
        self.m, self.terms, self.has_tau = CATALOGUE[name]
        self.D = max(len(factors) for _, factors in self.terms)

    def statement(self):
        from provekit_amd import prodcheck_wide

        return prodcheck_wide.Statement(self.n, self.m, self.terms, self.has_tau, self.n_bind)

    def pattern(self) -> bytes:
        d = LABEL + b"/n%d/m%d/T%d/tau%d/terms" % (self.n, self.m, len(self.terms), int(self.has_tau))
        d += b"-".join(b".".join(b"%d" % j for j in factors) for _, factors in self.terms)
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
        for c, factors in self.terms:
            for j in factors:
                c = c * v[j] % P
            total += c
        return total % P


def round_values(shape, tables, tau_rest=None, fold=None):
    """ONE round by the header's definition (pksw_round): h(0) .. h(D), or with a fold challenge (h, folded tables)"""
    return K.round_values(shape, tables, tau_rest, fold)


def prove(shape, tables, tau=None, bind=(), pattern=None):
    """-> (proof bytes, point, finals, s)"""
    n, D = shape.n, shape.D
    assert (tau is not None) == shape.has_tau and len(bind) == shape.n_bind and len(tables) == shape.m
    M = Merlin(pattern or shape.pattern())
    M.public(list(bind))
    if tau is not None:
        M.public(list(tau))
    M.public([c for c, _ in shape.terms])
    f = [list(t) for t in tables]
    point, s = [], None
    for i in range(n):
        h = round_values(shape, f, tau[i + 1 :] if tau is not None else None)
        if i == 0:
            s = ((1 - tau[0]) * h[0] + tau[0] * h[1]) % P if tau is not None else (h[0] + h[1]) % P
            M.add([s])
        M.add(h)
        r = M.challenge()
        point.append(r)
        half = len(f[0]) // 2
        f = [[(t[x] + r * (t[x + half] - t[x])) % P for x in range(half)] for t in f]
    finals = [t[0] for t in f]
    M.add(finals)
    assert M.a.done() and len(M.out) == 32 * (1 + n * (D + 1) + shape.m)
    return M.out, point, finals, s


def verify(shape, proof, tau=None, bind=(), expected_sum=None, pattern=None):
    """-> ("NONE", point, finals) or (the failed check's name, None, None): the names of pks_check_name"""
    return K.verify(shape, proof, tau, bind, expected_sum, pattern)
