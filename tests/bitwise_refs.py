"""The bitwise argument of include/provekit_bitwise.h on Python ints: the plan, the outer IO pattern, the seed, the decomposition of two
columns (c, the digit columns; m with the spare group), the operation's table and its extension U + beta V + beta^2 O, a prover that
hands the plan's groups and the table to the tuple lookup's reference prover and a verifier with the table check that names the check,
the side and the layer it fails at, the claims with their coefficients.  Written from the header's protocol text over
tests/tuplelookup_refs.py (the one inner lookup) and tests/prodcheck_refs.py (the sponge).  TEST INFRASTRUCTURE ONLY; small sizes (pure
Python).

Values are canonical ints throughout; Montgomery form exists only at the library's boundary (K.mont / K.unmont)."""
import random

import fracsum_refs as F
import prodcheck_refs as K
import tuplelookup_refs as T

P = K.P
V = K.V
LABEL = b"provekit-hip/bitwise/v1"
AND, XOR, OR = 0, 1, 2
OPS = (AND, XOR, OR)
NAMES = (b"and", b"xor", b"or")
WHICH = ("NONE", "DIGITS", "RECOMPOSE_A", "RECOMPOSE_B", "RECOMPOSE_C", "M")


def apply(op, a, b):
    return (a & b, a ^ b, a | b)[op]


def plan(d, L):
    """-> dict bits, k, c, digit_of (per group g < c)"""
    c = 4 if L == 3 else L
    return {"bits": L * d, "k": 2 * d, "c": c, "digit_of": list(range(L)) + [0] * (c - L)}  # the spare group: digit 0 again


def legal(n, op, d, L, n_bind=0):
    if not (1 <= n <= 28 and op in OPS and 1 <= d <= 12 and 1 <= L <= 4 and 0 <= n_bind <= 16):
        return False
    return n + T.log2c(plan(d, L)["c"]) <= 28


def pattern(n, op, d, L, n_bind=0) -> bytes:
    ops = [b"A%dbind" % n_bind] * bool(n_bind) + [b"S1seed"]
    return LABEL + b"/" + NAMES[op] + b"/n%d/d%d/l%d" % (n, d, L) + b"".join(b"\0" + o for o in ops)


def proof_bytes(n, op, d, L) -> int:
    return T.proof_bytes(n, 2 * d, 3, plan(d, L)["c"])


def seed_of(n, op, d, L, bind=()):
    M = K.Merlin(pattern(n, op, d, L, len(bind)))
    M.public(list(bind))
    seed = M.challenge()
    assert M.a.done()
    return seed


def table(op, d):
    """the three columns: row y = (u << d) | v is (u, v, u op v)"""
    size = 1 << d
    return [[y >> d for y in range(size * size)], [y & (size - 1) for y in range(size * size)], [apply(op, y >> d, y & (size - 1)) for y in range(size * size)]]


def digits_of(col, d, L):
    return [[(v >> (d * i)) & ((1 << d) - 1) for v in col] for i in range(L)]


def groups_of(d, L, digits):
    """digits: [a's, b's, c's], each L columns -> the c groups the lookup sees, each three columns; the spare repeats group 0"""
    return [[digits[j][i] for j in range(3)] for i in plan(d, L)["digit_of"]]


def count_bins(d, L, digits):
    """{y: m[y]} for the non-zero m[y] of all c groups, from the digits of a and b: a row's place is (a_i << d) | b_i"""
    bins = {}
    for i in plan(d, L)["digit_of"]:
        for u, v in zip(digits[0][i], digits[1][i]):
            bins[(u << d) | v] = bins.get((u << d) | v, 0) + 1
    return bins


def counts(d, L, digits):
    """m over the table's 2^(2d) rows"""
    m = [0] * (1 << (2 * d))
    for y, count in count_bins(d, L, digits).items():
        m[y] = count
    return m


def decompose_bins(op, d, L, a, b):
    """a, b: canonical ints below 2^(L d) -> (c, [a's, b's, c's digit columns], {y: m[y]} of the non-zero m[y]): for tables too large
    to list"""
    assert all(0 <= v < 1 << (L * d) for v in a + b)
    c = [apply(op, u, v) for u, v in zip(a, b)]
    digits = [digits_of(col, d, L) for col in (a, b, c)]
    return c, digits, count_bins(d, L, digits)


def decompose(op, d, L, a, b):
    """-> (c, [a's, b's, c's digit columns], m)"""
    c, digits, _ = decompose_bins(op, d, L, a, b)
    return c, digits, counts(d, L, digits)


def first_bad(op, d, L, a, b, c=None):
    """(the smallest failing x, its case "a" / "b" / "c") or None"""
    for x, (u, v) in enumerate(zip(a, b)):
        if u >> (L * d):
            return x, "a"
        if v >> (L * d):
            return x, "b"
        if c is not None and c[x] != apply(op, u, v):
            return x, "c"
    return None


def index_at(z):
    """I(z) = sum_j z_j 2^(v-1-j): the extension of y -> y, variable 0 the most significant bit"""
    acc = 0
    for zj in z:
        acc = (2 * acc + zj) % P
    return acc


def bit_op(op, s, t):
    """the operation's multilinear extension on one bit pair"""
    return (s * t, s + t - 2 * s * t, s + t - s * t)[op] % P


def uvo_at(op, d, z):
    """(U, V, O) at z, 2 d coordinates"""
    o = 0
    for j in range(d):
        o = (2 * o + bit_op(op, z[j], z[d + j])) % P
    return index_at(z[:d]), index_at(z[d:]), o


def table_at(op, d, z, beta):
    u, v, o = uvo_at(op, d, z)
    return (u + beta * v + beta * beta * o) % P


def claims(n, op, d, L, look):
    """look: the lookup's claims (T.claims' dict)"""
    pl = plan(d, L)
    coeff = [[0] * L for _ in range(3)]
    for g in range(pl["c"]):
        for j in range(3):
            coeff[j][pl["digit_of"][g]] = (coeff[j][pl["digit_of"][g]] + look["f_coeff"][g][j]) % P
    return {"z_lo": list(look["z_lo"]), "z_t": list(look["z_t"]), "digit_coeff": coeff, "digits_value": look["f_value"], "pow2": [1 << (d * i) for i in range(L)],
            "m_value": look["m_value"]}


def prove(n, op, d, L, digits, m, bind=(), validate=True, table_op=None):
    """digits: [a's, b's, c's] -> dict: proof, the claims' fields.  validate=False: a proof is written also when the lookup fails.
    table_op: another operation's table than the statement's, for proofs built to fail exactly the table check"""
    assert len(digits) == 3 and all(len(part) == L and all(len(col) == 1 << n for col in part) for part in digits) and len(m) == 1 << (2 * d)
    look = T.prove(n, 2 * d, groups_of(d, L, digits), table(op if table_op is None else table_op, d), m, [seed_of(n, op, d, L, bind)], validate)
    out = claims(n, op, d, L, look)
    out["proof"] = look["proof"]
    return out


def verify(n, op, d, L, proof, bind=(), pat=None):
    """-> ("NONE", "F", 0, total, claims dict) or (the failed check's name, the side, the layer, the offset within the proof or None
    where the sumcheck verifier states it, None)"""
    pl = plan(d, L)
    total = proof_bytes(n, op, d, L)
    if len(proof) < total:
        return "TRANSCRIPT_SHORT", "F", 0, len(proof), None
    if len(proof) > total:
        return "TRAILING_BYTES", "F", 0, total, None
    try:
        A = V.Arthur(pat or pattern(n, op, d, L, len(bind)), b"".join((x % P).to_bytes(32, "little") for x in bind))
        A.next_scalars(len(bind))
        (seed,) = A.challenge_scalars(1)
        if not A.done():
            return "IO_PATTERN", "F", 0, 0, None
    except V.VerifyError as err:
        return F._outer_error(err), "F", 0, 0, None
    check, side, lay, offset, got = T.verify(n, 2 * d, 3, pl["c"], proof, [seed])
    if check != "NONE":
        return check, side, lay, offset, None
    if got["t_value"] != table_at(op, d, got["z_t"], got["beta"]):
        return "TABLE", "T", 0, total, None
    return "NONE", "F", 0, total, claims(n, op, d, L, got)


def check_claims(cl, abc_evals, digit_evals, m_eval):
    """abc_evals = a, b, c at z_lo, digit_evals[j][i] = digit_{j,i}(z_lo), m_eval = m(z_t) -> "NONE", or the first claim that fails, in
    WHICH's order"""
    if sum(co * v for row, evs in zip(cl["digit_coeff"], digit_evals) for co, v in zip(row, evs)) % P != cl["digits_value"]:
        return "DIGITS"
    for j, name in enumerate(("RECOMPOSE_A", "RECOMPOSE_B", "RECOMPOSE_C")):
        if sum(p2 * v for p2, v in zip(cl["pow2"], digit_evals[j])) % P != abc_evals[j] % P:
            return name
    return "NONE" if m_eval % P == cl["m_value"] else "M"


def evaluations(abc, digits, m, cl):
    """the evaluations of the claims: what the caller opens"""
    return [F.mle_at(col, cl["z_lo"]) for col in abc], [[F.mle_at(col, cl["z_lo"]) for col in part] for part in digits], F.mle_at(m, cl["z_t"])


def edge_pairs(d, L):
    """(a, b): 0, 2^bits - 1, all-ones and alternating digits, equal operands"""
    top = (1 << (L * d)) - 1
    alt = sum(((1 << d) - 1) << (d * i) for i in range(0, L, 2))  # digits all ones, zero, all ones, ..
    bits = sum(1 << i for i in range(0, L * d, 2))  # 0101..
    out = []
    for pair in ((0, 0), (top, top), (0, top), (top, 0), (alt, top ^ alt), (alt, alt), (bits, top ^ bits), (bits, top), (top, bits)):
        if pair not in out:
            out.append(pair)
    return out


def columns(n, d, L, kind, seed=0):
    """(a, b): two columns of 2^n ints below 2^(L d).  kind: "random"; "edges" (as many of edge_pairs as the columns have room for,
    among random values); "skew" (one pair everywhere); "small" (values below 2^d: every high digit zero)"""
    rng = random.Random(1000 * n + 10 * d + L + seed)
    size, top = 1 << n, 1 << (L * d)
    if kind == "skew":
        return [rng.randrange(top)] * size, [rng.randrange(top)] * size
    if kind == "small":
        return [rng.randrange(1 << d) for _ in range(size)], [rng.randrange(1 << d) for _ in range(size)]
    a, b = [rng.randrange(top) for _ in range(size)], [rng.randrange(top) for _ in range(size)]
    if kind == "edges":
        for i, (u, v) in enumerate(edge_pairs(d, L)[:size]):
            a[(i * 3) % size], b[(i * 3) % size] = u, v  # distinct places: 3 is odd
    return a, b
