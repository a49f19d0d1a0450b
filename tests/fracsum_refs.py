"""The GKR fractional sum and the LogUp-GKR lookup of include/provekit_fracsum.h on Python ints: the two outer IO patterns, provers
that write whole proof bytes with every layer of both trees, and verifiers that name the check, the layer and the side they fail at.
Written from the header's protocol text over tests/prodcheck_refs.py (the layers' product sumchecks) and the oracle's sponge.
TEST INFRASTRUCTURE ONLY; small sizes (pure Python).

Values are canonical ints throughout; Montgomery form exists only at the library's boundary (K.mont / K.unmont)."""
import random

import prodcheck_refs as K

P = K.P
V = K.V
LABEL = b"provekit-hip/fracsum/v1"
LOOKUP_LABEL = b"provekit-hip/logup-gkr/v1"


class Layer(K.Shape):
    """layer d's constant sumcheck statement over d variables, binding one seed: eq (pL qR + qL u) with tables {pL, qL, qR, u}, or
    the unit form of the leaves' layer, eq (qR + qL u) with tables {qL, qR, u}"""

    def __init__(self, d, unit_leaves=False):
        self.name, self.n, self.n_bind, self.has_tau, self.D = "layer", d, 1, True, 2
        self.m, self.terms = (3, [(1, 0b010), (1, 0b101)]) if unit_leaves else (4, [(1, 0b0101), (1, 0b1010)])


def layer(n, unit, d):
    return Layer(d, unit_leaves=bool(unit) and d == n - 1)


def pattern(n, unit, n_bind=0) -> bytes:
    ops = [b"A%dbind" % n_bind] * bool(n_bind) + [b"A4top", b"S1rho"]
    for d in range(1, n):
        ops += [b"S1lambda", b"S1seed", b"A%dfinals" % layer(n, unit, d).m, b"S1rho"]
    return LABEL + b"/n%d/u%d" % (n, unit) + b"".join(b"\0" + op for op in ops)


def layer_at(n, unit, d) -> int:
    """where layer d's proof starts; layer_at(n, unit, n) is the length of the whole proof"""
    return 128 + sum(layer(n, unit, k).proof_bytes() for k in range(1, d))


def proof_bytes(n, unit) -> int:
    return layer_at(n, unit, n)


def layers_of(p, q):
    """([p_0 .. p_n], [q_0 .. q_n]) of the leaves (p, q) = (p_n, q_n); p None: every numerator is 1"""
    ps, qs = [list(p) if p is not None else [1] * len(q)], [list(q)]
    while len(qs[0]) > 1:
        a, b, half = ps[0], qs[0], len(qs[0]) // 2
        ps.insert(0, [(a[x] * b[x + half] + a[x + half] * b[x]) % P for x in range(half)])
        qs.insert(0, [b[x] * b[x + half] % P for x in range(half)])
    return ps, qs


def next_claim(l, r, rho):
    return ((1 - rho) * l + rho * r) % P


def prove(n, p, q, bind=(), validate=True):
    """p None: unit.  -> dict: proof, P, Q, point (z_n), value_p (c_p,n; None when unit), value_q, p_layers, q_layers.  validate=False:
    a proof is written also when Q = 0"""
    unit = int(p is None)
    assert len(q) == 1 << n and (unit or len(p) == 1 << n)
    ps, qs = layers_of(p, q)
    if validate:
        assert qs[0][0] != 0, "a zero denominator"
    M = K.Merlin(pattern(n, unit, len(bind)))
    M.public(list(bind))
    M.add(ps[1] + qs[1])
    rho = M.challenge()
    z, cp, cq = [rho], next_claim(ps[1][0], ps[1][1], rho), next_claim(qs[1][0], qs[1][1], rho)
    proof = M.out
    for d in range(1, n):
        lam, seed = M.challenge(), M.challenge()
        pc, qc, half = ps[d + 1], qs[d + 1], 1 << d
        u = [(pc[x + half] + lam * qc[x + half]) % P for x in range(half)]
        shape = layer(n, unit, d)
        tables = [qc[:half], qc[half:], u] if shape.m == 3 else [pc[:half], qc[:half], qc[half:], u]
        part, r, finals, s = K.prove(shape, tables, z, [seed])
        assert s == (cp + lam * cq) % P, "a layer's sum is the running claim"
        proof += part
        M.public(finals)
        rho = M.challenge()
        if shape.m == 3:
            b, c, e = finals
            assert e == (1 + lam * c) % P
            cp = None
        else:
            a, b, c, e = finals
            cp = next_claim(a, (e - lam * c) % P, rho)
        z, cq = [rho] + r, next_claim(b, c, rho)
    assert M.a.done() and len(proof) == proof_bytes(n, unit)
    if unit and n == 1:
        cp = None
    return {"proof": proof, "P": ps[0][0], "Q": qs[0][0], "point": z, "value_p": cp, "value_q": cq, "p_layers": ps, "q_layers": qs}


def _outer_error(err):
    msg = str(err)
    return "TRANSCRIPT_SHORT" if "too short" in msg else "NON_CANONICAL" if "non-canonical" in msg else "IO_PATTERN"


def verify(n, unit, proof, bind=(), pat=None, expected=None):
    """expected: (num, den) or None.  -> ("NONE", 0, total, dict with P, Q, point, value_p, value_q) or (the failed check's name, the
    layer, the offset or None where the sumcheck verifier states it, None)"""
    total = proof_bytes(n, unit)
    if len(proof) < total:
        return "TRANSCRIPT_SHORT", 0, len(proof), None
    if len(proof) > total:
        return "TRAILING_BYTES", 0, total, None
    # the outer transcript reads bind | top | every layer's finals, which are the last bytes of that layer's proof
    outer = b"".join((x % P).to_bytes(32, "little") for x in bind) + proof[:128]
    for d in range(1, n):
        end = layer_at(n, unit, d + 1)
        outer += proof[end - 32 * layer(n, unit, d).m : end]
    try:
        A = V.Arthur(pat or pattern(n, unit, len(bind)), outer)
        A.next_scalars(len(bind))
        p0, p1, q0, q1 = A.next_scalars(4)
        num, den = (p0 * q1 + p1 * q0) % P, q0 * q1 % P
        if den == 0:
            return "DENOMINATOR", 0, 128, None
        if unit and n == 1 and (p0, p1) != (1, 1):
            return "UNIT", 0, 128, None
        if expected is not None and (num * expected[1] - expected[0] * den) % P:
            return "FRACTION", 0, 128, None
        (rho,) = A.challenge_scalars(1)
        z, cp, cq = [rho], next_claim(p0, p1, rho), next_claim(q0, q1, rho)
        for d in range(1, n):
            lam, seed = A.challenge_scalars(1)[0], A.challenge_scalars(1)[0]
            shape = layer(n, unit, d)
            check, r, finals = K.verify(shape, proof[layer_at(n, unit, d) : layer_at(n, unit, d + 1)], z, [seed], (cp + lam * cq) % P)
            if check != "NONE":
                return check, d, None, None
            assert A.next_scalars(shape.m) == finals
            if shape.m == 3:
                b, c, e = finals
                if e != (1 + lam * c) % P:
                    return "UNIT", d, layer_at(n, unit, d + 1), None
            (rho,) = A.challenge_scalars(1)
            if shape.m == 3:
                cp = None
            else:
                a, b, c, e = finals
                cp = next_claim(a, (e - lam * c) % P, rho)
            z, cq = [rho] + r, next_claim(b, c, rho)
        if not A.done():
            return "IO_PATTERN", 0, None, None
    except V.VerifyError as err:
        return _outer_error(err), 0, None, None
    if unit and n == 1:
        cp = None
    return "NONE", 0, total, {"P": num, "Q": den, "point": z, "value_p": cp, "value_q": cq}


# ---- the lookup: LogUp without helper columns ------------------------------------------------------------------------------------------


def lookup_pattern(n, k, n_bind=0) -> bytes:
    ops = [b"A%dbind" % n_bind] * bool(n_bind) + [b"S1alpha", b"S2seeds"]
    return LOOKUP_LABEL + b"/n%d/k%d" % (n, k) + b"".join(b"\0" + op for op in ops)


def lookup_proof_bytes(n, k) -> int:
    return proof_bytes(n, 1) + proof_bytes(k, 0)


def lookup_challenges(n, k, bind=()):
    """(alpha, [seed_F, seed_T]) of the statement and its bind elements"""
    M = K.Merlin(lookup_pattern(n, k, len(bind)))
    M.public(list(bind))
    alpha, seeds = M.challenge(), M.a.challenge_scalars(2)
    assert M.a.done()
    return alpha, seeds


def multiplicities(f, t):
    """m[j] = how often t[j] occurs in f (t's entries distinct; every entry of f in t)"""
    where = {v: j for j, v in enumerate(t)}
    m = [0] * len(t)
    for v in f:
        m[where[v]] += 1
    return m


def lookup_prove(n, k, f, t, m, bind=(), validate=True):
    """-> dict: proof, alpha, z_f, z_t, f_value, t_value, m_value, fractions [(P_F, Q_F), (P_T, Q_T)].  validate=False: a proof is written
    also when the two fractions differ -- what a prover whose column is not inside the table can send"""
    assert len(f) == 1 << n and len(t) == len(m) == 1 << k
    alpha, seeds = lookup_challenges(n, k, bind)
    F = prove(n, None, [(alpha - v) % P for v in f], [seeds[0]], validate)
    T = prove(k, m, [(alpha - v) % P for v in t], [seeds[1]], validate)
    if validate:
        assert (F["P"] * T["Q"] - T["P"] * F["Q"]) % P == 0, "f is not inside t under m"
    return {"proof": F["proof"] + T["proof"], "alpha": alpha, "z_f": F["point"], "z_t": T["point"], "f_value": (alpha - F["value_q"]) % P,
            "t_value": (alpha - T["value_q"]) % P, "m_value": T["value_p"], "fractions": [(F["P"], F["Q"]), (T["P"], T["Q"])]}


def lookup_verify(n, k, proof, bind=(), pat=None):
    """-> ("NONE", "F", 0, dict) or (the failed check's name, the side, the layer, None)"""
    len_f, total = proof_bytes(n, 1), lookup_proof_bytes(n, k)
    if len(proof) < total:
        return "TRANSCRIPT_SHORT", "F", 0, None
    if len(proof) > total:
        return "TRAILING_BYTES", "F", 0, None
    try:
        A = V.Arthur(pat or lookup_pattern(n, k, len(bind)), b"".join((x % P).to_bytes(32, "little") for x in bind))
        A.next_scalars(len(bind))
        (alpha,) = A.challenge_scalars(1)
        seeds = A.challenge_scalars(2)
        if not A.done():
            return "IO_PATTERN", "F", 0, None
    except V.VerifyError as err:
        return _outer_error(err), "F", 0, None
    seen = []
    for side, size, unit, seed, part in (("F", n, 1, seeds[0], proof[:len_f]), ("T", k, 0, seeds[1], proof[len_f:])):
        check, lay, _, got = verify(size, unit, part, [seed])
        if check != "NONE":
            return check, side, lay, None
        seen.append(got)
    F, T = seen
    if (F["P"] * T["Q"] - T["P"] * F["Q"]) % P:
        return "FRACTION", "T", 0, None
    return "NONE", "F", 0, {"alpha": alpha, "z_f": F["point"], "z_t": T["point"], "f_value": (alpha - F["value_q"]) % P,
                            "t_value": (alpha - T["value_q"]) % P, "m_value": T["value_p"]}


def random_table(n, seed, zeros=()):
    rng = random.Random(seed)
    v = [rng.randrange(1, P) for _ in range(1 << n)]
    for x in zeros:
        v[x] = 0
    return v


def fraction_sum(p, q):
    """sum_x p[x] / q[x] as a field element (q without zeros); p None: unit"""
    return sum((1 if p is None else p[x]) * pow(q[x], -1, P) for x in range(len(q))) % P


def mle_at(table, point):
    """the multilinear extension of `table` at `point`, variable 0 <-> the most significant index bit"""
    eq = K.pr.eq_table(list(point))
    return sum(e * v for e, v in zip(eq, table)) % P
