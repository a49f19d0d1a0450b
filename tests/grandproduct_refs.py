"""The GKR grand product and the multiset-equality argument of include/provekit_grandproduct.h on Python ints: the two outer IO
patterns, provers that write whole proof bytes with every layer, and verifiers that name the check, the layer and the side they fail
at.  Written from the header's protocol text over tests/prodcheck_refs.py (the layers' product sumchecks) and the oracle's sponge.
TEST INFRASTRUCTURE ONLY; small sizes (pure Python).

Values are canonical ints throughout; Montgomery form exists only at the library's boundary (K.mont / K.unmont)."""
import random

import prodcheck_refs as K

P = K.P
V = K.V
LABEL = b"provekit-hip/grandproduct/v1"
MULTISET_LABEL = b"provekit-hip/multiset/v1"


class Layer(K.Shape):
    """layer d's constant sumcheck statement: sum_x eq(z_d, x) L_d(x) R_d(x) over d variables, binding one seed"""

    def __init__(self, d):
        self.name, self.n, self.n_bind, self.has_tau = "layer", d, 1, True
        self.m, self.terms, self.D = 2, [(1, 0b11)], 2


def pattern(n, n_bind=0) -> bytes:
    ops = [b"A%dbind" % n_bind] * bool(n_bind) + [b"A2top", b"S1rho"] + [b"S1seed", b"A2finals", b"S1rho"] * (n - 1)
    return LABEL + b"/n%d" % n + b"".join(b"\0" + op for op in ops)


def layer_at(d) -> int:
    """where layer d's proof starts; layer_at(n) is the length of the whole proof"""
    return 64 + sum(Layer(k).proof_bytes() for k in range(1, d))


def proof_bytes(n) -> int:
    return layer_at(n)


def layers_of(v):
    """[V_0, .., V_n] of the table v = V_n"""
    out = [list(v)]
    while len(out[0]) > 1:
        top, half = out[0], len(out[0]) // 2
        out.insert(0, [top[x] * top[x + half] % P for x in range(half)])
    return out


def next_claim(l, r, rho):
    return ((1 - rho) * l + rho * r) % P


def prove(n, v, bind=()):
    """-> dict: proof, P, point (z_n), value (c_n), layers ([V_0 .. V_n])"""
    assert len(v) == 1 << n
    layers = layers_of(v)
    M = K.Merlin(pattern(n, len(bind)))
    M.public(list(bind))
    M.add(layers[1])
    rho = M.challenge()
    z, c = [rho], next_claim(layers[1][0], layers[1][1], rho)
    proof = M.out
    for d in range(1, n):
        seed = M.challenge()
        child, half = layers[d + 1], 1 << d
        part, r, (l, rr), s = K.prove(Layer(d), [child[:half], child[half:]], z, [seed])
        assert s == c, "a layer's sum is the running claim"
        proof += part
        M.public([l, rr])
        rho = M.challenge()
        z, c = [rho] + r, next_claim(l, rr, rho)
    assert M.a.done() and len(proof) == proof_bytes(n)
    return {"proof": proof, "P": layers[0][0], "point": z, "value": c, "layers": layers}


def _outer_error(err):
    msg = str(err)
    return "TRANSCRIPT_SHORT" if "too short" in msg else "NON_CANONICAL" if "non-canonical" in msg else "IO_PATTERN"


def verify(n, proof, bind=(), pat=None, expected_product=None):
    """-> ("NONE", 0, dict with P, point, value) or (the failed check's name, the layer, None)"""
    total = proof_bytes(n)
    if len(proof) < total:
        return "TRANSCRIPT_SHORT", 0, None
    if len(proof) > total:
        return "TRAILING_BYTES", 0, None
    # the outer transcript reads bind | top | every layer's two finals, which are the last 64 bytes of that layer's proof
    outer = b"".join((x % P).to_bytes(32, "little") for x in bind) + proof[:64] + b"".join(proof[layer_at(d + 1) - 64 : layer_at(d + 1)] for d in range(1, n))
    try:
        A = V.Arthur(pat or pattern(n, len(bind)), outer)
        A.next_scalars(len(bind))
        top = A.next_scalars(2)
        product = top[0] * top[1] % P
        if expected_product is not None and product != expected_product % P:
            return "PRODUCT", 0, None
        (rho,) = A.challenge_scalars(1)
        z, c = [rho], next_claim(top[0], top[1], rho)
        for d in range(1, n):
            (seed,) = A.challenge_scalars(1)
            shape = Layer(d)
            check, r, finals = K.verify(shape, proof[layer_at(d) : layer_at(d + 1)], z, [seed], c)
            if check != "NONE":
                return check, d, None
            assert A.next_scalars(2) == finals
            (rho,) = A.challenge_scalars(1)
            z, c = [rho] + r, next_claim(finals[0], finals[1], rho)
        if not A.done():
            return "IO_PATTERN", 0, None
    except V.VerifyError as err:
        return _outer_error(err), 0, None
    return "NONE", 0, {"P": product, "point": z, "value": c}


# ---- multiset equality ---------------------------------------------------------------------------------------------------------------


def multiset_pattern(n, w, n_bind=0) -> bytes:
    ops = [b"A%dbind" % n_bind] * bool(n_bind) + [b"S1gamma"] + [b"S1beta"] * (w > 1) + [b"S2seeds"]
    return MULTISET_LABEL + b"/n%d/w%d" % (n, w) + b"".join(b"\0" + op for op in ops)


def multiset_proof_bytes(n) -> int:
    return 2 * proof_bytes(n)


def leaves(cols, gamma, beta):
    return [(gamma - sum(pow(beta, j, P) * col[x] for j, col in enumerate(cols))) % P for x in range(len(cols[0]))]


def _challenges(A, w):
    (gamma,) = A.challenge_scalars(1)
    beta = A.challenge_scalars(1)[0] if w > 1 else 1
    seeds = A.challenge_scalars(2)
    return gamma, beta, seeds


def multiset_prove(n, a_cols, b_cols, bind=(), validate=True):
    """-> dict: proof, gamma, beta, z_a, z_b, comb_a, comb_b, products.  validate=False: a proof is written also when the two products
    differ -- what a prover with unequal multisets can send: both grand products hold, and their products are not the same"""
    w = len(a_cols)
    assert len(b_cols) == w and all(len(c) == 1 << n for c in a_cols + b_cols)
    M = K.Merlin(multiset_pattern(n, w, len(bind)))
    M.public(list(bind))
    gamma, beta, seeds = _challenges(M.a, w)
    assert M.a.done()
    sides = [prove(n, leaves(cols, gamma, beta), [seed]) for cols, seed in zip((a_cols, b_cols), seeds)]
    if validate:
        assert sides[0]["P"] == sides[1]["P"], "the two sides are not equal as multisets"
    return {"proof": sides[0]["proof"] + sides[1]["proof"], "gamma": gamma, "beta": beta, "z_a": sides[0]["point"], "z_b": sides[1]["point"],
            "comb_a": (gamma - sides[0]["value"]) % P, "comb_b": (gamma - sides[1]["value"]) % P, "products": [s["P"] for s in sides]}


def multiset_verify(n, w, proof, bind=(), pat=None):
    """-> ("NONE", "A", 0, dict) or (the failed check's name, the side, the layer, None)"""
    half = proof_bytes(n)
    if len(proof) < 2 * half:
        return "TRANSCRIPT_SHORT", "A", 0, None
    if len(proof) > 2 * half:
        return "TRAILING_BYTES", "A", 0, None
    try:
        A = V.Arthur(pat or multiset_pattern(n, w, len(bind)), b"".join((x % P).to_bytes(32, "little") for x in bind))
        A.next_scalars(len(bind))
        gamma, beta, seeds = _challenges(A, w)
        if not A.done():
            return "IO_PATTERN", "A", 0, None
    except V.VerifyError as err:
        return _outer_error(err), "A", 0, None
    seen = []
    for side, seed, part in zip("AB", seeds, (proof[:half], proof[half:])):
        check, layer, got = verify(n, part, [seed])
        if check != "NONE":
            return check, side, layer, None
        seen.append(got)
    if seen[0]["P"] != seen[1]["P"]:
        return "PRODUCT", "B", 0, None
    return "NONE", "A", 0, {"gamma": gamma, "beta": beta, "z_a": seen[0]["point"], "z_b": seen[1]["point"],
                            "comb_a": (gamma - seen[0]["value"]) % P, "comb_b": (gamma - seen[1]["value"]) % P}


def random_table(n, seed, zeros=()):
    rng = random.Random(seed)
    v = [rng.randrange(1, P) for _ in range(1 << n)]
    for x in zeros:
        v[x] = 0
    return v


def mle_at(table, point):
    """the multilinear extension of `table` at `point`, variable 0 <-> the most significant index bit"""
    eq = K.pr.eq_table(list(point))
    return sum(e * v for e, v in zip(eq, table)) % P
