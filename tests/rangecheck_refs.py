"""The limb-decomposed range check of include/provekit_rangecheck.h on Python ints: the plan, the outer IO pattern, the seed, the
decomposition of a column (limbs; m with the scaled and the spare group), a prover that hands the plan's groups and the identity table
to the tuple lookup's reference prover and a verifier with the table check that names the check, the side and the layer it fails at,
the claims with their coefficients.  Written from the header's protocol text over tests/tuplelookup_refs.py (the one inner lookup) and
tests/prodcheck_refs.py (the sponge).  TEST INFRASTRUCTURE ONLY; small sizes (pure Python).

Values are canonical ints throughout; Montgomery form exists only at the library's boundary (K.mont / K.unmont)."""
import random

import fracsum_refs as F
import prodcheck_refs as K
import tuplelookup_refs as T

P = K.P
V = K.V
LABEL = b"provekit-hip/range/v1"
WHICH = ("NONE", "LIMBS", "RECOMPOSE", "M")


def plan(bits, k):
    """-> dict L, r, G, c, limb_of, shift_of (per group g < c), or None when more than four groups are needed"""
    L = -(-bits // k)
    r = bits - (L - 1) * k
    G = L + (r < k)
    if G > 4:
        return None
    c = 4 if G == 3 else G
    limb_of = list(range(L)) + [L - 1] * (G - L) + [0] * (c - G)  # the limbs, the top check, the spare group: limb 0 again
    shift_of = [0] * L + [k - r] * (G - L) + [0] * (c - G)
    return {"L": L, "r": r, "G": G, "c": c, "limb_of": limb_of, "shift_of": shift_of}


def legal(n, bits, k, n_bind=0):
    if not (1 <= n <= 28 and 1 <= bits <= 64 and 1 <= k <= 28 and 0 <= n_bind <= 16):
        return False
    pl = plan(bits, k)
    return pl is not None and n + T.log2c(pl["c"]) <= 28


def pattern(n, bits, k, n_bind=0) -> bytes:
    ops = [b"A%dbind" % n_bind] * bool(n_bind) + [b"S1seed"]
    return LABEL + b"/n%d/b%d/k%d" % (n, bits, k) + b"".join(b"\0" + op for op in ops)


def proof_bytes(n, bits, k) -> int:
    return T.proof_bytes(n, k, 1, plan(bits, k)["c"])


def seed_of(n, bits, k, bind=()):
    M = K.Merlin(pattern(n, bits, k, len(bind)))
    M.public(list(bind))
    seed = M.challenge()
    assert M.a.done()
    return seed


def groups_of(bits, k, limbs):
    """the c columns the lookup sees: a limb column, the top limb scaled, the spare repeat"""
    pl = plan(bits, k)
    return [[(v << s) % P for v in limbs[i]] for i, s in zip(pl["limb_of"], pl["shift_of"])]


def decompose(bits, k, f):
    """f: canonical ints, all below 2^bits -> (the L limb columns, m over 0 .. 2^k - 1 of all c groups)"""
    pl = plan(bits, k)
    assert all(0 <= v < 1 << bits for v in f)
    limbs = [[(v >> (k * i)) & ((1 << k) - 1) for v in f] for i in range(pl["L"])]
    m = [0] * (1 << k)
    for col in groups_of(bits, k, limbs):
        for y in col:
            m[y] += 1
    return limbs, m


def first_bad(bits, f):
    """the smallest x with f[x] >= 2^bits, or None"""
    return next((x for x, v in enumerate(f) if v >> bits), None)


def claims(n, bits, k, look):
    """look: the lookup's claims (T.claims' dict)"""
    pl = plan(bits, k)
    coeff = [0] * pl["L"]
    for g in range(pl["c"]):
        coeff[pl["limb_of"][g]] = (coeff[pl["limb_of"][g]] + look["f_coeff"][g][0] * (1 << pl["shift_of"][g])) % P
    return {"z_lo": list(look["z_lo"]), "z_t": list(look["z_t"]), "limb_coeff": coeff, "limbs_value": look["f_value"], "pow2": [1 << (k * i) for i in range(pl["L"])],
            "m_value": look["m_value"]}


def prove(n, bits, k, limbs, m, bind=(), validate=True, table=None, groups=None):
    """limbs: L columns of 2^n ints -> dict: proof, the claims' fields.  validate=False: a proof is written also when the lookup fails.
    table: another table than 0 .. 2^k - 1, groups: other columns than the plan's, for proofs built to fail exactly the table check"""
    pl = plan(bits, k)
    assert len(limbs) == pl["L"] and all(len(col) == 1 << n for col in limbs) and len(m) == 1 << k
    cols = groups_of(bits, k, limbs) if groups is None else groups
    look = T.prove(n, k, [[col] for col in cols], [list(range(1 << k)) if table is None else table], m, [seed_of(n, bits, k, bind)], validate)
    out = claims(n, bits, k, look)
    out["proof"] = look["proof"]
    return out


def index_at(z):
    """I(z) = sum_j z_j 2^(v-1-j): the extension of y -> y, variable 0 the most significant bit"""
    acc = 0
    for zj in z:
        acc = (2 * acc + zj) % P
    return acc


def verify(n, bits, k, proof, bind=(), pat=None):
    """-> ("NONE", "F", 0, total, claims dict) or (the failed check's name, the side, the layer, the offset within the proof or None
    where the sumcheck verifier states it, None)"""
    pl = plan(bits, k)
    total = proof_bytes(n, bits, k)
    if len(proof) < total:
        return "TRANSCRIPT_SHORT", "F", 0, len(proof), None
    if len(proof) > total:
        return "TRAILING_BYTES", "F", 0, total, None
    try:
        A = V.Arthur(pat or pattern(n, bits, k, len(bind)), b"".join((x % P).to_bytes(32, "little") for x in bind))
        A.next_scalars(len(bind))
        (seed,) = A.challenge_scalars(1)
        if not A.done():
            return "IO_PATTERN", "F", 0, 0, None
    except V.VerifyError as err:
        return F._outer_error(err), "F", 0, 0, None
    check, side, lay, offset, got = T.verify(n, k, 1, pl["c"], proof, [seed])
    if check != "NONE":
        return check, side, lay, offset, None
    if got["t_value"] != index_at(got["z_t"]):
        return "TABLE", "T", 0, total, None
    return "NONE", "F", 0, total, claims(n, bits, k, got)


def check_claims(cl, f_eval, limb_evals, m_eval):
    """f_eval = f(z_lo), limb_evals[i] = limb_i(z_lo), m_eval = m(z_t) -> "NONE", or the first claim that fails, in WHICH's order"""
    if sum(co * v for co, v in zip(cl["limb_coeff"], limb_evals)) % P != cl["limbs_value"]:
        return "LIMBS"
    if sum(p2 * v for p2, v in zip(cl["pow2"], limb_evals)) % P != f_eval % P:
        return "RECOMPOSE"
    return "NONE" if m_eval % P == cl["m_value"] else "M"


def evaluations(f, limbs, m, cl):
    """the evaluations of the claims: what the caller opens"""
    return F.mle_at(f, cl["z_lo"]), [F.mle_at(col, cl["z_lo"]) for col in limbs], F.mle_at(m, cl["z_t"])


def edge_values(bits, k):
    """0, 2^bits - 1 (every limb all ones), 2^k - 1, 2^k and every limb 1, where they are below 2^bits"""
    top = 1 << bits
    out = []
    for v in (0, top - 1, (1 << k) - 1, 1 << k, sum(1 << (k * i) for i in range(-(-bits // k)))):
        if v < top and v not in out:
            out.append(v)
    return out


def column(n, bits, k, kind, seed=0):
    """2^n ints below 2^bits.  kind: "random"; "edges" (as many of edge_values as the column has room for, among random values);
    "skew" (every value equal); "small" (values below 2^min(k, bits): every high limb zero)"""
    rng = random.Random(1000 * n + 10 * bits + k + seed)
    size, top = 1 << n, 1 << bits
    if kind == "skew":
        return [rng.randrange(top)] * size
    if kind == "small":
        return [rng.randrange(1 << min(k, bits)) for _ in range(size)]
    f = [rng.randrange(top) for _ in range(size)]
    if kind == "edges":
        for i, v in enumerate(edge_values(bits, k)[:size]):
            f[(i * 3) % size] = v  # distinct places: 3 is odd
    return f
