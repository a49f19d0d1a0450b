"""The LogUp lookup argument of include/provekit_lookup.h on Python ints: the outer IO pattern, a prover that writes whole proof bytes
with every intermediate table, and a verifier that names the check and the side it fails at.  Written from the header's protocol text
over tests/prodcheck_refs.py (the two product sumchecks) and the oracle's sponge.  TEST INFRASTRUCTURE ONLY; small sizes (pure Python).

Values are canonical ints throughout; Montgomery form exists only at the library's boundary (K.mont / K.unmont)."""
import random

import prodcheck_refs as K

P = K.P
V = K.V
LABEL = b"provekit-hip/lookup/v1"
INV2 = (P + 1) // 2
CLAIMS = ("hf_at_rf", "f_at_rf", "ht_at_rt", "t_at_rt", "m_at_rt", "hf_at_half", "ht_at_half")


class Side(K.Shape):
    """the two constant sumcheck statements: F = eq h_f d_f (sum 1) over n variables, T = eq (h_t d_t - m) (sum 0) over k"""

    def __init__(self, side, n):
        self.name, self.n, self.n_bind, self.has_tau = side, n, 1, True
        self.m, self.terms = (2, [(1, 0b11)]) if side == "F" else (3, [(1, 0b011), (P - 1, 0b100)])
        self.D = 2
        self.expected = 1 if side == "F" else 0


def pattern(n, k, n_bind=0, n_bind2=0) -> bytes:
    ops = [b"A%dbind" % n_bind] * bool(n_bind) + [b"S1alpha"] + [b"A%dhelpers" % n_bind2] * bool(n_bind2)
    ops += [b"A1sum", b"S%dtau_f" % n, b"S%dtau_t" % k, b"S1seed"]
    return LABEL + b"/n%d/k%d" % (n, k) + b"".join(b"\0" + op for op in ops)


def proof_bytes(n, k) -> int:
    return 32 + Side("F", n).proof_bytes() + Side("T", k).proof_bytes()


def alpha_of(n, k, bind, n_bind2=0):
    """the alpha a proof of this statement draws after `bind`"""
    M = K.Merlin(pattern(n, k, len(bind), n_bind2))
    M.public(list(bind))
    return M.challenge()


def derive_claims(n, k, alpha, s, finals_f, finals_t):
    return {"hf_at_rf": finals_f[0], "f_at_rf": (alpha - finals_f[1]) % P, "ht_at_rt": finals_t[0], "t_at_rt": (alpha - finals_t[1]) % P,
            "m_at_rt": finals_t[2], "hf_at_half": s * pow(INV2, n, P) % P, "ht_at_half": s * pow(INV2, k, P) % P}


def multiplicities(k, idx):
    m = [0] * (1 << k)
    for i in idx:
        m[i] += 1
    return m


def first_bad(f, t, idx):
    """the smallest x whose lookup fails validation, or None"""
    for x, i in enumerate(idx):
        if i >= len(t) or f[x] != t[i]:
            return x
    return None


def prove(n, k, f, t, idx, bind=(), bind2=(), validate=True):
    """-> dict: proof, alpha, s, m, h_f, h_t, d_f, d_t, r_f, r_t, claims.  validate=False: f is not checked against t[idx], and the f
    side's helper columns are those of f as it stands, h_f = 1 / (alpha - f).  Both sumchecks then still hold -- what a prover with a
    non-member in f can send -- and s, the sum of h_t, is no longer the sum of h_f"""
    assert len(f) == len(idx) == 1 << n and len(t) == 1 << k
    if validate:
        assert first_bad(f, t, idx) is None
    m = multiplicities(k, idx)
    M = K.Merlin(pattern(n, k, len(bind), len(bind2)))
    M.public(list(bind))
    alpha = M.challenge()
    d_t = [(alpha - v) % P for v in t]
    assert all(d_t), "alpha is an entry of t"
    g = [pow(v, -1, P) for v in d_t]
    h_t = [c * v % P for c, v in zip(m, g)]
    d_f = [(alpha - v) % P for v in f]
    h_f = [g[i] if f[x] == t[i] else pow(d_f[x], -1, P) for x, i in enumerate(idx)]
    M.public(list(bind2))
    s = sum(h_t) % P
    M.add([s])
    tau_f = [M.challenge() for _ in range(n)]
    tau_t = [M.challenge() for _ in range(k)]
    seed = M.challenge()
    assert M.a.done()
    pf, r_f, finals_f, s_f = K.prove(Side("F", n), [h_f, d_f], tau_f, [seed])
    pt, r_t, finals_t, s_t = K.prove(Side("T", k), [h_t, d_t, m], tau_t, [seed])
    assert (s_f, s_t) == (1, 0)
    return {"proof": M.out + pf + pt, "alpha": alpha, "s": s, "m": m, "h_f": h_f, "h_t": h_t, "d_f": d_f, "d_t": d_t, "r_f": r_f, "r_t": r_t,
            "claims": derive_claims(n, k, alpha, s, finals_f, finals_t)}


def verify(n, k, proof, bind=(), bind2=(), pat=None):
    """-> ("NONE", "OUTER", dict with alpha, s, r_f, r_t, claims) or (the failed check's name, the side, None)"""
    F, T = Side("F", n), Side("T", k)
    total = 32 + F.proof_bytes() + T.proof_bytes()
    if len(proof) < total:
        return "TRANSCRIPT_SHORT", "OUTER", None
    if len(proof) > total:
        return "TRAILING_BYTES", "OUTER", None
    prefix = b"".join((v % P).to_bytes(32, "little") for v in list(bind) + list(bind2))
    try:
        A = V.Arthur(pat or pattern(n, k, len(bind), len(bind2)), prefix + proof[:32])
        A.next_scalars(len(bind))
        (alpha,) = A.challenge_scalars(1)
        A.next_scalars(len(bind2))
        (s,) = A.next_scalars(1)
        tau_f, tau_t = A.challenge_scalars(n), A.challenge_scalars(k)
        (seed,) = A.challenge_scalars(1)
        if not A.done():
            return "IO_PATTERN", "OUTER", None
    except V.VerifyError as err:
        msg = str(err)
        return ("TRANSCRIPT_SHORT" if "too short" in msg else "NON_CANONICAL" if "non-canonical" in msg else "IO_PATTERN"), "OUTER", None
    at = 32
    check, r_f, finals_f = K.verify(F, proof[at : at + F.proof_bytes()], tau_f, [seed], F.expected)
    if check != "NONE":
        return check, "F", None
    at += F.proof_bytes()
    check, r_t, finals_t = K.verify(T, proof[at:], tau_t, [seed], T.expected)
    if check != "NONE":
        return check, "T", None
    return "NONE", "OUTER", {"alpha": alpha, "s": s, "r_f": r_f, "r_t": r_t, "claims": derive_claims(n, k, alpha, s, finals_f, finals_t)}


def random_case(n, k, seed, distinct=True, used=None):
    """(f, t, idx): a seeded table of 2^k values and 2^n lookups into it; `used`: only that many leading entries are ever looked up"""
    rng = random.Random(seed)
    t = [rng.randrange(P) for _ in range(1 << k)]
    if not distinct and k >= 1:
        for y in range(1, 1 << k, 2):  # every odd entry repeats its even neighbour
            t[y] = t[y - 1]
    idx = [rng.randrange(used or (1 << k)) for _ in range(1 << n)]
    return [t[i] for i in idx], t, idx


def mle_at(table, point):
    """the multilinear extension of `table` at `point`, variable 0 <-> the most significant index bit"""
    eq = K.pr.eq_table(list(point))
    return sum(e * v for e, v in zip(eq, table)) % P
