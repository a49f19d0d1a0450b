"""The tuple lookup of include/provekit_tuplelookup.h on Python ints: the outer IO pattern, the challenges, the stacked leaves, the
multiplicities, a prover that writes whole proof bytes and a verifier that names the check, the side and the layer it fails at, and the
claims with their coefficients.  Written from the header's protocol text over tests/fracsum_refs.py (the two fractional sums) and
tests/prodcheck_refs.py (the sponge).  The reference project contains no such argument: this file is the measure for bytes, claims and
verdicts.  TEST INFRASTRUCTURE ONLY; small sizes (pure Python).

Values are canonical ints throughout; Montgomery form exists only at the library's boundary (K.mont / K.unmont).  f is a list of c
groups, a group a list of w columns, a column a list of 2^n ints; t is a list of w columns of 2^k ints."""
import fracsum_refs as F
import prodcheck_refs as K

P = K.P
V = K.V
LABEL = b"provekit-hip/tuple-lookup/v1"


def log2c(c):
    return {1: 0, 2: 1, 4: 2}[c]


def legal(n, k, w, c, n_bind=0):
    return 1 <= n <= 28 and 1 <= k <= 28 and 1 <= w <= 4 and c in (1, 2, 4) and n + log2c(c) <= 28 and 0 <= n_bind <= 16


def pattern(n, k, w, c, n_bind=0) -> bytes:
    ops = [b"A%dbind" % n_bind] * bool(n_bind) + [b"S1alpha"] + [b"S1beta"] * (w > 1) + [b"S2seeds"]
    return LABEL + b"/n%d/k%d/w%d/c%d" % (n, k, w, c) + b"".join(b"\0" + op for op in ops)


def proof_bytes(n, k, w, c) -> int:
    return F.proof_bytes(n + log2c(c), 1) + F.proof_bytes(k, 0)


def challenges(n, k, w, c, bind=()):
    """(alpha, beta, [seed_F, seed_T]) of the statement and its bind elements; beta = 1 without an operation when w = 1"""
    M = K.Merlin(pattern(n, k, w, c, len(bind)))
    M.public(list(bind))
    alpha = M.challenge()
    beta = M.challenge() if w > 1 else 1
    seeds = M.a.challenge_scalars(2)
    assert M.a.done()
    return alpha, beta, seeds


def compress(cols, x, beta):
    return sum(pow(beta, j, P) * col[x] for j, col in enumerate(cols)) % P


def leaves(groups, alpha, beta):
    """alpha - sum_j beta^j col[g][j][x], the groups stacked: index g 2^n + x"""
    return [(alpha - compress(cols, x, beta)) % P for cols in groups for x in range(len(cols[0]))]


def rows(cols):
    return list(zip(*cols))


def multiplicities(f, t):
    """m[y] = how many rows of all groups equal row y of t (t's rows distinct; every row of f in t)"""
    where = {row: y for y, row in enumerate(rows(t))}
    m = [0] * len(t[0])
    for cols in f:
        for row in rows(cols):
            m[where[row]] += 1
    return m


def eq_hi(z_hi, g):
    """eq(z_hi, g): coordinate i of z_hi <-> bit len(z_hi) - 1 - i of g (variable 0 is the most significant index bit)"""
    e = 1
    for i, z in enumerate(z_hi):
        e = e * (z if (g >> (len(z_hi) - 1 - i)) & 1 else 1 - z) % P
    return e


def claims(n, k, w, c, alpha, beta, z_f, cq_f, z_t, cp_t, cq_t):
    hi = log2c(c)
    return {"alpha": alpha, "beta": beta, "z_lo": list(z_f[hi:]), "z_t": list(z_t),
            "f_coeff": [[eq_hi(z_f[:hi], g) * pow(beta, j, P) % P for j in range(w)] for g in range(c)], "t_coeff": [pow(beta, j, P) for j in range(w)],
            "f_value": (alpha - cq_f) % P, "t_value": (alpha - cq_t) % P, "m_value": cp_t}


def prove(n, k, f, t, m, bind=(), validate=True):
    """-> dict: proof, the claims' fields, fractions [(P_F, Q_F), (P_T, Q_T)].  validate=False: a proof is written also when the two
    fractions differ -- what a prover whose rows are not inside the table can send"""
    c, w = len(f), len(t)
    assert all(len(cols) == w and all(len(col) == 1 << n for col in cols) for cols in f) and all(len(col) == 1 << k for col in t) and len(m) == 1 << k
    alpha, beta, seeds = challenges(n, k, w, c, bind)
    Fs = F.prove(n + log2c(c), None, leaves(f, alpha, beta), [seeds[0]], validate)
    Ts = F.prove(k, m, leaves([t], alpha, beta), [seeds[1]], validate)
    if validate:
        assert (Fs["P"] * Ts["Q"] - Ts["P"] * Fs["Q"]) % P == 0, "the rows are not inside t under m"
    out = claims(n, k, w, c, alpha, beta, Fs["point"], Fs["value_q"], Ts["point"], Ts["value_p"], Ts["value_q"])
    out.update(proof=Fs["proof"] + Ts["proof"], fractions=[(Fs["P"], Fs["Q"]), (Ts["P"], Ts["Q"])])
    return out


def verify(n, k, w, c, proof, bind=(), pat=None):
    """-> ("NONE", "F", 0, total, claims dict) or (the failed check's name, the side, the layer, the offset within the whole proof or
    None where the sumcheck verifier states it, None)"""
    nf = n + log2c(c)
    len_f, total = F.proof_bytes(nf, 1), proof_bytes(n, k, w, c)
    if len(proof) < total:
        return "TRANSCRIPT_SHORT", "F", 0, len(proof), None
    if len(proof) > total:
        return "TRAILING_BYTES", "F", 0, total, None
    try:
        A = V.Arthur(pat or pattern(n, k, w, c, len(bind)), b"".join((x % P).to_bytes(32, "little") for x in bind))
        A.next_scalars(len(bind))
        (alpha,) = A.challenge_scalars(1)
        beta = A.challenge_scalars(1)[0] if w > 1 else 1
        seeds = A.challenge_scalars(2)
        if not A.done():
            return "IO_PATTERN", "F", 0, 0, None
    except V.VerifyError as err:
        return F._outer_error(err), "F", 0, 0, None
    seen = []
    for side, size, unit, seed, part, at in (("F", nf, 1, seeds[0], proof[:len_f], 0), ("T", k, 0, seeds[1], proof[len_f:], len_f)):
        check, lay, offset, got = F.verify(size, unit, part, [seed])
        if check != "NONE":
            return check, side, lay, None if offset is None else offset + at, None
        seen.append(got)
    Fs, Ts = seen
    if (Fs["P"] * Ts["Q"] - Ts["P"] * Fs["Q"]) % P:
        return "FRACTION", "T", 0, len_f + 128, None
    return "NONE", "F", 0, total, claims(n, k, w, c, alpha, beta, Fs["point"], Fs["value_q"], Ts["point"], Ts["value_p"], Ts["value_q"])


def check_claims(cl, f_evals, t_evals, m_eval):
    """f_evals[g][j] = f[g][j](z_lo), t_evals[j] = t[j](z_t), m_eval = m(z_t) -> "NONE", or the first claim that fails: "F", "T", "M" """
    if sum(co * v for row, evs in zip(cl["f_coeff"], f_evals) for co, v in zip(row, evs)) % P != cl["f_value"]:
        return "F"
    if sum(co * v for co, v in zip(cl["t_coeff"], t_evals)) % P != cl["t_value"]:
        return "T"
    return "NONE" if m_eval % P == cl["m_value"] else "M"


def evaluations(f, t, m, cl):
    """the columns' multilinear extensions at the claims' points: what the caller opens"""
    return [[F.mle_at(col, cl["z_lo"]) for col in cols] for cols in f], [F.mle_at(col, cl["z_t"]) for col in t], F.mle_at(m, cl["z_t"])


def random_case(n, k, w, c, seed):
    """(f, t, m, idx): a table of 2^k distinct random rows and c groups of 2^n rows drawn from it; idx[g][x] the row of t"""
    import random

    rng = random.Random(seed)
    t = [[rng.randrange(P) for _ in range(1 << k)] for _ in range(w)]
    assert len(set(rows(t))) == 1 << k
    idx = [[rng.randrange(1 << k) for _ in range(1 << n)] for _ in range(c)]
    f = [[[t[j][i] for i in idx[g]] for j in range(w)] for g in range(c)]
    return f, t, multiplicities(f, t), idx
