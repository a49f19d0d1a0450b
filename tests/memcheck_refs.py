"""The read-write memory check of include/provekit_memcheck.h on Python ints: the trace semantics as a plain replay loop, the outer IO
pattern, the challenges, the two stacked leaf tables and the time side's column, a prover that writes whole proof bytes and a verifier
that names the check, the side and the layer it fails at, and the claims with their coefficients.  Written from the header's protocol
text over tests/fracsum_refs.py (the fractional sums and the lookup) and tests/prodcheck_refs.py (the sponge).  TEST INFRASTRUCTURE
ONLY; small sizes (pure Python).

Values are canonical ints throughout; Montgomery form exists only at the library's boundary (K.mont / K.unmont).  A trace is a dict of
the eight columns a, wv, rv, rt (2^n ints each), init, fin, ft (2^k) and m (2^n)."""
import random

import fracsum_refs as F
import prodcheck_refs as K

P = K.P
V = K.V
LABEL = b"provekit-hip/memcheck/v1"
SIDES = ("OPS", "MEM", "TIME")
COLUMNS = ("a", "wv", "rv", "rt", "init", "fin", "ft", "m")


def legal(n, k, n_bind=0):
    return 1 <= n <= 27 and 1 <= k <= 27 and 0 <= n_bind <= 16


def pattern(n, k, n_bind=0) -> bytes:
    ops = [b"A%dbind" % n_bind] * bool(n_bind) + [b"S1gamma", b"S1beta", b"S3seeds"]
    return LABEL + b"/n%d/k%d" % (n, k) + b"".join(b"\0" + op for op in ops)


def side_bytes(n, k):
    return [F.proof_bytes(n + 1, 0), F.proof_bytes(k + 1, 0), F.lookup_proof_bytes(n, n)]


def proof_bytes(n, k) -> int:
    return sum(side_bytes(n, k))


def challenges(n, k, bind=()):
    """(gamma, beta, [seed_OPS, seed_MEM, seed_TIME]) of the statement and its bind elements"""
    M = K.Merlin(pattern(n, k, len(bind)))
    M.public(list(bind))
    gamma, beta = M.challenge(), M.challenge()
    seeds = M.a.challenge_scalars(3)
    assert M.a.done()
    return gamma, beta, seeds


def replay(addr, wv, init):
    """the trace of the operations (addr[i], wv[i]) on a memory that starts as init: operation i reads its cell, then writes wv[i] at
    the global time i + 1.  A plain replay, one operation after the other"""
    mem, when = list(init), [0] * len(init)
    rv, rt = [], []
    for i, (a, v) in enumerate(zip(addr, wv)):
        rv.append(mem[a]), rt.append(when[a])
        mem[a], when[a] = v, i + 1
    m = [0] * len(addr)
    for i, t in enumerate(rt):
        m[i - t] += 1
    return {"a": list(addr), "wv": list(wv), "rv": rv, "rt": rt, "init": list(init), "fin": mem, "ft": when, "m": m}


def future_read():
    """the header's trace (n = k = 1) whose two multisets are equal although operation 0 reads a value nothing has written yet; the
    second cell is never used.  m is the histogram its honest neighbour would have"""
    return {"a": [0, 0], "wv": [7, 7], "rv": [7, 0], "rt": [2, 0], "init": [0, 5], "fin": [7, 5], "ft": [1, 0], "m": [1, 1]}


def triples(tr):
    """(the write set, the read set) as sorted lists of triples"""
    cells, ops = range(len(tr["init"])), range(len(tr["a"]))
    written = [(j, tr["init"][j], 0) for j in cells] + [(tr["a"][i], tr["wv"][i], i + 1) for i in ops]
    read = [(tr["a"][i], tr["rv"][i], tr["rt"][i]) for i in ops] + [(j, tr["fin"][j], tr["ft"][j]) for j in cells]
    return sorted(written), sorted(read)


def leaves(tr, gamma, beta):
    """(q OPS: 2^(n+1), q MEM: 2^(k+1), f: 2^n) of the protocol's steps 2 to 4"""
    b2 = beta * beta % P
    ops, cells = range(len(tr["a"])), range(len(tr["init"]))
    q_ops = [(gamma - (tr["a"][i] + beta * tr["wv"][i] + b2 * (i + 1))) % P for i in ops] + [(gamma - (tr["a"][i] + beta * tr["rv"][i] + b2 * tr["rt"][i])) % P for i in ops]
    q_mem = [(gamma - (j + beta * tr["init"][j])) % P for j in cells] + [(gamma - (j + beta * tr["fin"][j] + b2 * tr["ft"][j])) % P for j in cells]
    return q_ops, q_mem, [(i - tr["rt"][i]) % P for i in ops]


def signs(v):
    return [1] * (1 << v) + [P - 1] * (1 << v)


def index_at(z):
    """I(z) = sum_j z_j 2^(v-1-j): the extension of x -> x, variable 0 the most significant bit"""
    acc = 0
    for zj in z:
        acc = (2 * acc + zj) % P
    return acc


def claims(n, k, gamma, beta, z_ops, cq_ops, z_mem, cq_mem, time):
    z0, y0, b2 = z_ops[0], z_mem[0], beta * beta % P
    return {"gamma": gamma, "beta": beta, "z_ops": list(z_ops[1:]), "z_mem": list(z_mem[1:]), "z_f": list(time["z_f"]), "z_t": list(time["z_t"]),
            "ops_coeff": [1, beta * (1 - z0) % P, beta * z0 % P, b2 * z0 % P], "mem_coeff": [beta * (1 - y0) % P, beta * y0 % P, b2 * y0 % P],
            "ops_value": (gamma - cq_ops - b2 * (1 - z0) * (index_at(z_ops[1:]) + 1)) % P, "mem_value": (gamma - cq_mem - index_at(z_mem[1:])) % P,
            "rt_value": (index_at(time["z_f"]) - time["f_value"]) % P, "m_value": time["m_value"]}


def balanced(a, b):
    return (a["P"] * b["Q"] + b["P"] * a["Q"]) % P == 0


def prove(n, k, tr, bind=(), validate=True, sign_ops=None, sign_mem=None, table=None):
    """-> dict: proof, the claims' fields, sums [OPS, MEM] (F.prove's dicts) and balanced.  validate=False: a proof is written also
    when the trace is inconsistent -- what a prover that does not care can send.  sign_ops, sign_mem, table: other numerator tables and
    another time table than the protocol's, for proofs built to fail exactly one of the verifier's own checks"""
    assert all(len(tr[c]) == 1 << n for c in ("a", "wv", "rv", "rt", "m")) and all(len(tr[c]) == 1 << k for c in ("init", "fin", "ft"))
    gamma, beta, seeds = challenges(n, k, bind)
    q_ops, q_mem, f = leaves(tr, gamma, beta)
    O = F.prove(n + 1, sign_ops or signs(n), q_ops, [seeds[0]], validate)
    M = F.prove(k + 1, sign_mem or signs(k), q_mem, [seeds[1]], validate)
    if validate:
        assert balanced(O, M), "the multisets differ"
    T = F.lookup_prove(n, n, f, table or list(range(1 << n)), tr["m"], [seeds[2]], validate)
    out = claims(n, k, gamma, beta, O["point"], O["value_q"], M["point"], M["value_q"], T)
    out.update(proof=O["proof"] + M["proof"] + T["proof"], sums=[O, M], balanced=balanced(O, M))
    return out


def lookup_verify(n, k, proof, bind):
    """F.lookup_verify with the offsets the library states: -> (check, layer, offset or None, claims dict or None)"""
    len_f = F.proof_bytes(n, 1)
    alpha, seeds = F.lookup_challenges(n, k, bind)
    seen = []
    for size, unit, seed, part, at in ((n, 1, seeds[0], proof[:len_f], 0), (k, 0, seeds[1], proof[len_f:], len_f)):
        check, lay, offset, got = F.verify(size, unit, part, [seed])
        if check != "NONE":
            return check, lay, None if offset is None else offset + at, None
        seen.append(got)
    A, B = seen
    if (A["P"] * B["Q"] - B["P"] * A["Q"]) % P:
        return "FRACTION", 0, len_f + 128, None
    return "NONE", 0, len(proof), {"alpha": alpha, "z_f": A["point"], "z_t": B["point"], "f_value": (alpha - A["value_q"]) % P, "t_value": (alpha - B["value_q"]) % P,
                                  "m_value": B["value_p"]}


def verify(n, k, proof, bind=(), pat=None):
    """-> ("NONE", "OPS", 0, total, claims dict) or (the failed check's name, the side, the layer, the offset within the whole proof or
    None where the sumcheck verifier states it, None)"""
    part = side_bytes(n, k)
    at, total = [0, part[0], part[0] + part[1]], sum(part)
    if len(proof) < total:
        return "TRANSCRIPT_SHORT", "OPS", 0, len(proof), None
    if len(proof) > total:
        return "TRAILING_BYTES", "OPS", 0, total, None
    try:
        A = V.Arthur(pat or pattern(n, k, len(bind)), b"".join((x % P).to_bytes(32, "little") for x in bind))
        A.next_scalars(len(bind))
        (gamma,) = A.challenge_scalars(1)
        (beta,) = A.challenge_scalars(1)
        seeds = A.challenge_scalars(3)
        if not A.done():
            return "IO_PATTERN", "OPS", 0, 0, None
    except V.VerifyError as err:
        return F._outer_error(err), "OPS", 0, 0, None
    seen = []
    for side, size in ((0, n + 1), (1, k + 1)):
        check, lay, offset, got = F.verify(size, 0, proof[at[side] : at[side] + part[side]], [seeds[side]])
        if check != "NONE":
            return check, SIDES[side], lay, None if offset is None else offset + at[side], None
        if got["value_p"] != (1 - 2 * got["point"][0]) % P:
            return "SIGN", SIDES[side], 0, at[side] + part[side], None
        seen.append(got)
    O, M = seen
    if not balanced(O, M):
        return "BALANCE", "MEM", 0, at[1] + 128, None
    check, lay, offset, time = lookup_verify(n, n, proof[at[2] :], [seeds[2]])
    if check != "NONE":
        return check, "TIME", lay, None if offset is None else offset + at[2], None
    if time["t_value"] != index_at(time["z_t"]):
        return "TIME_TABLE", "TIME", 0, total, None
    return "NONE", "OPS", 0, total, claims(n, k, gamma, beta, O["point"], O["value_q"], M["point"], M["value_q"], time)


def check_claims(cl, ops_evals, mem_evals, rt_eval, m_eval):
    """ops_evals = (a, wv, rv, rt)(z_ops), mem_evals = (init, fin, ft)(z_mem), rt_eval = rt(z_f), m_eval = m(z_t) -> "NONE", or the first
    claim that fails: "OPS", "MEM", "RT", "M" """
    if sum(co * v for co, v in zip(cl["ops_coeff"], ops_evals)) % P != cl["ops_value"]:
        return "OPS"
    if sum(co * v for co, v in zip(cl["mem_coeff"], mem_evals)) % P != cl["mem_value"]:
        return "MEM"
    if rt_eval % P != cl["rt_value"]:
        return "RT"
    return "NONE" if m_eval % P == cl["m_value"] else "M"


def evaluations(tr, cl):
    """the columns' multilinear extensions at the claims' points: what the caller opens"""
    return ([F.mle_at(tr[c], cl["z_ops"]) for c in ("a", "wv", "rv", "rt")], [F.mle_at(tr[c], cl["z_mem"]) for c in ("init", "fin", "ft")],
            F.mle_at(tr["rt"], cl["z_f"]), F.mle_at(tr["m"], cl["z_t"]))


def random_ops(n, k, seed, pattern_name="random"):
    """(addr, wv, init): 2^n operations on 2^k cells.  pattern_name: "random", "one address", "last cell", "distinct" (each cell at most
    once, n < k leaves cells untouched) or "round robin" (operation i on cell i mod 3: three runs of a third of the operations each, so
    that in sorted order a run of 2^10 / 3 or more keys lies across an edge between workgroups of 256).  The values include 0 and
    p - 1"""
    rng = random.Random(seed)
    rows, cells = 1 << n, 1 << k
    if pattern_name == "one address":
        addr = [rng.randrange(cells)] * rows
    elif pattern_name == "last cell":
        addr = [cells - 1] * rows
    elif pattern_name == "distinct":
        addr = [(3 * i + 1) % cells for i in range(rows)] if rows <= cells else None
    elif pattern_name == "round robin":
        addr = [i % min(cells, 3) for i in range(rows)]
    else:
        addr = [rng.randrange(cells) for _ in range(rows)]
    if addr is None:
        raise ValueError("distinct addresses need n <= k")
    wv = [rng.choice((0, P - 1, rng.randrange(P))) if i % 3 == 0 else rng.randrange(P) for i in range(rows)]
    init = [rng.choice((0, P - 1, rng.randrange(P))) if j % 3 == 0 else rng.randrange(P) for j in range(cells)]
    return addr, wv, init
