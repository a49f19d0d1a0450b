"""The sparse-matrix evaluation proof (Spark) of include/provekit_spark.h on Python ints: the outer IO pattern, the challenges, the
committed and the per-query columns, a prover that writes whole proof bytes and a verifier that names the check, the side and the layer
it fails at, the claims with their coefficients, the stacked flattening of an R1CS and M~(rx, ry) by its definition.  Written from the
header's protocol text over tests/prodcheck_refs.py (the product sumcheck and the sponge) and tests/tuplelookup_refs.py (the two ROM
lookups).  TEST INFRASTRUCTURE ONLY; small sizes (pure Python).

Values are canonical ints throughout; Montgomery form exists only at the library's boundary (K.mont / K.unmont).  A matrix is a dict of
its entry list row_idx, col_idx (2^n ints each) and the five committed columns row, col, val (2^n), m_row (2^s), m_col (2^t); a query
adds e_row and e_col (2^n)."""
import random

import fracsum_refs as F
import prodcheck_refs as K
import tuplelookup_refs as T

P = K.P
V = K.V
LABEL = b"provekit-hip/spark/v1"
SIDES = ("VAL", "ROW", "COL")
COLUMNS = ("row", "col", "val", "m_row", "m_col", "e_row", "e_col")
WHICH = ("NONE", "VAL", "E_ROW", "E_COL", "ROW", "M_ROW", "COL", "M_COL")


def legal(n, s, t, n_bind=0):
    return 1 <= n <= 28 and 1 <= s <= 28 and 1 <= t <= 28 and 0 <= n_bind <= 16


def pattern(n, s, t, n_bind=0) -> bytes:
    ops = [b"A%dbind" % n_bind] * bool(n_bind) + [b"A%drx" % s, b"A%dry" % t, b"S3seeds"]
    return LABEL + b"/n%d/s%d/t%d" % (n, s, t) + b"".join(b"\0" + op for op in ops)


def val_shape(n):
    return K.Shape("triple", n, 1)  # one term of three tables, no tau, one bind element: the seed


def side_bytes(n, s, t):
    return [val_shape(n).proof_bytes(), T.proof_bytes(n, s, 2, 1), T.proof_bytes(n, t, 2, 1)]


def proof_bytes(n, s, t) -> int:
    return sum(side_bytes(n, s, t))


def challenges(n, s, t, rx, ry, bind=()):
    """[seed_VAL, seed_ROW, seed_COL] of the statement, its bind elements and the point"""
    M = K.Merlin(pattern(n, s, t, len(bind)))
    M.public(list(bind))
    M.public(list(rx))
    M.public(list(ry))
    seeds = M.a.challenge_scalars(3)
    assert M.a.done()
    return seeds


def eq_table(r):
    """eq(r, j) for j < 2^len(r), coordinate 0 <-> the most significant bit of j"""
    return K.pr.eq_table(list(r))


def eq_at(r, y):
    e = 1
    for a, b in zip(r, y):
        e = e * K.eq1(a, b) % P
    return e


def index_at(z):
    """I(z) = sum_j z_j 2^(v-1-j): the extension of x -> x, variable 0 the most significant bit"""
    acc = 0
    for zj in z:
        acc = (2 * acc + zj) % P
    return acc


def matrix(n, s, t, row_idx, col_idx, val):
    """the committed columns of an entry list of exactly 2^n entries (padding (0, 0, 0) included by the caller)"""
    assert len(row_idx) == len(col_idx) == len(val) == 1 << n and all(r < 1 << s for r in row_idx) and all(c < 1 << t for c in col_idx)
    m_row, m_col = [0] * (1 << s), [0] * (1 << t)
    for r, c in zip(row_idx, col_idx):
        m_row[r] += 1
        m_col[c] += 1
    return {"row_idx": list(row_idx), "col_idx": list(col_idx), "row": list(row_idx), "col": list(col_idx), "val": [v % P for v in val], "m_row": m_row, "m_col": m_col}


def query(M, rx, ry):
    """the matrix's columns with the per-query ones"""
    er, ec = eq_table(rx), eq_table(ry)
    return dict(M, e_row=[er[r] for r in M["row_idx"]], e_col=[ec[c] for c in M["col_idx"]])


def value(M, rx, ry):
    """sum_k val[k] eq(rx, row[k]) eq(ry, col[k]): what the sumcheck proves"""
    er, ec = eq_table(rx), eq_table(ry)
    return sum(v * er[r] * ec[c] for v, r, c in zip(M["val"], M["row_idx"], M["col_idx"])) % P


def dense_value(M, s, t, rx, ry):
    """M~(rx, ry) by its definition: the dense matrix (duplicates add), then its multilinear extension"""
    dense = [[0] * (1 << t) for _ in range(1 << s)]
    for v, r, c in zip(M["val"], M["row_idx"], M["col_idx"]):
        dense[r][c] = (dense[r][c] + v) % P
    er, ec = eq_table(rx), eq_table(ry)
    return sum(er[i] * ec[j] * dense[i][j] for i in range(1 << s) for j in range(1 << t)) % P


def claims(n, s, t, v, z_val, finals, look):
    """look: the two lookups' claims (T.claims' dicts), ROW then COL"""
    return {"value": v, "z_val": list(z_val), "val_values": list(finals), "beta": [c["beta"] for c in look], "z_f": [list(c["z_lo"]) for c in look],
            "f_coeff": [list(c["f_coeff"][0]) for c in look], "f_value": [c["f_value"] for c in look], "z_m": [list(c["z_t"]) for c in look],
            "m_value": [c["m_value"] for c in look]}


def prove(n, s, t, Q, rx, ry, bind=(), validate=True, table_rx=None, table_ry=None):
    """Q: a query's columns -> dict: proof, the claims' fields.  validate=False: a proof is written also when a lookup fails.  table_rx,
    table_ry: other points than the statement's for the two lookups' tables, for proofs built to fail exactly the table check"""
    assert all(len(Q[c]) == 1 << n for c in ("row", "col", "val", "e_row", "e_col")) and len(Q["m_row"]) == 1 << s and len(Q["m_col"]) == 1 << t
    seeds = challenges(n, s, t, rx, ry, bind)
    proof, z_val, finals, v = K.prove(val_shape(n), [Q["val"], Q["e_row"], Q["e_col"]], None, [seeds[0]])
    look = []
    for idx, e, m, bits, point, seed in ((Q["row"], Q["e_row"], Q["m_row"], s, table_rx or rx, seeds[1]), (Q["col"], Q["e_col"], Q["m_col"], t, table_ry or ry, seeds[2])):
        L = T.prove(n, bits, [[idx, e]], [list(range(1 << bits)), eq_table(point)], m, [seed], validate)
        proof += L["proof"]
        look.append(L)
    out = claims(n, s, t, v, z_val, finals, look)
    out["proof"] = proof
    return out


def verify(n, s, t, proof, rx, ry, bind=(), expected=None, pat=None):
    """-> ("NONE", "VAL", 0, total, claims dict) or (the failed check's name, the side, the layer, the offset within the whole proof or
    None where the sumcheck verifier states it, None)"""
    part = side_bytes(n, s, t)
    at, total = [0, part[0], part[0] + part[1]], sum(part)
    if len(proof) < total:
        return "TRANSCRIPT_SHORT", "VAL", 0, len(proof), None
    if len(proof) > total:
        return "TRAILING_BYTES", "VAL", 0, total, None
    try:
        public = list(bind) + list(rx) + list(ry)
        A = V.Arthur(pat or pattern(n, s, t, len(bind)), b"".join((x % P).to_bytes(32, "little") for x in public))
        A.next_scalars(len(bind))
        A.next_scalars(s)
        A.next_scalars(t)
        seeds = A.challenge_scalars(3)
        if not A.done():
            return "IO_PATTERN", "VAL", 0, 0, None
    except V.VerifyError as err:
        return F._outer_error(err), "VAL", 0, 0, None
    check, z_val, finals = K.verify(val_shape(n), proof[: part[0]], None, [seeds[0]], expected)
    if check != "NONE":
        return check, "VAL", 0, None, None
    v = int.from_bytes(proof[:32], "little")
    look = []
    for side, bits, point in ((1, s, rx), (2, t, ry)):
        check, _, lay, offset, got = T.verify(n, bits, 2, 1, proof[at[side] : at[side] + part[side]], [seeds[side]])
        if check != "NONE":
            return check, SIDES[side], lay, None if offset is None else offset + at[side], None
        if got["t_value"] != (index_at(got["z_t"]) + got["beta"] * eq_at(point, got["z_t"])) % P:
            return "TABLE", SIDES[side], 0, at[side] + part[side], None
        look.append(got)
    return "NONE", "VAL", 0, total, claims(n, s, t, v, z_val, finals, look)


def check_claims(cl, val_evals, row_evals, m_row_eval, col_evals, m_col_eval):
    """val_evals = (val, e_row, e_col)(z_val), row_evals = (row, e_row)(z_f[0]), m_row_eval = m_row(z_m[0]), col_evals, m_col_eval the
    same of side COL -> "NONE", or the first claim that fails, in WHICH's order"""
    for j in range(3):
        if val_evals[j] % P != cl["val_values"][j]:
            return WHICH[1 + j]
    for side, (evs, m_eval) in enumerate(((row_evals, m_row_eval), (col_evals, m_col_eval))):
        if sum(co * v for co, v in zip(cl["f_coeff"][side], evs)) % P != cl["f_value"][side]:
            return ("ROW", "COL")[side]
        if m_eval % P != cl["m_value"][side]:
            return ("M_ROW", "M_COL")[side]
    return "NONE"


def evaluations(Q, cl):
    """the nine evaluations of the claims: what the caller opens"""
    return ([F.mle_at(Q[c], cl["z_val"]) for c in ("val", "e_row", "e_col")], [F.mle_at(Q[c], cl["z_f"][0]) for c in ("row", "e_row")], F.mle_at(Q["m_row"], cl["z_m"][0]),
            [F.mle_at(Q[c], cl["z_f"][1]) for c in ("col", "e_col")], F.mle_at(Q["m_col"], cl["z_m"][1]))


def stack_r1cs(num_constraints, mats, interner, n, s):
    """mats: three CSR triples (new_row_indices, col_indices, values) with values indexing `interner` -> (row_idx, col_idx, val) of 2^n
    entries: stacked row = matrix 2^s + row, matrices in order, CSR order, padding (0, 0, 0)"""
    rows, cols, vals = [], [], []
    for g, (starts, col_indices, values) in enumerate(mats):
        for r in range(num_constraints):
            to = starts[r + 1] if r + 1 < num_constraints else len(col_indices)
            for e in range(starts[r], to):
                rows.append((g << s) + r), cols.append(col_indices[e]), vals.append(interner[values[e]])
    pad = (1 << n) - len(rows)
    assert pad >= 0
    return rows + [0] * pad, cols + [0] * pad, vals + [0] * pad


def random_r1cs(num_constraints, num_witnesses, per_row, seed):
    """three random CSR matrices over one interner: column 0 (the constant-one witness) is in every row of A"""
    rng = random.Random(seed)
    interner = [1, P - 1] + [rng.randrange(P) for _ in range(6)]
    mats = []
    for g in range(3):
        starts, col_indices, values = [], [], []
        for r in range(num_constraints):
            starts.append(len(col_indices))
            cs = sorted(rng.sample(range(num_witnesses), min(per_row, num_witnesses) if (r + g) % 3 else 1))
            if g == 0 and 0 not in cs:
                cs = [0] + cs
            for c in cs:
                col_indices.append(c), values.append(rng.randrange(len(interner)))
        mats.append((starts, col_indices, values))
    return mats, interner


def random_entries(n, s, t, seed, pattern_name="random"):
    """(row_idx, col_idx, val): 2^n entries.  pattern_name: "random", "one column" (full skew: every entry in column 0 -- the
    constant-one witness), "distinct" (every row index and every column index at most once where the matrix has room, else a
    permutation pattern), "duplicates" (one position many times: they add) or "padding" ((0, 0, 0) throughout).  The values include 0
    and p - 1"""
    rng = random.Random(seed)
    entries, rows, cols = 1 << n, 1 << s, 1 << t
    val = [rng.choice((0, P - 1, rng.randrange(P))) if k % 3 == 0 else rng.randrange(P) for k in range(entries)]
    if pattern_name == "one column":
        return [rng.randrange(rows) for _ in range(entries)], [0] * entries, val
    if pattern_name == "distinct":
        return [(5 * k + 1) % rows for k in range(entries)], [(3 * k + 2) % cols for k in range(entries)], val
    if pattern_name == "duplicates":
        r, c = rng.randrange(rows), rng.randrange(cols)
        return [r if k % 2 else rng.randrange(rows) for k in range(entries)], [c if k % 2 else rng.randrange(cols) for k in range(entries)], val
    if pattern_name == "padding":
        return [0] * entries, [0] * entries, [0] * entries
    return [rng.randrange(rows) for _ in range(entries)], [rng.randrange(cols) for _ in range(entries)], val


def eq_hi(u, g):
    return T.eq_hi(u, g)
