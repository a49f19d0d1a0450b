"""CPU: libprovekit_bitwise.so's host side.  The header/library/binding symbol match and what the library links; pkb_plan against the
reference's for all 3 x 12 x 4 shapes (op, d, L), every refusal with its reason; the formula of the table's extension against the
brute-force extension of the table's rows; the outer IO pattern and the proof length against the reference's; pkb_verify on proofs the
Python reference prover builds (tests/bitwise_refs.py): acceptance with the reference's claims, field for field, every tampering with
the check, the side, the layer and the offset both verifiers must name, the table check reached by a proof built to fail exactly it;
pkb_check_claims, each of the five claims named; hostile framing through the sanitizer build of the host verifier (a program of its own,
run as a subprocess)."""
import ctypes
import os
import random
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
HEADER = os.path.join(ROOT, "include", "provekit_bitwise.h")
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pkb_verify_asan")

import bitwise_refs as B  # noqa: E402
import fracsum_refs as F  # noqa: E402
import prodcheck_refs as K  # noqa: E402
import tuplelookup_refs as T  # noqa: E402

P = K.P
NEEDED = {"libprovekit_tuplelookup.so", "libprovekit_fracsum.so", "libprovekit_sumcheck.so", "libprovekit_hip.so"}


def test_the_header_declares_what_the_library_exports_and_the_binding_binds():
    from provekit_amd import bitwise as bw, tuplelookup as tl

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pkb_[a-z0-9_]+)\s*\(", src)))
    nm = subprocess.run(["nm", "-D", "--defined-only", bw.BITWISE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" [A-Za-z] (pkb_[a-z0-9_]+)$", nm, flags=re.M)))
    assert declared == exported == sorted(bw.SIGNATURES) and len(exported) == 15
    assert ctypes.CDLL(bw.BITWISE_LIB_PATH).pkb_abi_version() == 1
    assert ctypes.sizeof(bw.StatementStruct) == 20 and ctypes.sizeof(bw.PlanStruct) == 28 and ctypes.sizeof(bw.ClaimsStruct) == 32 * (28 + 28 + 12 + 1 + 4 + 1)
    # the names below it, then the one of this library's own, numbered after PKF_CHECK_COUNT
    assert bw.CHECKS[: len(tl.CHECKS)] == tl.CHECKS and bw.CHECKS[len(tl.CHECKS) :] == ("TABLE",)
    assert [bw.lib.pkb_check_name(i).decode() for i in range(len(bw.CHECKS))] == list(bw.CHECKS)
    assert bw.count_lds_max_d() == 6  # 2^(2 d) <= 2^12 bins
    assert (bw.AND, bw.XOR, bw.OR) == (B.AND, B.XOR, B.OR) and B.LABEL == bw.LABEL
    # the library calls the product and the tuple-lookup library only through their C ABIs; neither WHIR nor the verify library
    und = subprocess.run(["nm", "-D", "--undefined-only", bw.BITWISE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\b_ZN2pk\w+", und) and not re.findall(r"\b_ZN3pk[sftxr]\w+", und) and not re.findall(r"\bpk[vwlgmxsr]_\w+", und), und
    inc = os.path.join(ROOT, "include")

    def names(prefix, header):
        return set(re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % prefix, open(os.path.join(inc, header)).read()))

    assert set(re.findall(r"\bpk_\w+", und)) == {"pk_malloc", "pk_free", "pk_ctx_sync"} <= names("pk", "provekit_hip.h")
    assert {"pkt_prove", "pkt_verify", "pkt_prover_create", "pkt_proof_bytes", "pkt_prover_arena_bytes"} <= set(re.findall(r"\bpkt_\w+", und)) <= names("pkt", "provekit_tuplelookup.h")
    assert set(re.findall(r"\bpkf_\w+", und)) <= {"pkf_check_name"}
    needed = subprocess.run(["readelf", "-d", bw.BITWISE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\[(libprovekit_\w+\.so)\]", needed)) == NEEDED


def test_the_plan_is_the_references_for_every_shape():
    from provekit_amd import bitwise as bw

    seen = 0
    for op in B.OPS:
        for d in range(1, 13):
            for L in range(1, 5):
                want = B.plan(d, L)
                assert B.legal(4, op, d, L)
                got = bw.plan(bw.Statement(4, op, d, L))
                assert (got.bits, got.k, got.c, got.digit_of) == (want["bits"], want["k"], want["c"], want["digit_of"]), (op, d, L)
                # what the plan promises: the digits cover the bits, the groups fill the lookup, the spare group is digit 0
                assert got.bits == L * d <= 48 and got.c in (1, 2, 4) and L <= got.c < 2 * L and got.digit_of[:L] == list(range(L)) and set(got.digit_of[L:]) <= {0}
                seen += 1
    assert seen == 144
    assert B.plan(8, 4) == {"bits": 32, "k": 16, "c": 4, "digit_of": [0, 1, 2, 3]} and B.plan(6, 3)["digit_of"] == [0, 1, 2, 0] and B.plan(5, 1)["c"] == 1
    # n + log2 c <= 28
    assert bw.plan(bw.Statement(28, B.AND, 8, 1)).c == 1 and bw.plan(bw.Statement(27, B.XOR, 8, 2)).c == 2 and bw.plan(bw.Statement(26, B.OR, 8, 3)).c == 4


# the bounds and their neighbours: d = 0 / 13, L = 0 / 5, n + log2 c = 29, n_bind = 17, an unknown op (stmt: n, op, d, L[, n_bind])
REFUSALS = [((0, 0, 8, 4), "n must be"), ((29, 0, 8, 1), "n must be"), ((4, 3, 8, 4), "op must be"), ((4, 2**31, 8, 4), "op must be"), ((4, 0, 0, 4), "d must be"),
            ((4, 1, 13, 4), "d must be"), ((4, 2, 8, 0), "L must be"), ((4, 0, 8, 5), "L must be"), ((28, 1, 8, 2), "n \\+ log2 c must be at most 28"),
            ((27, 1, 8, 3), "n \\+ log2 c must be at most 28"), ((27, 2, 12, 4), "n \\+ log2 c must be at most 28"), ((4, 0, 8, 4, 17), "n_bind must be")]
NEIGHBOURS = [(1, 0, 1, 1), (28, 2, 12, 1), (27, 1, 12, 2), (26, 0, 12, 3), (26, 1, 12, 4), (4, 2, 8, 4, 16)]  # the last statements the library takes


@pytest.mark.parametrize("stmt, reason", REFUSALS)
def test_every_refusal_is_made_with_a_reason(stmt, reason):
    from provekit_amd import bitwise as bw
    from provekit_amd._lib import ProveKitHipError

    assert not B.legal(*stmt)
    s = bw.Statement(*stmt)
    for call in (bw.plan, bw.io_pattern, bw.proof_bytes, bw.arena_bytes):
        with pytest.raises(ProveKitHipError, match=reason) as e:
            call(s)
        assert e.value.code == -1
    st, r, which = s.struct(), bw.ResultStruct(), ctypes.c_int(0)  # the verifier refuses the statement before it looks at anything else
    assert bw.lib.pkb_verify(ctypes.addressof(st), None, 0, None, None, 0, None, None, None, ctypes.byref(r)) == -1
    assert re.search(reason, bw.lib.pkb_create_error().decode())
    cl, ev = bw.ClaimsStruct(), K.mont([0] * 15)
    d = ev.ctypes.data
    assert bw.lib.pkb_check_claims(ctypes.addressof(st), ctypes.addressof(cl), d, d, d, ctypes.byref(which)) == -1
    assert re.search(reason, bw.lib.pkb_create_error().decode())


def test_the_neighbours_of_every_bound_are_taken():
    from provekit_amd import bitwise as bw

    for stmt in NEIGHBOURS:
        assert B.legal(*stmt)
        s = bw.Statement(*stmt)
        assert bw.plan(s).bits == stmt[2] * stmt[3] and bw.proof_bytes(s) == B.proof_bytes(*stmt[:4]) and bw.arena_bytes(s) > 0


def test_verify_refuses_elements_that_do_not_match_the_statement():
    from provekit_amd import bitwise as bw
    from provekit_amd._lib import ProveKitHipError

    stmt = bw.Statement(3, B.XOR, 2, 2, 1)
    st, r = stmt.struct(), bw.ResultStruct()
    assert bw.lib.pkb_verify(ctypes.addressof(st), None, 0, None, None, 0, None, None, None, ctypes.byref(r)) == -1
    assert b"binds elements: pass" in bw.lib.pkb_create_error()
    with pytest.raises(ProveKitHipError, match="bind element 0 is not below p") as e:
        bw.verify(stmt, b"", bind=np.array([[2**64 - 1] * 4], dtype=np.uint64))
    assert e.value.code == -1


def brute_force_extension(col, z):
    """sum_y col[y] eq(z, y), variable 0 the most significant bit of y"""
    v = len(z)
    acc = 0
    for y, value in enumerate(col):
        e = 1
        for i, zi in enumerate(z):
            e = e * (zi if (y >> (v - 1 - i)) & 1 else 1 - zi) % P
        acc = (acc + value * e) % P
    return acc


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("op", B.OPS)
def test_the_tables_formula_is_the_brute_force_extension_of_its_rows(op, d):
    rows = B.table(op, d)
    assert len(rows) == 3 and all(len(col) == 1 << (2 * d) for col in rows)
    assert all(rows[2][(u << d) | v] == B.apply(op, u, v) and rows[0][(u << d) | v] == u and rows[1][(u << d) | v] == v for u in range(1 << d) for v in range(1 << d))
    rng = random.Random(100 * op + d)
    points = [[rng.randrange(P) for _ in range(2 * d)] for _ in range(4)]
    points += [[(y >> (2 * d - 1 - i)) & 1 for i in range(2 * d)] for y in range(1 << (2 * d))]  # every 0/1 point: the rows themselves
    points += [[rng.choice((0, 1, rng.randrange(P))) for _ in range(2 * d)] for _ in range(4)]  # mixed
    for z in points:
        u, v, o = B.uvo_at(op, d, z)
        assert [u, v, o] == [brute_force_extension(col, z) for col in rows], (op, d, z)
        beta = rng.randrange(P)
        compressed = [(rows[0][y] + beta * rows[1][y] + beta * beta * rows[2][y]) % P for y in range(1 << (2 * d))]
        assert B.table_at(op, d, z, beta) == brute_force_extension(compressed, z)
    for y in range(1 << (2 * d)):  # on a 0/1 point the formula is the row
        assert B.uvo_at(op, d, points[4 + y]) == (rows[0][y], rows[1][y], rows[2][y])


STATEMENTS = [(n, op, d, L, n_bind) for n in (1, 9, 26) for op in B.OPS for d, L in ((1, 1), (8, 4), (6, 3), (12, 4), (10, 1), (4, 2)) for n_bind in (0, 3, 16)]


def test_io_patterns_and_proof_lengths_are_the_references_and_differ_between_statements():
    from provekit_amd import bitwise as bw, tuplelookup as tl

    pats = {}
    for n, op, d, L, n_bind in STATEMENTS:
        stmt = bw.Statement(n, op, d, L, n_bind)
        pat = pats[(n, op, d, L, n_bind)] = bw.io_pattern(stmt)
        assert pat == B.pattern(n, op, d, L, n_bind), (n, op, d, L, n_bind)
        assert bw.proof_bytes(stmt) == B.proof_bytes(n, op, d, L) == tl.proof_bytes(tl.Statement(n, 2 * d, 3, B.plan(d, L)["c"], 1))
    assert len(set(pats.values())) == len(pats)
    assert pats[(9, B.XOR, 8, 4, 0)].split(b"\0") == [bw.LABEL + b"/xor/n9/d8/l4", b"S1seed"]
    assert pats[(9, B.AND, 8, 4, 3)].split(b"\0") == [bw.LABEL + b"/and/n9/d8/l4", b"A3bind", b"S1seed"]
    assert pats[(9, B.OR, 6, 3, 3)].split(b"\0") == [bw.LABEL + b"/or/n9/d6/l3", b"A3bind", b"S1seed"]
    s = lambda d, L: bw.proof_bytes(bw.Statement(9, B.AND, d, L))  # noqa: E731
    assert s(4, 1) < s(4, 2) < s(4, 3) == s(4, 4) < s(5, 4)


SIZES = [(1, 1, 1), (2, 2, 2), (2, 2, 3), (3, 3, 4)]  # (n, d, L): c = 1, 2, 4 (spare), 4
CASES = [(op,) + size for size in SIZES for op in B.OPS]


class Case:
    def __init__(self, op, n, d, L):
        self.op, self.n, self.d, self.L = op, n, d, L
        self.plan = B.plan(d, L)
        self.a, self.b = B.columns(n, d, L, "edges")
        self.c, self.digits, self.m = B.decompose(op, d, L, self.a, self.b)
        self.bind = K.random_elements(2, seed=9)
        self.ref = B.prove(n, op, d, L, self.digits, self.m, self.bind)
        self.len_f = F.proof_bytes(n + T.log2c(self.plan["c"]), 1)

    def size(self):
        return self.n, self.op, self.d, self.L

    def stmt(self, op=None):
        from provekit_amd import bitwise as bw

        return bw.Statement(self.n, self.op if op is None else op, self.d, self.L, 2)

    def both(self, proof, bind=None, pattern=None):
        """the library's verdict, after asserting that the reference names the same check, side, layer and (where it states one) offset"""
        from provekit_amd import bitwise as bw

        bind = self.bind if bind is None else bind
        check, side, layer, offset, seen = B.verify(*self.size(), proof, bind, pattern)
        res, lib_side, lib_layer, claims = bw.verify(self.stmt(), proof, K.mont(bind), pattern)
        assert (res.check, lib_side, lib_layer) == (check, side, layer) and res.accepted == (check == "NONE"), (res, lib_side, lib_layer, check, side, layer)
        assert offset is None or res.offset == offset, (res, offset)
        return res, lib_side, lib_layer, claims, seen


@pytest.fixture(scope="module")
def cases():
    return {case: Case(*case) for case in CASES}


def same_claims(claims, ref):
    for name in ("z_lo", "z_t", "pow2"):
        assert K.unmont(getattr(claims, name)) == ref[name], name
    assert [K.unmont(row) for row in claims.digit_coeff] == ref["digit_coeff"]
    assert K.unmont(claims.digits_value) == [ref["digits_value"]] and K.unmont(claims.m_value) == [ref["m_value"]]


def lib_check(c, claims, evs):
    from provekit_amd import bitwise as bw

    abc, digit_evals, m_eval = evs
    return bw.check_claims(c.stmt(), claims, K.mont(abc), K.mont([v for part in digit_evals for v in part]), K.mont([m_eval]))


@pytest.mark.parametrize("case", CASES)
def test_reference_proofs_are_accepted_with_the_references_claims_and_each_claim_is_named(cases, case):
    from provekit_amd import bitwise as bw
    from provekit_amd._lib import ProveKitHipError

    c = cases[case]
    ref, pl, L, d = c.ref, c.plan, c.L, c.d
    # the digits recompose the columns, c is the operation, and m counts every group
    for col, part in zip((c.a, c.b, c.c), c.digits):
        assert all(sum(part[i][x] << (d * i) for i in range(L)) == col[x] for x in range(1 << c.n))
    assert all(c.c[x] == B.apply(c.op, c.a[x], c.b[x]) for x in range(1 << c.n)) and sum(c.m) == pl["c"] << c.n
    res, side, layer, claims, seen = c.both(ref["proof"])
    assert res.accepted and (side, layer) == ("F", 0) and res.offset == len(ref["proof"]) == B.proof_bytes(*c.size()) and res.message == ""
    same_claims(claims, ref)
    same_claims(claims, seen)
    assert ref["pow2"] == [1 << (d * i) for i in range(L)]
    # the five claims hold of the columns' extensions at the two points: what the caller opens
    evs = B.evaluations((c.a, c.b, c.c), c.digits, c.m, ref)
    assert B.check_claims(ref, *evs) == "NONE" and lib_check(c, claims, evs) == "NONE"
    # the lookup's own claim, over all c groups, is the same statement: the spare group is group 0's columns again
    groups = B.groups_of(d, L, c.digits)
    look = T.verify(c.n, 2 * d, 3, pl["c"], ref["proof"], [B.seed_of(*c.size(), c.bind)])[4]
    t_evals = list(B.uvo_at(c.op, d, look["z_t"]))
    assert T.check_claims(look, [[F.mle_at(col, look["z_lo"]) for col in cols] for cols in groups], t_evals, evs[2]) == "NONE"
    # each evaluation off by one fails the claim it belongs to; the first failing claim is named
    abc, digit_evals, m_eval = evs
    for j, name in enumerate(("RECOMPOSE_A", "RECOMPOSE_B", "RECOMPOSE_C")):
        bad = list(abc)
        bad[j] = (bad[j] + 1) % P
        assert lib_check(c, claims, (bad, digit_evals, m_eval)) == B.check_claims(ref, bad, digit_evals, m_eval) == name
        assert lib_check(c, claims, (bad, digit_evals, (m_eval + 1) % P)) == name  # before M
        for i in range(L):
            off = [list(part) for part in digit_evals]
            off[j][i] = (off[j][i] + 1) % P
            assert lib_check(c, claims, (abc, off, m_eval)) == B.check_claims(ref, abc, off, m_eval) == "DIGITS", (j, i)
            # a digit changed together with its column so that they still recompose: the lookup's claim alone catches it
            moved = list(abc)
            moved[j] = (moved[j] + (1 << (d * i))) % P
            assert lib_check(c, claims, (moved, off, m_eval)) == "DIGITS"
    assert lib_check(c, claims, (abc, digit_evals, (m_eval + 1) % P)) == B.check_claims(ref, abc, digit_evals, (m_eval + 1) % P) == "M"
    assert lib_check(c, claims, ([(v + 1) % P for v in abc], digit_evals, m_eval)) == "RECOMPOSE_A"  # the first of three
    # a column whose digits are right but whose word differs: another column's evaluation in c's place is named as c's recomposition
    if abc[2] != abc[0]:
        assert lib_check(c, claims, ([abc[0], abc[1], abc[0]], digit_evals, m_eval)) == B.check_claims(ref, [abc[0], abc[1], abc[0]], digit_evals, m_eval) == "RECOMPOSE_C"
    big = np.array([[2**64 - 1] * 4], dtype=np.uint64)
    flat = K.mont([v for part in digit_evals for v in part])
    with pytest.raises(ProveKitHipError, match="m_eval element 0 is not below p"):
        bw.check_claims(c.stmt(), claims, K.mont(abc), flat, big)
    with pytest.raises(ProveKitHipError, match="digit_evals element %d is not below p" % (3 * L - 1)):
        bw.check_claims(c.stmt(), claims, K.mont(abc), np.concatenate([flat[:-1], big]), K.mont([m_eval]))
    with pytest.raises(ProveKitHipError, match="abc_evals element 2 is not below p"):
        bw.check_claims(c.stmt(), claims, np.concatenate([K.mont(abc)[:2], big]), flat, K.mont([m_eval]))
    # the caller's own pattern bytes
    assert c.both(ref["proof"], pattern=B.pattern(*c.size(), 2))[0].accepted


def _bump(proof, element, delta=1):
    t = bytearray(proof)
    v = (int.from_bytes(t[32 * element : 32 * element + 32], "little") + delta) % P
    t[32 * element : 32 * element + 32] = v.to_bytes(32, "little")
    return bytes(t)


def _set(proof, element, value):
    t = bytearray(proof)
    t[32 * element : 32 * element + 32] = (value % P).to_bytes(32, "little")
    return bytes(t)


def other_seed(c, res, side):
    """a proof under another seed is rejected on side F, where the seed is absorbed first; a side F without a layer (one variable) holds
    no challenge but its last point, so there the first thing that moves is on side T: its chain of 2 d >= 2 variables, the fractions
    or the table claim.  (`both` has already required the reference's verdict to be the same.)"""
    return not res.accepted and (side == "F" or (c.n + T.log2c(c.plan["c"]) == 1 and side == "T"))


@pytest.mark.parametrize("case", CASES)
def test_every_tampering_is_rejected_at_the_named_check_side_layer_and_offset(cases, case):
    c = cases[case]
    n, op, d, L = c.size()
    proof = c.ref["proof"]
    # each byte class of each of the two chains: a top value, a layer's s, a round value, a final
    for side_name, start, vars_, unit in (("F", 0, n + T.log2c(c.plan["c"]), 1), ("T", c.len_f, 2 * d, 0)):
        at = start // 32
        for e in range(4):
            res, side, layer, _, _ = c.both(_bump(proof, at + e))
            assert not res.accepted, (side_name, e, res)
            if vars_ > 1:
                assert (res.check, side, layer) == ("SUM", side_name, 1), (side_name, e, res)
            elif unit and e < 2:
                assert (res.check, side, layer, res.offset) == ("UNIT", side_name, 0, start + 128)
            else:  # no layer: another fraction, which is not the other chain's; or the same fraction and another table claim
                assert (res.check, side, layer) in (("FRACTION", "T", 0), ("TABLE", "T", 0))
        for e in range(1, vars_):
            lay = at + F.layer_at(vars_, unit, e) // 32
            end = at + F.layer_at(vars_, unit, e + 1) // 32
            res, side, layer, _, _ = c.both(_bump(proof, lay))
            assert (res.check, side, layer, res.offset) == ("SUM", side_name, e, 32 * (lay + 1))
            res, side, layer, _, _ = c.both(_bump(proof, lay + 1))
            assert (res.check, side, layer, res.offset) == ("ROUND", side_name, e, 32 * (lay + 4))
            res, side, layer, _, _ = c.both(_bump(proof, end - 1))
            assert (res.check, side, layer, res.offset) == ("FINAL", side_name, e, 32 * end)
        res, side, layer, _, _ = c.both(_set(proof, at + 3, 0))
        assert (res.check, side, layer, res.offset) == ("DENOMINATOR", side_name, 0, start + 128)
    t_ = bytearray(proof)  # v + p: the same value mod p, not canonical on the wire
    v = int.from_bytes(t_[:32], "little") + P
    if v < 1 << 256:
        t_[:32] = v.to_bytes(32, "little")
        res, side, layer, _, _ = c.both(bytes(t_))
        assert (res.check, side, layer) == ("NON_CANONICAL", "F", 0)
    # a flipped bit in every region: the first and the last element of each side
    for at in (0, c.len_f - 1, c.len_f, len(proof) - 32):
        t_ = bytearray(proof)
        t_[at] ^= 1
        res, side, layer, _, _ = c.both(bytes(t_))
        assert not res.accepted and res.check != "NONE", (at, res)
    # a bind element enters nothing but the seed: the lookup's challenges move
    for e in range(2):
        changed = list(c.bind)
        changed[e] = (changed[e] + 1) % P
        res, side, layer, _, _ = c.both(proof, bind=changed)
        assert other_seed(c, res, side)
    # framing: the proof has a fixed length
    for cut in sorted({0, 31, 128, c.len_f - 1, c.len_f, c.len_f + 1, len(proof) - 1}):
        res, side, layer, _, _ = c.both(proof[:cut])
        assert (res.check, side, layer, res.offset) == ("TRANSCRIPT_SHORT", "F", 0, cut)
    for extra in (b"\0", bytes(32)):
        res, side, layer, _, _ = c.both(proof + extra)
        assert (res.check, side, layer, res.offset) == ("TRAILING_BYTES", "F", 0, len(proof))
    # another statement's pattern: other operations are IO_PATTERN; the same operations under another label are another seed
    res, side, layer, _, _ = c.both(proof, pattern=B.pattern(n, op, d, L, 1))
    assert (res.check, side, layer, res.offset) == ("IO_PATTERN", "F", 0, 0)
    res, side, _, _, _ = c.both(proof, pattern=B.pattern(n, op, d, L, 2).replace(b"/v1/", b"/v2/"))
    assert other_seed(c, res, side)


@pytest.mark.parametrize("size", SIZES)
def test_the_table_check_is_reached_by_a_proof_over_another_operations_table(cases, size):
    """a proof built by the reference under the AND statement's label, but over the XOR table with c = a XOR b: every chain holds, the
    fractions agree, pkt_verify accepts -- and the table is not AND's.  The same for every ordered pair of operations"""
    from provekit_amd import tuplelookup as tl

    n, d, L = size
    for op in B.OPS:
        c = cases[(op,) + size]
        for other in B.OPS:
            if other == op:
                continue
            _, digits, m = B.decompose(other, d, L, c.a, c.b)
            forged = B.prove(n, op, d, L, digits, m, c.bind, table_op=other)
            seed = B.seed_of(n, op, d, L, c.bind)
            res, _, _, _ = tl.verify(tl.Statement(n, 2 * d, 3, c.plan["c"], 1), forged["proof"], K.mont([seed]))
            assert res.accepted, res
            res, side, layer, _, _ = c.both(forged["proof"])
            assert (res.check, side, layer, res.offset) == ("TABLE", "T", 0, len(forged["proof"])), (op, other)
            assert "its table is not the operation's" in res.message
        # a wrong digit with the honest table is the lookup's FRACTION; a wrong m the same
        bad = [[list(col) for col in part] for part in c.digits]
        bad[2][L - 1][0] ^= 1
        for digits, m in ((bad, c.m), (c.digits, [(c.m[0] + 1) % P] + c.m[1:])):
            forged = B.prove(n, op, d, L, digits, m, c.bind, validate=False)
            res, side, layer, _, _ = c.both(forged["proof"])
            assert (res.check, side, layer, res.offset) == ("FRACTION", "T", 0, c.len_f + 128)


@pytest.mark.parametrize("case", CASES)
def test_a_proof_for_one_operation_is_rejected_under_another(cases, case):
    from provekit_amd import bitwise as bw

    c = cases[case]
    for other in B.OPS:
        if other == c.op:
            continue  # the same lookup statement and length: the label differs, and the table
        assert bw.proof_bytes(c.stmt(other)) == len(c.ref["proof"])
        res, side, layer, _ = bw.verify(c.stmt(other), c.ref["proof"], K.mont(c.bind))
        assert other_seed(c, res, side), (other, res)
        assert B.verify(c.n, other, c.d, c.L, c.ref["proof"], c.bind)[0] == res.check
    if c.L < 3:  # another lookup statement: another length
        res, side, layer, _ = bw.verify(bw.Statement(c.n, c.op, c.d, 4, 2), c.ref["proof"], K.mont(c.bind))
        assert res.check == "TRANSCRIPT_SHORT"


def _blob(head, pat, bind, proofs):
    blob = struct.pack("<%dI" % len(head), *head) + struct.pack("<I", len(pat)) + pat + K.mont(bind).tobytes()
    return blob + struct.pack("<I", len(proofs)) + b"".join(struct.pack("<Q", len(p)) + p for p in proofs)


def test_hostile_framing_and_counts_under_the_sanitizers(cases, tmp_path):
    """the host verifier alone, with the three verifiers below it, built with -fsanitize=address,undefined as a program of its own (make
    -C provekit_amd/csrc asan): proofs cut at every kind of place and grown, from exact-size heap blocks; statements whose counts would
    size buffers if they were believed"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pkb_verify_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}

    def run(blob):
        f = tmp_path / "cases.bin"
        f.write_bytes(blob)
        p = subprocess.run([ASAN, "verify", str(f)], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        return p.stdout.splitlines()

    for case in ((B.XOR, 2, 2, 2), (B.AND, 3, 3, 4), (B.OR, 2, 2, 3)):
        c = cases[case]
        size = c.size()
        proof, b1 = c.ref["proof"], c.len_f
        rng = np.random.default_rng(1)
        bad = [[list(col) for col in part] for part in c.digits]
        bad[0][0][1] = 1 << c.d
        other = (c.op + 1) % 3
        hostile = {"honest": proof, "zero length": b"", "one byte": b"\1", "all ones": b"\xff" * len(proof), "extended": proof + bytes(64),
                   "random bytes": rng.integers(0, 256, size=len(proof), dtype=np.uint8).tobytes(),
                   "random tail": proof[:b1] + rng.integers(0, 256, size=len(proof) - b1, dtype=np.uint8).tobytes(),
                   "parts rotated": proof[b1:] + proof[:b1], "a digit changed": B.prove(*size, bad, c.m, c.bind, validate=False)["proof"],
                   "another table": B.prove(*size, *B.decompose(other, c.d, c.L, c.a, c.b)[1:], c.bind, table_op=other)["proof"]}
        for cut in (1, 31, 33, b1 - 1, b1, b1 + 1, b1 + 127, len(proof) - 1):
            hostile[f"cut at {cut}"] = proof[:cut]
        for pat in (b"", B.pattern(*size, 2)):
            lines = run(_blob(list(size) + [2], pat, c.bind, list(hostile.values())))
            assert len(lines) == len(hostile)
            for (name, bad_proof), line in zip(hostile.items(), lines):
                rc_, accepted, check, side, layer, offset = line.split()[:6]
                want = B.verify(*size, bad_proof, c.bind)
                assert (rc_, check, accepted, side, layer) == ("0", want[0], "1" if want[0] == "NONE" else "0", str(("F", "T").index(want[1])), str(want[2])), (name, line)
                assert int(offset) <= max(len(bad_proof), len(proof))
        assert [B.verify(*size, hostile[name], c.bind)[0] for name in ("honest", "a digit changed", "another table")] == ["NONE", "FRACTION", "TABLE"]
    for bad in ([2**31, 0, 8, 4, 0], [5, 2**32 - 1, 8, 4, 0], [5, 0, 2**31, 4, 0], [5, 0, 8, 2**31, 0], [5, 0, 8, 4, 2**30], [29, 0, 8, 1, 0], [5, 0, 13, 4, 0], [0, 0, 0, 0, 0]):
        # nothing after the statement: a count that was believed would read past the block
        lines = run(struct.pack("<5I", *bad))
        assert lines and lines[0].startswith("-1 0 REFUSED"), (bad, lines)
