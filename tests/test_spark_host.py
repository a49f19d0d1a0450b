"""CPU: libprovekit_spark.so's host side.  The header/library/binding symbol match and what the library links; the outer IO pattern
and the proof length against the reference's; every refusal with its reason; pkx_verify on proofs the Python reference prover builds
(tests/spark_refs.py): acceptance with the reference's claims, field for field, every tampering with the check, the side, the layer
and the offset both verifiers must name, and each of the verifier's own checks reached by a proof built to fail exactly it (TABLE on
either side, SUM); a proof for one rx under another; pkx_check_claims; the stacked flattening of an R1CS and the one query that serves
its three matrices; hostile framing through the sanitizer build of the host verifier (a program of its own, run as a subprocess)."""
import ctypes
import itertools
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
HEADER = os.path.join(ROOT, "include", "provekit_spark.h")
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pkx_verify_asan")

import fracsum_refs as F  # noqa: E402
import prodcheck_refs as K  # noqa: E402
import spark_refs as X  # noqa: E402

P = K.P
NEEDED = {"libprovekit_tuplelookup.so", "libprovekit_fracsum.so", "libprovekit_sumcheck.so", "libprovekit_hip.so"}


def test_the_header_declares_what_the_library_exports_and_the_binding_binds():
    from provekit_amd import spark as sp, tuplelookup as tl

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pkx_[a-z0-9_]+)\s*\(", src)))
    nm = subprocess.run(["nm", "-D", "--defined-only", sp.SPARK_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" [A-Za-z] (pkx_[a-z0-9_]+)$", nm, flags=re.M)))
    assert declared == exported == sorted(sp.SIGNATURES) and len(exported) == 16
    assert ctypes.CDLL(sp.SPARK_LIB_PATH).pkx_abi_version() == 1
    assert ctypes.sizeof(sp.StatementStruct) == 16 and ctypes.sizeof(sp.ClaimsStruct) == 32 * (1 + 28 + 3 + 2 + 2 * 28 + 4 + 2 + 2 * 28 + 2)
    # the names below it, then the one of this library's own, numbered after PKF_CHECK_COUNT
    assert sp.CHECKS[: len(tl.CHECKS)] == tl.CHECKS and sp.CHECKS[len(tl.CHECKS) :] == ("TABLE",)
    assert [sp.lib.pkx_check_name(i).decode() for i in range(len(sp.CHECKS))] == list(sp.CHECKS)
    assert sp.count_lds_max() == 12
    # the library calls the product, the sumcheck and the tuple-lookup library only through their C ABIs; neither WHIR nor the verify library
    und = subprocess.run(["nm", "-D", "--undefined-only", sp.SPARK_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\b_ZN2pk\w+", und) and not re.findall(r"\b_ZN3pk[sft]\w+", und) and not re.findall(r"\bpk[vwlgm]_\w+", und), und
    inc = os.path.join(ROOT, "include")

    def names(prefix, header):
        return set(re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % prefix, open(os.path.join(inc, header)).read()))

    assert set(re.findall(r"\bpk_\w+", und)) == {"pk_malloc", "pk_free", "pk_ctx_sync", "pk_eq_table"} <= names("pk", "provekit_hip.h")
    assert {"pkt_prove", "pkt_verify", "pkt_prover_create", "pkt_proof_bytes", "pkt_prover_arena_bytes"} <= set(re.findall(r"\bpkt_\w+", und)) <= names("pkt", "provekit_tuplelookup.h")
    assert {"pks_prove", "pks_verify", "pks_prover_create", "pks_proof_bytes"} <= set(re.findall(r"\bpks_\w+", und)) <= names("pks", "provekit_sumcheck.h")
    assert set(re.findall(r"\bpkf_\w+", und)) <= {"pkf_check_name"}
    needed = subprocess.run(["readelf", "-d", sp.SPARK_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\[(libprovekit_\w+\.so)\]", needed)) == NEEDED


STATEMENTS = list(itertools.product((1, 2, 9, 28), (1, 5, 28), (1, 7, 28), (0, 2, 16)))


def test_io_patterns_and_proof_lengths_are_the_references_and_differ_between_statements():
    from provekit_amd import prodcheck as pc, spark as sp, tuplelookup as tl

    pats = {}
    for n, s, t, n_bind in STATEMENTS:
        stmt = sp.Statement(n, s, t, n_bind)
        pat = pats[(n, s, t, n_bind)] = sp.io_pattern(stmt)
        assert pat == X.pattern(n, s, t, n_bind), (n, s, t, n_bind)
        want = pc.proof_bytes(X.val_shape(n).statement()) + tl.proof_bytes(tl.Statement(n, s, 2, 1, 1)) + tl.proof_bytes(tl.Statement(n, t, 2, 1, 1))
        assert sp.proof_bytes(stmt) == X.proof_bytes(n, s, t) == want
    assert len(set(pats.values())) == len(pats)
    assert pats[(9, 5, 7, 0)].split(b"\0") == [sp.LABEL + b"/n9/s5/t7", b"A5rx", b"A7ry", b"S3seeds"]
    assert pats[(9, 5, 7, 2)].split(b"\0") == [sp.LABEL + b"/n9/s5/t7", b"A2bind", b"A5rx", b"A7ry", b"S3seeds"]


REFUSALS = [((0, 1, 1), "n must be"), ((29, 1, 1), "n must be"), ((4, 0, 1), "s must be"), ((4, 29, 1), "s must be"), ((4, 1, 0), "t must be"), ((4, 1, 29), "t must be"),
            ((4, 2, 2, 17), "n_bind must be")]


@pytest.mark.parametrize("stmt, reason", REFUSALS)
def test_every_refusal_is_made_with_a_reason(stmt, reason):
    from provekit_amd import spark as sp
    from provekit_amd._lib import ProveKitHipError

    s = sp.Statement(*stmt)
    for call in (sp.io_pattern, sp.proof_bytes, sp.arena_bytes):
        with pytest.raises(ProveKitHipError, match=reason) as e:
            call(s)
        assert e.value.code == -1
    st, r, which = s.struct(), sp.ResultStruct(), ctypes.c_int(0)  # the verifier refuses the statement before it looks at anything else
    assert sp.lib.pkx_verify(ctypes.addressof(st), None, 0, None, None, None, None, None, 0, None, None, None, ctypes.byref(r)) == -1
    assert re.search(reason, sp.lib.pkx_create_error().decode())
    cl, ev = sp.ClaimsStruct(), K.mont([0] * 4)
    d = ev.ctypes.data
    assert sp.lib.pkx_check_claims(ctypes.addressof(st), ctypes.addressof(cl), d, d, d, d, d, ctypes.byref(which)) == -1
    assert re.search(reason, sp.lib.pkx_create_error().decode())


def test_verify_refuses_elements_that_do_not_match_the_statement():
    from provekit_amd import spark as sp
    from provekit_amd._lib import ProveKitHipError

    too_big = np.array([[2**64 - 1] * 4], dtype=np.uint64)
    stmt = sp.Statement(3, 1, 1, 1)
    st, r, one = stmt.struct(), sp.ResultStruct(), K.mont([1])
    assert sp.lib.pkx_verify(ctypes.addressof(st), None, 0, None, None, None, None, None, 0, None, None, None, ctypes.byref(r)) == -1
    assert b"(rx, ry) is the statement: pass it" in sp.lib.pkx_create_error()
    assert sp.lib.pkx_verify(ctypes.addressof(st), None, 0, one.ctypes.data, one.ctypes.data, None, None, None, 0, None, None, None, ctypes.byref(r)) == -1
    assert b"binds elements: pass" in sp.lib.pkx_create_error()
    for kw, reason in ((dict(rx=too_big), "rx element 0"), (dict(ry=too_big), "ry element 0"), (dict(bind=too_big), "bind element 0"), (dict(expected_value=too_big[0]), "expected_value element 0")):
        args = dict(rx=one, ry=one, bind=one)
        args.update(kw)
        with pytest.raises(ProveKitHipError, match=reason + " is not below p") as e:
            sp.verify(stmt, b"", **args)
        assert e.value.code == -1


SIZES = [(1, 1, 1), (2, 3, 1), (3, 1, 2), (4, 3, 3)]


class Case:
    def __init__(self, n, s, t):
        self.n, self.s, self.t = n, s, t
        seed = 100 * n + 10 * s + t
        self.M = X.matrix(n, s, t, *X.random_entries(n, s, t, seed))
        self.rx, self.ry, self.bind = K.random_elements(s, seed + 1), K.random_elements(t, seed + 2), K.random_elements(2, seed=9)
        self.Q = X.query(self.M, self.rx, self.ry)
        self.ref = X.prove(n, s, t, self.Q, self.rx, self.ry, self.bind)
        self.part = X.side_bytes(n, s, t)
        self.at = [0, self.part[0], self.part[0] + self.part[1]]

    def stmt(self):
        from provekit_amd import spark as sp

        return sp.Statement(self.n, self.s, self.t, 2)

    def both(self, proof, bind=None, pattern=None, rx=None, ry=None, expected=None):
        """the library's verdict, after asserting that the reference names the same check, side, layer and (where it states one) offset"""
        from provekit_amd import spark as sp

        bind, rx, ry = self.bind if bind is None else bind, self.rx if rx is None else rx, self.ry if ry is None else ry
        check, side, layer, offset, seen = X.verify(self.n, self.s, self.t, proof, rx, ry, bind, expected, pattern)
        res, lib_side, lib_layer, claims = sp.verify(self.stmt(), proof, K.mont(rx), K.mont(ry), K.mont(bind), None if expected is None else K.mont([expected])[0], pattern)
        assert (res.check, lib_side, lib_layer) == (check, side, layer) and res.accepted == (check == "NONE"), (res, lib_side, lib_layer, check, side, layer)
        assert offset is None or res.offset == offset, (res, offset)
        return res, lib_side, lib_layer, claims, seen


@pytest.fixture(scope="module")
def cases():
    return {size: Case(*size) for size in SIZES}


def _same_claims(claims, ref):
    assert K.unmont(claims.value) == [ref["value"]]
    assert K.unmont(claims.z_val) == ref["z_val"] and K.unmont(claims.val_values) == ref["val_values"]
    for side in range(2):
        assert K.unmont(claims.beta[side]) == [ref["beta"][side]] and K.unmont(claims.f_value[side]) == [ref["f_value"][side]]
        assert K.unmont(claims.m_value[side]) == [ref["m_value"][side]]
        for name in ("z_f", "f_coeff", "z_m"):
            assert K.unmont(getattr(claims, name)[side]) == ref[name][side], (name, side)


def _lib_check(c, claims, evs):
    from provekit_amd import spark as sp

    v, r, mr, co, mc = evs
    return sp.check_claims(c.stmt(), claims, K.mont(v), K.mont(r), K.mont([mr]), K.mont(co), K.mont([mc]))


@pytest.mark.parametrize("size", SIZES)
def test_reference_proofs_are_accepted_with_the_references_claims_and_the_claims_hold(cases, size):
    from provekit_amd import spark as sp
    from provekit_amd._lib import ProveKitHipError

    c = cases[size]
    ref = c.ref
    # what is proved is the matrix's extension by its definition
    assert ref["value"] == X.value(c.M, c.rx, c.ry) == X.dense_value(c.M, c.s, c.t, c.rx, c.ry)
    res, side, layer, claims, seen = c.both(ref["proof"])
    assert res.accepted and (side, layer) == ("VAL", 0) and res.offset == len(ref["proof"]) == X.proof_bytes(*size) and res.message == ""
    _same_claims(claims, ref)
    _same_claims(claims, seen)
    assert ref["f_coeff"] == [[1, ref["beta"][0]], [1, ref["beta"][1]]]
    # with the value expected
    assert c.both(ref["proof"], expected=ref["value"])[0].accepted
    # the nine evaluations are the columns' extensions at the five points: what the caller opens
    evs = X.evaluations(c.Q, ref)
    assert X.check_claims(ref, *evs) == "NONE" and _lib_check(c, claims, evs) == "NONE"
    # each of the nine evaluations off by one fails the claim it belongs to
    places = [(0, 0, "VAL"), (0, 1, "E_ROW"), (0, 2, "E_COL"), (1, 0, "ROW"), (1, 1, "ROW"), (2, None, "M_ROW"), (3, 0, "COL"), (3, 1, "COL"), (4, None, "M_COL")]
    for group, j, name in places:
        bad = [list(e) if isinstance(e, list) else e for e in evs]
        if j is None:
            bad[group] = (bad[group] + 1) % P
        else:
            bad[group][j] = (bad[group][j] + 1) % P
        assert _lib_check(c, claims, bad) == X.check_claims(ref, *bad) == name, (group, j)
    # the first failing claim is named
    bad = [list(e) if isinstance(e, list) else e for e in evs]
    bad[0][2], bad[2] = (bad[0][2] + 1) % P, (bad[2] + 1) % P
    assert _lib_check(c, claims, bad) == "E_COL"
    with pytest.raises(ProveKitHipError, match="m_col_eval element 0 is not below p"):
        sp.check_claims(c.stmt(), claims, K.mont(evs[0]), K.mont(evs[1]), K.mont([evs[2]]), K.mont(evs[3]), np.array([[2**64 - 1] * 4], dtype=np.uint64))
    # the caller's own pattern bytes
    assert c.both(ref["proof"], pattern=X.pattern(*size, 2))[0].accepted


def _bump(proof, element, delta=1):
    t = bytearray(proof)
    v = (int.from_bytes(t[32 * element : 32 * element + 32], "little") + delta) % P
    t[32 * element : 32 * element + 32] = v.to_bytes(32, "little")
    return bytes(t)


def _set(proof, element, value):
    t = bytearray(proof)
    t[32 * element : 32 * element + 32] = (value % P).to_bytes(32, "little")
    return bytes(t)


def _chains(c):
    """the four fractional-sum proofs inside a proof: (side, first byte, variables, unit)"""
    return [("ROW", c.at[1], c.n, 1), ("ROW", c.at[1] + F.proof_bytes(c.n, 1), c.s, 0), ("COL", c.at[2], c.n, 1), ("COL", c.at[2] + F.proof_bytes(c.n, 1), c.t, 0)]


@pytest.mark.parametrize("size", SIZES)
def test_every_tampering_is_rejected_at_the_named_check_side_layer_and_offset(cases, size):
    c = cases[size]
    n, s, t = size
    proof = c.ref["proof"]
    # side VAL: the sum, every round's values, the finals.  Without an expected value a changed sum is the first round's failure
    res, side, layer, _, _ = c.both(_bump(proof, 0))
    assert (res.check, side, layer, res.offset) == ("ROUND", "VAL", 0, 32 * 5)
    res, side, layer, _, _ = c.both(_bump(proof, 0), expected=c.ref["value"])
    assert (res.check, side, layer, res.offset) == ("SUM", "VAL", 0, 32)
    for i in range(n):
        res, side, layer, _, _ = c.both(_bump(proof, 1 + 4 * i))  # h_i(0)
        assert (res.check, side, layer, res.offset) == ("ROUND", "VAL", 0, 32 * (1 + 4 * (i + 1)))
        res, side, layer, _, _ = c.both(_bump(proof, 1 + 4 * i + 3))  # h_i(3): the round's own sum stands, the next claim moves
        assert (res.check, side, layer) == ("ROUND" if i + 1 < n else "FINAL", "VAL", 0)
    for j in range(3):
        res, side, layer, _, _ = c.both(_bump(proof, 1 + 4 * n + j))
        assert (res.check, side, layer, res.offset) == ("FINAL", "VAL", 0, c.at[1])
    # each byte class of each of the four chains: a top value, s, a round value, a final
    for side_name, start, vars_, unit in _chains(c):
        at = start // 32
        for e in range(4):
            res, side, layer, _, _ = c.both(_bump(proof, at + e))
            assert not res.accepted and side == side_name, (side_name, e, res)
            if vars_ > 1:
                assert (res.check, layer) == ("SUM", 1), (side_name, e, res)
            elif unit and e < 2:
                assert (res.check, layer, res.offset) == ("UNIT", 0, start + 128)
            else:  # no layer: another fraction, which is not the other chain's; or the same fraction and another table claim
                assert (res.check, layer) in (("FRACTION", 0), ("TABLE", 0))
        for d in range(1, vars_):
            lay = at + F.layer_at(vars_, unit, d) // 32
            end = at + F.layer_at(vars_, unit, d + 1) // 32
            res, side, layer, _, _ = c.both(_bump(proof, lay))
            assert (res.check, side, layer, res.offset) == ("SUM", side_name, d, 32 * (lay + 1))
            res, side, layer, _, _ = c.both(_bump(proof, lay + 1))
            assert (res.check, side, layer, res.offset) == ("ROUND", side_name, d, 32 * (lay + 4))
            res, side, layer, _, _ = c.both(_bump(proof, end - 1))
            assert (res.check, side, layer, res.offset) == ("FINAL", side_name, d, 32 * end)
        res, side, layer, _, _ = c.both(_set(proof, at + 3, 0))
        assert (res.check, side, layer, res.offset) == ("DENOMINATOR", side_name, 0, start + 128)
    t_ = bytearray(proof)  # v + p: the same value mod p, not canonical on the wire
    v = int.from_bytes(t_[:32], "little") + P
    if v < 1 << 256:
        t_[:32] = v.to_bytes(32, "little")
        res, side, layer, _, _ = c.both(bytes(t_))
        assert (res.check, side, layer, res.offset) == ("NON_CANONICAL", "VAL", 0, 32)
    # a bind element enters nothing but the seeds: side VAL's first round no longer adds up... the round values do, the challenges move
    for e in range(2):
        changed = list(c.bind)
        changed[e] = (changed[e] + 1) % P
        res, side, layer, _, _ = c.both(proof, bind=changed)
        assert not res.accepted and side == "VAL" and res.check in ("ROUND", "FINAL")
    # framing: all three parts have a fixed length
    for cut in sorted({0, 31, 128, c.at[1] - 1, c.at[1], c.at[2], c.at[2] + 1, len(proof) - 1}):
        res, side, layer, _, _ = c.both(proof[:cut])
        assert (res.check, side, layer, res.offset) == ("TRANSCRIPT_SHORT", "VAL", 0, cut)
    for extra in (b"\0", bytes(32)):
        res, side, layer, _, _ = c.both(proof + extra)
        assert (res.check, side, layer, res.offset) == ("TRAILING_BYTES", "VAL", 0, len(proof))
    # another statement's pattern: other operations are IO_PATTERN; the same operations under another label are other seeds
    res, side, layer, _, _ = c.both(proof, pattern=X.pattern(n, s, t, 1))
    assert (res.check, side, layer, res.offset) == ("IO_PATTERN", "VAL", 0, 0)
    res, side, _, _, _ = c.both(proof, pattern=X.pattern(n, s, t, 2).replace(b"/v1/", b"/v2/"))
    assert not res.accepted and side == "VAL"


@pytest.mark.parametrize("size", SIZES)
def test_each_of_the_verifiers_own_checks_is_reached_by_a_proof_built_to_fail_exactly_it(cases, size):
    c = cases[size]
    n, s, t = size
    # TABLE on either side: every chain of the proof holds and the two fractions agree, over a lookup into eq of ANOTHER point
    other_rx, other_ry = [(x + 1) % P for x in c.rx], [(y + 1) % P for y in c.ry]
    forged = X.prove(n, s, t, dict(c.Q, e_row=X.query(c.M, other_rx, c.ry)["e_row"]), c.rx, c.ry, c.bind, table_rx=other_rx)
    res, side, layer, _, _ = c.both(forged["proof"])
    assert (res.check, side, layer, res.offset) == ("TABLE", "ROW", 0, c.at[2])
    forged = X.prove(n, s, t, dict(c.Q, e_col=X.query(c.M, c.rx, other_ry)["e_col"]), c.rx, c.ry, c.bind, table_ry=other_ry)
    res, side, layer, _, _ = c.both(forged["proof"])
    assert (res.check, side, layer, res.offset) == ("TABLE", "COL", 0, len(forged["proof"]))
    # SUM: the honest proof under another expected value
    res, side, layer, _, _ = c.both(c.ref["proof"], expected=(c.ref["value"] + 1) % P)
    assert (res.check, side, layer, res.offset) == ("SUM", "VAL", 0, 32)
    # a wrong e_row with the honest table is the lookup's FRACTION on its side; a wrong m the same
    for column, side_name in (("e_row", "ROW"), ("e_col", "COL"), ("m_row", "ROW"), ("m_col", "COL")):
        changed = dict(c.Q)
        changed[column] = [(changed[column][0] + 1) % P] + list(changed[column][1:])
        forged = X.prove(n, s, t, changed, c.rx, c.ry, c.bind, validate=False)
        res, side, layer, _, _ = c.both(forged["proof"])
        assert (res.check, side, layer) == ("FRACTION", side_name, 0), column
        assert res.offset == c.at[X.SIDES.index(side_name)] + F.proof_bytes(n, 1) + 128


@pytest.mark.parametrize("size", SIZES)
def test_a_proof_for_one_point_is_rejected_under_another(cases, size):
    c = cases[size]
    for rx, ry in (([(c.rx[0] + 1) % P] + c.rx[1:], c.ry), (c.rx, c.ry[:-1] + [(c.ry[-1] + 1) % P])):
        res, side, layer, _, _ = c.both(c.ref["proof"], rx=rx, ry=ry)
        assert not res.accepted and side == "VAL" and res.check in ("ROUND", "FINAL")  # other seeds: the first side's challenges move


def test_the_stacked_query_is_the_eq_combination_of_three_per_matrix_evaluations():
    from provekit_amd import spark as sp
    from provekit_amd._lib import ProveKitHipError

    nc, nw, s, t, n = 6, 7, 3, 3, 6
    mats, interner = X.random_r1cs(nc, nw, 3, seed=5)
    rows, cols, vals = X.stack_r1cs(nc, mats, interner, n, s)
    got = sp.entries_from_r1cs(nc, nw, mats, K.mont(interner), n, s, t)
    assert got[0].tolist() == rows and got[1].tolist() == cols and K.unmont(got[2]) == vals
    assert sum(len(m[1]) for m in mats) < 1 << n and rows[-1] == cols[-1] == vals[-1] == 0  # padding at the end
    rx, ry, u = K.random_elements(s, 1), K.random_elements(t, 2), K.random_elements(2, 3)
    per_matrix = []
    for g in range(3):
        r_g, c_g, v_g = X.stack_r1cs(nc, [mats[g]], interner, n, s)
        per_matrix.append(X.value(X.matrix(n, s, t, r_g, c_g, v_g), rx, ry))
    stacked = X.matrix(n, s + 2, t, rows, cols, vals)
    want = sum(X.eq_hi(u, g) * per_matrix[g] for g in range(3)) % P
    assert X.value(stacked, u + rx, ry) == X.dense_value(stacked, s + 2, t, u + rx, ry) == want
    # and the one query is proved and verified as any other
    Q = X.query(stacked, u + rx, ry)
    ref = X.prove(n, s + 2, t, Q, u + rx, ry)
    res, side, layer, claims = sp.verify(sp.Statement(n, s + 2, t), ref["proof"], K.mont(u + rx), K.mont(ry), expected_value=K.mont([want])[0])
    assert res.accepted and K.unmont(claims.value) == [want]
    assert sp.verify(sp.Statement(n, s + 2, t), ref["proof"], K.mont(u + rx), K.mont(ry), expected_value=K.mont([(want + 1) % P])[0])[0].check == "SUM"
    # refusals carry their reason
    for args, reason in (((nc, nw, mats, K.mont(interner), 3, s, t), "2\\^n is below"), ((nc, nw, mats, K.mont(interner), n, 2, t), "2\\^s is below"),
                         ((nc, nw, mats, K.mont(interner), n, s, 2), "2\\^t is below"), ((nc, nw, mats, K.mont(interner), n, 27, t), "s must be"),
                         ((nc, nw, mats, K.mont(interner[:2]), n, s, t), "value index is outside"), ((nc, 3, mats, K.mont(interner), n, s, t), "column is outside")):
        with pytest.raises(ProveKitHipError, match=reason) as e:
            sp.entries_from_r1cs(*args)
        assert e.value.code == -1


def _blob(head, pat, bind, point, proofs):
    blob = struct.pack("<%dI" % len(head), *head) + struct.pack("<I", len(pat)) + pat + K.mont(bind).tobytes() + K.mont(point).tobytes()
    return blob + struct.pack("<I", len(proofs)) + b"".join(struct.pack("<Q", len(p)) + p for p in proofs)


def test_hostile_framing_and_counts_under_the_sanitizers(cases, tmp_path):
    """the host verifier alone, with the three verifiers below it, built with -fsanitize=address,undefined as a program of its own (make
    -C provekit_amd/csrc asan): proofs cut at every kind of place and grown, from exact-size heap blocks; statements whose counts would
    size buffers if they were believed"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pkx_verify_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}

    def run(blob):
        f = tmp_path / "cases.bin"
        f.write_bytes(blob)
        p = subprocess.run([ASAN, "verify", str(f)], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        return p.stdout.splitlines()

    for size in ((3, 1, 2), (2, 3, 1)):
        c = cases[size]
        proof, b1, b2 = c.ref["proof"], c.at[1], c.at[2]
        rng = np.random.default_rng(1)
        changed = dict(c.Q, e_row=[(c.Q["e_row"][0] + 1) % P] + c.Q["e_row"][1:])
        hostile = {"honest": proof, "zero length": b"", "one byte": b"\1", "all ones": b"\xff" * len(proof), "extended": proof + bytes(64),
                   "random bytes": rng.integers(0, 256, size=len(proof), dtype=np.uint8).tobytes(),
                   "random lookups": proof[:b1] + rng.integers(0, 256, size=len(proof) - b1, dtype=np.uint8).tobytes(),
                   "random tail": proof[:b2] + rng.integers(0, 256, size=len(proof) - b2, dtype=np.uint8).tobytes(),
                   "parts rotated": proof[b1:] + proof[:b1], "an e_row changed": X.prove(*size, changed, c.rx, c.ry, c.bind, validate=False)["proof"]}
        for cut in (1, 31, 33, b1 - 1, b1, b1 + 1, b1 + 127, b2 - 1, b2, b2 + 1, len(proof) - 1):
            hostile[f"cut at {cut}"] = proof[:cut]
        for pat in (b"", X.pattern(*size, 2)):
            lines = run(_blob(list(size) + [2], pat, c.bind, c.rx + c.ry, list(hostile.values())))
            assert len(lines) == len(hostile)
            for (name, bad), line in zip(hostile.items(), lines):
                rc, accepted, check, side, layer, offset = line.split()[:6]
                want = X.verify(*size, bad, c.rx, c.ry, c.bind)
                assert (rc, check, accepted, side, layer) == ("0", want[0], "1" if want[0] == "NONE" else "0", str(X.SIDES.index(want[1])), str(want[2])), (name, line)
                assert int(offset) <= max(len(bad), len(proof))
    for bad in ([2**31, 1, 1, 0], [5, 2**32 - 1, 1, 0], [5, 2, 2**31, 0], [5, 2, 2, 2**30], [29, 2, 2, 0], [0, 0, 0, 0]):
        # nothing after the statement: a count that was believed would read past the block
        lines = run(struct.pack("<4I", *bad))
        assert lines and lines[0].startswith("-1 0 REFUSED"), (bad, lines)
