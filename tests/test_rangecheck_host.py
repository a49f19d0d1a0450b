"""CPU: libprovekit_rangecheck.so's host side.  The header/library/binding symbol match and what the library links; pkr_plan against the
reference's for all 64 x 28 pairs (bits, k), every refusal with its reason; the outer IO pattern and the proof length against the
reference's; pkr_verify on proofs the Python reference prover builds (tests/rangecheck_refs.py): acceptance with the reference's
claims, field for field, every tampering with the check, the side, the layer and the offset both verifiers must name, the table check
reached by a proof built to fail exactly it; a proof for one `bits` under another; pkr_check_claims; hostile framing through the
sanitizer build of the host verifier (a program of its own, run as a subprocess)."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
HEADER = os.path.join(ROOT, "include", "provekit_rangecheck.h")
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pkr_verify_asan")

import fracsum_refs as F  # noqa: E402
import prodcheck_refs as K  # noqa: E402
import rangecheck_refs as R  # noqa: E402
import tuplelookup_refs as T  # noqa: E402

P = K.P
NEEDED = {"libprovekit_tuplelookup.so", "libprovekit_fracsum.so", "libprovekit_sumcheck.so", "libprovekit_hip.so"}
# the issue's table: (bits, k) -> (L, r, G, c), None: refused
PLANS = {(8, 8): (1, 8, 1, 1), (16, 8): (2, 8, 2, 2), (5, 8): (1, 5, 2, 2), (24, 8): (3, 8, 3, 4), (7, 4): (2, 3, 3, 4), (20, 8): (3, 4, 4, 4), (32, 12): (3, 8, 4, 4),
         (64, 16): (4, 16, 4, 4), (63, 16): None, (63, 21): (3, 21, 3, 4)}


def test_the_header_declares_what_the_library_exports_and_the_binding_binds():
    from provekit_amd import rangecheck as rc, tuplelookup as tl

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pkr_[a-z0-9_]+)\s*\(", src)))
    nm = subprocess.run(["nm", "-D", "--defined-only", rc.RANGECHECK_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" [A-Za-z] (pkr_[a-z0-9_]+)$", nm, flags=re.M)))
    assert declared == exported == sorted(rc.SIGNATURES) and len(exported) == 15
    assert ctypes.CDLL(rc.RANGECHECK_LIB_PATH).pkr_abi_version() == 1
    assert ctypes.sizeof(rc.StatementStruct) == 16 and ctypes.sizeof(rc.PlanStruct) == 48 and ctypes.sizeof(rc.ClaimsStruct) == 32 * (28 + 28 + 4 + 1 + 4 + 1)
    # the names below it, then the one of this library's own, numbered after PKF_CHECK_COUNT
    assert rc.CHECKS[: len(tl.CHECKS)] == tl.CHECKS and rc.CHECKS[len(tl.CHECKS) :] == ("TABLE",)
    assert [rc.lib.pkr_check_name(i).decode() for i in range(len(rc.CHECKS))] == list(rc.CHECKS)
    assert rc.count_lds_max_k() == 12
    # the library calls the product and the tuple-lookup library only through their C ABIs; neither WHIR nor the verify library
    und = subprocess.run(["nm", "-D", "--undefined-only", rc.RANGECHECK_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\b_ZN2pk\w+", und) and not re.findall(r"\b_ZN3pk[sftx]\w+", und) and not re.findall(r"\bpk[vwlgmxs]_\w+", und), und
    inc = os.path.join(ROOT, "include")

    def names(prefix, header):
        return set(re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % prefix, open(os.path.join(inc, header)).read()))

    assert set(re.findall(r"\bpk_\w+", und)) == {"pk_malloc", "pk_free", "pk_ctx_sync"} <= names("pk", "provekit_hip.h")
    assert {"pkt_prove", "pkt_verify", "pkt_prover_create", "pkt_proof_bytes", "pkt_prover_arena_bytes"} <= set(re.findall(r"\bpkt_\w+", und)) <= names("pkt", "provekit_tuplelookup.h")
    assert set(re.findall(r"\bpkf_\w+", und)) <= {"pkf_check_name"}
    needed = subprocess.run(["readelf", "-d", rc.RANGECHECK_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\[(libprovekit_\w+\.so)\]", needed)) == NEEDED


def test_the_plan_is_the_references_for_all_pairs_and_the_refusals_carry_a_reason():
    from provekit_amd import rangecheck as rc
    from provekit_amd._lib import ProveKitHipError

    legal = 0
    for bits in range(1, 65):
        for k in range(1, 29):
            want = R.plan(bits, k)
            assert R.legal(4, bits, k) == (want is not None)
            if want is None:
                with pytest.raises(ProveKitHipError, match=r"needs \d+ groups, at most 4 .*: k = (\d+) works") as e:
                    rc.plan(rc.Statement(4, bits, k))
                assert e.value.code == -1
                works = int(re.search(r"k = (\d+) works", str(e.value)).group(1))
                assert works == -(-bits // 3) and R.plan(bits, works) is not None  # the k it names works
                continue
            legal += 1
            got = rc.plan(rc.Statement(4, bits, k))
            assert (got.limbs, got.top_bits, got.groups, got.c, got.limb_of, got.shift_of) == (want["L"], want["r"], want["G"], want["c"], want["limb_of"], want["shift_of"]), (bits, k)
            # what the plan promises: the limbs cover the bits, the shifted top limb stays inside the table, the groups fill the lookup
            assert (got.limbs - 1) * k + got.top_bits == bits and 1 <= got.top_bits <= k and got.c in (1, 2, 4) and got.groups <= got.c < 2 * got.groups
    assert legal == 1157
    for bits in range(1, 65):  # every bits has a legal k, and every k >= ceil(bits / 3) is one
        assert all(R.plan(bits, k) is not None for k in range(-(-bits // 3), 29))
    for (bits, k), want in PLANS.items():
        pl = R.plan(bits, k)
        assert (None if pl is None else (pl["L"], pl["r"], pl["G"], pl["c"])) == want, (bits, k)
    assert R.plan(24, 8)["limb_of"] == [0, 1, 2, 0] and R.plan(20, 8)["limb_of"] == [0, 1, 2, 2] and R.plan(20, 8)["shift_of"] == [0, 0, 0, 4]
    # n + log2 c <= 28
    assert rc.plan(rc.Statement(28, 8, 8)).c == 1 and rc.plan(rc.Statement(27, 16, 8)).c == 2 and rc.plan(rc.Statement(26, 64, 16)).c == 4
    for stmt in ((28, 16, 8), (27, 64, 16)):
        with pytest.raises(ProveKitHipError, match="n \\+ log2 c must be at most 28"):
            rc.plan(rc.Statement(*stmt))
        assert not R.legal(*stmt)


STATEMENTS = [(n, bits, k, n_bind) for n in (1, 9, 26) for bits, k in ((1, 1), (8, 8), (5, 8), (24, 8), (32, 12), (64, 16), (64, 28)) for n_bind in (0, 3, 16)]


def test_io_patterns_and_proof_lengths_are_the_references_and_differ_between_statements():
    from provekit_amd import rangecheck as rc, tuplelookup as tl

    pats = {}
    for n, bits, k, n_bind in STATEMENTS:
        stmt = rc.Statement(n, bits, k, n_bind)
        pat = pats[(n, bits, k, n_bind)] = rc.io_pattern(stmt)
        assert pat == R.pattern(n, bits, k, n_bind), (n, bits, k, n_bind)
        assert rc.proof_bytes(stmt) == R.proof_bytes(n, bits, k) == tl.proof_bytes(tl.Statement(n, k, 1, R.plan(bits, k)["c"], 1))
    assert len(set(pats.values())) == len(pats)
    assert pats[(9, 32, 12, 0)].split(b"\0") == [rc.LABEL + b"/n9/b32/k12", b"S1seed"]
    assert pats[(9, 32, 12, 3)].split(b"\0") == [rc.LABEL + b"/n9/b32/k12", b"A3bind", b"S1seed"]
    assert rc.proof_bytes(rc.Statement(9, 8, 8)) < rc.proof_bytes(rc.Statement(9, 16, 8)) < rc.proof_bytes(rc.Statement(9, 24, 8)) == rc.proof_bytes(rc.Statement(9, 20, 8))


REFUSALS = [((0, 8, 8), "n must be"), ((29, 8, 8), "n must be"), ((4, 0, 8), "bits must be"), ((4, 65, 8), "bits must be"), ((4, 8, 0), "k must be"), ((4, 8, 29), "k must be"),
            ((4, 63, 16), "needs 5 groups"), ((4, 64, 8), "needs 8 groups"), ((4, 8, 8, 17), "n_bind must be")]


@pytest.mark.parametrize("stmt, reason", REFUSALS)
def test_every_refusal_is_made_with_a_reason(stmt, reason):
    from provekit_amd import rangecheck as rc
    from provekit_amd._lib import ProveKitHipError

    s = rc.Statement(*stmt)
    for call in (rc.plan, rc.io_pattern, rc.proof_bytes, rc.arena_bytes):
        with pytest.raises(ProveKitHipError, match=reason) as e:
            call(s)
        assert e.value.code == -1
    st, r, which = s.struct(), rc.ResultStruct(), ctypes.c_int(0)  # the verifier refuses the statement before it looks at anything else
    assert rc.lib.pkr_verify(ctypes.addressof(st), None, 0, None, None, 0, None, None, None, ctypes.byref(r)) == -1
    assert re.search(reason, rc.lib.pkr_create_error().decode())
    cl, ev = rc.ClaimsStruct(), K.mont([0] * 4)
    d = ev.ctypes.data
    assert rc.lib.pkr_check_claims(ctypes.addressof(st), ctypes.addressof(cl), d, d, d, ctypes.byref(which)) == -1
    assert re.search(reason, rc.lib.pkr_create_error().decode())


def test_verify_refuses_elements_that_do_not_match_the_statement():
    from provekit_amd import rangecheck as rc
    from provekit_amd._lib import ProveKitHipError

    stmt = rc.Statement(3, 8, 8, 1)
    st, r = stmt.struct(), rc.ResultStruct()
    assert rc.lib.pkr_verify(ctypes.addressof(st), None, 0, None, None, 0, None, None, None, ctypes.byref(r)) == -1
    assert b"binds elements: pass" in rc.lib.pkr_create_error()
    with pytest.raises(ProveKitHipError, match="bind element 0 is not below p") as e:
        rc.verify(stmt, b"", bind=np.array([[2**64 - 1] * 4], dtype=np.uint64))
    assert e.value.code == -1


SIZES = [(1, 1, 1), (3, 8, 8), (3, 16, 8), (2, 24, 8), (3, 7, 4), (2, 20, 8)]  # (n, bits, k): c = 1, 1, 2, 4 (spare), 4 (spare + top check), 4 (top check)


class Case:
    def __init__(self, n, bits, k):
        self.n, self.bits, self.k = n, bits, k
        self.plan = R.plan(bits, k)
        self.f = R.column(n, bits, k, "edges")
        self.limbs, self.m = R.decompose(bits, k, self.f)
        self.bind = K.random_elements(2, seed=9)
        self.ref = R.prove(n, bits, k, self.limbs, self.m, self.bind)
        self.len_f = F.proof_bytes(n + T.log2c(self.plan["c"]), 1)

    def stmt(self, bits=None):
        from provekit_amd import rangecheck as rc

        return rc.Statement(self.n, self.bits if bits is None else bits, self.k, 2)

    def both(self, proof, bind=None, pattern=None):
        """the library's verdict, after asserting that the reference names the same check, side, layer and (where it states one) offset"""
        from provekit_amd import rangecheck as rc

        bind = self.bind if bind is None else bind
        check, side, layer, offset, seen = R.verify(self.n, self.bits, self.k, proof, bind, pattern)
        res, lib_side, lib_layer, claims = rc.verify(self.stmt(), proof, K.mont(bind), pattern)
        assert (res.check, lib_side, lib_layer) == (check, side, layer) and res.accepted == (check == "NONE"), (res, lib_side, lib_layer, check, side, layer)
        assert offset is None or res.offset == offset, (res, offset)
        return res, lib_side, lib_layer, claims, seen


@pytest.fixture(scope="module")
def cases():
    return {size: Case(*size) for size in SIZES}


def same_claims(claims, ref):
    for name in ("z_lo", "z_t", "limb_coeff", "pow2"):
        assert K.unmont(getattr(claims, name)) == ref[name], name
    assert K.unmont(claims.limbs_value) == [ref["limbs_value"]] and K.unmont(claims.m_value) == [ref["m_value"]]


def lib_check(c, claims, evs):
    from provekit_amd import rangecheck as rc

    f_eval, limb_evals, m_eval = evs
    return rc.check_claims(c.stmt(), claims, K.mont([f_eval]), K.mont(limb_evals), K.mont([m_eval]))


@pytest.mark.parametrize("size", SIZES)
def test_reference_proofs_are_accepted_with_the_references_claims_and_the_claims_hold(cases, size):
    from provekit_amd import rangecheck as rc
    from provekit_amd._lib import ProveKitHipError

    c = cases[size]
    ref, pl = c.ref, c.plan
    # the limbs recompose the column, and m counts every group
    assert all(sum(c.limbs[i][x] << (c.k * i) for i in range(pl["L"])) == c.f[x] for x in range(1 << c.n)) and sum(c.m) == pl["c"] << c.n
    res, side, layer, claims, seen = c.both(ref["proof"])
    assert res.accepted and (side, layer) == ("F", 0) and res.offset == len(ref["proof"]) == R.proof_bytes(*size) and res.message == ""
    same_claims(claims, ref)
    same_claims(claims, seen)
    assert ref["pow2"] == [1 << (c.k * i) for i in range(pl["L"])]
    # the three claims hold of the columns' extensions at the two points: what the caller opens
    evs = R.evaluations(c.f, c.limbs, c.m, ref)
    assert R.check_claims(ref, *evs) == "NONE" and lib_check(c, claims, evs) == "NONE"
    # the lookup's own claim, over all c groups, is the same statement: the scaled and the spare column are multiples of limb columns
    groups = R.groups_of(c.bits, c.k, c.limbs)
    look = T.verify(c.n, c.k, 1, pl["c"], ref["proof"], [R.seed_of(c.n, c.bits, c.k, c.bind)])[4]
    assert T.check_claims(look, [[F.mle_at(col, look["z_lo"])] for col in groups], [R.index_at(look["z_t"])], evs[2]) == "NONE"
    # each evaluation off by one fails the claim it belongs to; the first failing claim is named
    f_eval, limb_evals, m_eval = evs
    assert lib_check(c, claims, ((f_eval + 1) % P, limb_evals, m_eval)) == R.check_claims(ref, (f_eval + 1) % P, limb_evals, m_eval) == "RECOMPOSE"
    assert lib_check(c, claims, (f_eval, limb_evals, (m_eval + 1) % P)) == R.check_claims(ref, f_eval, limb_evals, (m_eval + 1) % P) == "M"
    for i in range(pl["L"]):
        bad = list(limb_evals)
        bad[i] = (bad[i] + 1) % P
        assert lib_check(c, claims, (f_eval, bad, m_eval)) == R.check_claims(ref, f_eval, bad, m_eval) == "LIMBS", i
        # a limb changed together with f so that they still recompose: the lookup's claim alone catches it
        assert lib_check(c, claims, ((f_eval + (1 << (c.k * i))) % P, bad, (m_eval + 1) % P)) == "LIMBS"
    assert lib_check(c, claims, ((f_eval + 1) % P, limb_evals, (m_eval + 1) % P)) == "RECOMPOSE"
    with pytest.raises(ProveKitHipError, match="m_eval element 0 is not below p"):
        rc.check_claims(c.stmt(), claims, K.mont([f_eval]), K.mont(limb_evals), np.array([[2**64 - 1] * 4], dtype=np.uint64))
    with pytest.raises(ProveKitHipError, match="limb_evals element %d is not below p" % (pl["L"] - 1)):
        rc.check_claims(c.stmt(), claims, K.mont([f_eval]), np.concatenate([K.mont(limb_evals)[:-1], np.array([[2**64 - 1] * 4], dtype=np.uint64)]), K.mont([m_eval]))
    with pytest.raises(ProveKitHipError, match="f_eval element 0 is not below p"):
        rc.check_claims(c.stmt(), claims, np.array([[2**64 - 1] * 4], dtype=np.uint64), K.mont(limb_evals), K.mont([m_eval]))
    # the caller's own pattern bytes
    assert c.both(ref["proof"], pattern=R.pattern(*size, 2))[0].accepted


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
    """a proof under another seed is rejected on side F, where the seed is absorbed first; a side F without a layer holds no challenge
    but its last point, and there it is the fractions or the table claim that move"""
    return not res.accepted and (side == "F" or (c.n + T.log2c(c.plan["c"]) == 1 and res.check in ("FRACTION", "TABLE")))


@pytest.mark.parametrize("size", SIZES)
def test_every_tampering_is_rejected_at_the_named_check_side_layer_and_offset(cases, size):
    c = cases[size]
    n, bits, k = size
    proof = c.ref["proof"]
    # each byte class of each of the two chains: a top value, a layer's s, a round value, a final
    for side_name, start, vars_, unit in (("F", 0, n + T.log2c(c.plan["c"]), 1), ("T", c.len_f, k, 0)):
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
        assert (res.check, side, layer) == ("NON_CANONICAL", "F", 0)
    # a bind element enters nothing but the seed: the lookup's challenges move
    for e in range(2):
        changed = list(c.bind)
        changed[e] = (changed[e] + 1) % P
        res, side, layer, _, _ = c.both(proof, bind=changed)
        # (chains without a layer hold no challenge but their last points: there the table claim is what moves)
        assert other_seed(c, res, side)
    # framing: the proof has a fixed length
    for cut in sorted({0, 31, 128, c.len_f - 1, c.len_f, c.len_f + 1, len(proof) - 1}):
        res, side, layer, _, _ = c.both(proof[:cut])
        assert (res.check, side, layer, res.offset) == ("TRANSCRIPT_SHORT", "F", 0, cut)
    for extra in (b"\0", bytes(32)):
        res, side, layer, _, _ = c.both(proof + extra)
        assert (res.check, side, layer, res.offset) == ("TRAILING_BYTES", "F", 0, len(proof))
    # another statement's pattern: other operations are IO_PATTERN; the same operations under another label are another seed
    res, side, layer, _, _ = c.both(proof, pattern=R.pattern(n, bits, k, 1))
    assert (res.check, side, layer, res.offset) == ("IO_PATTERN", "F", 0, 0)
    res, side, _, _, _ = c.both(proof, pattern=R.pattern(n, bits, k, 2).replace(b"/v1/", b"/v2/"))
    assert other_seed(c, res, side)


@pytest.mark.parametrize("size", SIZES)
def test_the_table_check_is_reached_by_a_proof_over_another_table(cases, size):
    """the limbs plus one, looked up in (1, .., 2^k): every chain holds, the fractions agree, pkt_verify accepts -- and the table is not I_k"""
    from provekit_amd import tuplelookup as tl

    c = cases[size]
    n, bits, k = size
    moved = [[(v + 1) % P for v in col] for col in R.groups_of(bits, k, c.limbs)]
    forged = R.prove(n, bits, k, c.limbs, c.m, c.bind, table=list(range(1, (1 << k) + 1)), groups=moved)
    seed = R.seed_of(n, bits, k, c.bind)
    res, _, _, _ = tl.verify(tl.Statement(n, k, 1, c.plan["c"], 1), forged["proof"], K.mont([seed]))
    assert res.accepted, res
    res, side, layer, _, _ = c.both(forged["proof"])
    assert (res.check, side, layer, res.offset) == ("TABLE", "T", 0, len(forged["proof"]))
    assert "its table is not 0 .. 2^k - 1" in res.message
    # a wrong limb with the honest table is the lookup's FRACTION; a wrong m the same
    bad_limbs = [list(col) for col in c.limbs]
    bad_limbs[-1][0] = 1 << k
    for limbs, m in ((bad_limbs, c.m), (c.limbs, [(c.m[0] + 1) % P] + c.m[1:])):
        forged = R.prove(n, bits, k, limbs, m, c.bind, validate=False)
        res, side, layer, _, _ = c.both(forged["proof"])
        assert (res.check, side, layer, res.offset) == ("FRACTION", "T", 0, c.len_f + 128)


@pytest.mark.parametrize("size", SIZES)
def test_a_proof_for_one_bits_is_rejected_under_another(cases, size):
    from provekit_amd import rangecheck as rc

    c = cases[size]
    n, bits, k = size
    others = [b for b in range(1, 65) if b != bits and R.plan(b, k) is not None and R.plan(b, k)["c"] == c.plan["c"]]
    assert others or size == (1, 1, 1) or c.plan["c"] == 1
    for other in others[:3]:  # the same lookup statement and length: only the label differs
        assert rc.proof_bytes(c.stmt(other)) == len(c.ref["proof"])
        res, side, layer, _ = rc.verify(c.stmt(other), c.ref["proof"], K.mont(c.bind))
        assert other_seed(c, res, side), (other, res)
        assert R.verify(n, other, k, c.ref["proof"], c.bind)[0] == res.check
    # another lookup statement: another length
    if c.plan["c"] < 4:
        res, side, layer, _ = rc.verify(rc.Statement(n, 3 * k, k, 2), c.ref["proof"], K.mont(c.bind))
        assert res.check == "TRANSCRIPT_SHORT"


def _blob(head, pat, bind, proofs):
    blob = struct.pack("<%dI" % len(head), *head) + struct.pack("<I", len(pat)) + pat + K.mont(bind).tobytes()
    return blob + struct.pack("<I", len(proofs)) + b"".join(struct.pack("<Q", len(p)) + p for p in proofs)


def test_hostile_framing_and_counts_under_the_sanitizers(cases, tmp_path):
    """the host verifier alone, with the three verifiers below it, built with -fsanitize=address,undefined as a program of its own (make
    -C provekit_amd/csrc asan): proofs cut at every kind of place and grown, from exact-size heap blocks; statements whose counts would
    size buffers if they were believed"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pkr_verify_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}

    def run(blob):
        f = tmp_path / "cases.bin"
        f.write_bytes(blob)
        p = subprocess.run([ASAN, "verify", str(f)], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        return p.stdout.splitlines()

    for size in ((3, 16, 8), (3, 7, 4)):
        c = cases[size]
        proof, b1 = c.ref["proof"], c.len_f
        rng = np.random.default_rng(1)
        bad_limbs = [list(col) for col in c.limbs]
        bad_limbs[0][1] = 1 << c.k
        hostile = {"honest": proof, "zero length": b"", "one byte": b"\1", "all ones": b"\xff" * len(proof), "extended": proof + bytes(64),
                   "random bytes": rng.integers(0, 256, size=len(proof), dtype=np.uint8).tobytes(),
                   "random tail": proof[:b1] + rng.integers(0, 256, size=len(proof) - b1, dtype=np.uint8).tobytes(),
                   "parts rotated": proof[b1:] + proof[:b1], "a limb changed": R.prove(*size, bad_limbs, c.m, c.bind, validate=False)["proof"],
                   "another table": R.prove(*size, c.limbs, c.m, c.bind, table=list(range(1, (1 << c.k) + 1)),
                                            groups=[[(v + 1) % P for v in col] for col in R.groups_of(c.bits, c.k, c.limbs)])["proof"]}
        for cut in (1, 31, 33, b1 - 1, b1, b1 + 1, b1 + 127, len(proof) - 1):
            hostile[f"cut at {cut}"] = proof[:cut]
        for pat in (b"", R.pattern(*size, 2)):
            lines = run(_blob(list(size) + [2], pat, c.bind, list(hostile.values())))
            assert len(lines) == len(hostile)
            for (name, bad), line in zip(hostile.items(), lines):
                rc_, accepted, check, side, layer, offset = line.split()[:6]
                want = R.verify(*size, bad, c.bind)
                assert (rc_, check, accepted, side, layer) == ("0", want[0], "1" if want[0] == "NONE" else "0", str(("F", "T").index(want[1])), str(want[2])), (name, line)
                assert int(offset) <= max(len(bad), len(proof))
        assert [R.verify(*size, hostile[name], c.bind)[0] for name in ("honest", "a limb changed", "another table")] == ["NONE", "FRACTION", "TABLE"]
    for bad in ([2**31, 8, 8, 0], [5, 2**32 - 1, 8, 0], [5, 8, 2**31, 0], [5, 8, 8, 2**30], [29, 8, 8, 0], [5, 63, 16, 0], [0, 0, 0, 0]):
        # nothing after the statement: a count that was believed would read past the block
        lines = run(struct.pack("<4I", *bad))
        assert lines and lines[0].startswith("-1 0 REFUSED"), (bad, lines)
