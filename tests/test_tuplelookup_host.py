"""CPU: libprovekit_tuplelookup.so's host side.  The header/library/binding symbol match and what the library links; the outer IO
pattern and the proof length against the reference's; every refusal with its reason; pkt_verify on proofs the Python reference prover
builds (tests/tuplelookup_refs.py): acceptance with the reference's claims, field for field, and every tampering with the check, the
side, the layer and the offset both verifiers must name; pkt_check_claims; hostile framing through the sanitizer build of the host
verifier (a program of its own, run as a subprocess)."""
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
HEADER = os.path.join(ROOT, "include", "provekit_tuplelookup.h")
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pkt_verify_asan")

import fracsum_refs as F  # noqa: E402
import prodcheck_refs as K  # noqa: E402
import tuplelookup_refs as T  # noqa: E402

P = K.P


def test_the_header_declares_what_the_library_exports_and_the_binding_binds():
    from provekit_amd import fracsum as fs, tuplelookup as tl

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pkt_[a-z0-9_]+)\s*\(", src)))
    nm = subprocess.run(["nm", "-D", "--defined-only", tl.TUPLELOOKUP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" [A-Za-z] (pkt_[a-z0-9_]+)$", nm, flags=re.M)))
    assert declared == exported == sorted(tl.SIGNATURES) and len(exported) == 15
    assert ctypes.CDLL(tl.TUPLELOOKUP_LIB_PATH).pkt_abi_version() == 1
    assert ctypes.sizeof(tl.StatementStruct) == 20 and ctypes.sizeof(tl.ClaimsStruct) == 32 * (2 + 2 * 28 + 4 * 4 + 4 + 3)
    # no check numbers of its own: pkf's names, all of them
    assert tl.CHECKS == fs.CHECKS and [tl.lib.pkt_check_name(i).decode() for i in range(len(tl.CHECKS))] == list(fs.CHECKS)
    assert not re.search(r"#define PKT_CHECK_", open(HEADER).read())
    # the library calls the product and the fractional-sum library only through their C ABIs, and no other library above the product
    und = subprocess.run(["nm", "-D", "--undefined-only", tl.TUPLELOOKUP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\b_ZN2pk\w+", und) and not re.findall(r"\b_ZN3pk[sf]\w+", und) and not re.findall(r"\bpk[vwlg]_\w+", und), und
    inc = os.path.join(ROOT, "include")

    def names(prefix, header):
        return set(re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % prefix, open(os.path.join(inc, header)).read()))

    assert set(re.findall(r"\bpk_\w+", und)) == {"pk_malloc", "pk_free", "pk_ctx_sync"} <= names("pk", "provekit_hip.h")
    called = set(re.findall(r"\bpkf_\w+", und))
    assert {"pkf_prove", "pkf_verify", "pkf_prover_create", "pkf_proof_bytes"} <= called <= names("pkf", "provekit_fracsum.h")
    assert set(re.findall(r"\bpks_\w+", und)) <= names("pks", "provekit_sumcheck.h")
    needed = subprocess.run(["readelf", "-d", tl.TUPLELOOKUP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    libs = set(re.findall(r"\[(libprovekit_\w+\.so)\]", needed))
    assert libs == NEEDED, libs


# what the build gives: the sumcheck library is named on the link line and kept
NEEDED = {"libprovekit_fracsum.so", "libprovekit_sumcheck.so", "libprovekit_hip.so"}

STATEMENTS = [s for s in itertools.product((1, 2, 8, 27, 28), (1, 5, 28), (1, 2, 4), (1, 2, 4), (0, 3, 16)) if T.legal(*s)]


def test_io_patterns_and_proof_lengths_are_the_references_and_differ_between_statements():
    from provekit_amd import fracsum as fs, tuplelookup as tl

    assert len(STATEMENTS) == 5 * 3 * 3 * 3 * 3 - 3 * 3 * 3 * (2 + 1)  # n = 28 takes c = 1 alone, n = 27 c = 1 and 2
    pats = {}
    for n, k, w, c, n_bind in STATEMENTS:
        stmt = tl.Statement(n, k, w, c, n_bind)
        pat = pats[(n, k, w, c, n_bind)] = tl.io_pattern(stmt)
        assert pat == T.pattern(n, k, w, c, n_bind), (n, k, w, c, n_bind)
        assert (b"S1beta" in pat.split(b"\0")) == (w > 1)
        assert tl.proof_bytes(stmt) == T.proof_bytes(n, k, w, c) == fs.proof_bytes(fs.Statement(n + T.log2c(c), 1, 1)) + fs.proof_bytes(fs.Statement(k, 1, 0))
    assert len(set(pats.values())) == len(pats)
    assert pats[(8, 5, 1, 1, 0)].split(b"\0") == [tl.LABEL + b"/n8/k5/w1/c1", b"S1alpha", b"S2seeds"]
    assert pats[(8, 5, 2, 4, 3)].split(b"\0") == [tl.LABEL + b"/n8/k5/w2/c4", b"A3bind", b"S1alpha", b"S1beta", b"S2seeds"]


def test_arena_bytes_states_the_leaves_the_counts_and_the_two_fractional_sum_provers():
    from provekit_amd import fracsum as fs, tuplelookup as tl

    for n, k, w, c in ((1, 1, 1, 1), (12, 7, 3, 4), (5, 13, 4, 2)):
        inner = fs.arena_bytes(fs.Statement(n + T.log2c(c), 1, 1)) + fs.arena_bytes(fs.Statement(k, 1, 0))
        own = 32 * (c * 2**n + 2**k) + 4 * 2**k + 8
        assert inner + own <= tl.arena_bytes(tl.Statement(n, k, w, c)) <= inner + own + 256
    assert 1 <= tl.count_lds_max_k() <= 14  # u32 bins in the 64 KiB of LDS a kernel gets without asking


@pytest.mark.parametrize("stmt, reason", [
    ((0, 1), "n must be"), ((29, 1), "n must be"), ((4, 0), "k must be"), ((4, 29), "k must be"), ((4, 2, 0), "w must be"), ((4, 2, 5), "w must be"),
    ((4, 2, 1, 0), "c must be"), ((4, 2, 1, 3), "c must be"), ((4, 2, 1, 8), "c must be"), ((28, 2, 1, 2), r"n \+ log2 c must be"),
    ((27, 2, 1, 4), r"n \+ log2 c must be"), ((4, 2, 1, 1, 17), "n_bind must be"),
])
def test_every_refusal_is_made_with_a_reason(stmt, reason):
    from provekit_amd import tuplelookup as tl
    from provekit_amd._lib import ProveKitHipError

    s = tl.Statement(*stmt)
    for call in (tl.io_pattern, tl.proof_bytes, tl.arena_bytes):
        with pytest.raises(ProveKitHipError, match=reason) as e:
            call(s)
        assert e.value.code == -1
    st, r, which = s.struct(), tl.ResultStruct(), ctypes.c_int(0)  # the verifier refuses the statement before it looks at anything else
    assert tl.lib.pkt_verify(ctypes.addressof(st), None, 0, None, None, 0, None, None, None, ctypes.byref(r)) == -1
    assert re.search(reason, tl.lib.pkt_create_error().decode())
    cl, ev = tl.ClaimsStruct(), K.mont([0] * 16)
    assert tl.lib.pkt_check_claims(ctypes.addressof(st), ctypes.addressof(cl), ev.ctypes.data, ev.ctypes.data, ev.ctypes.data, ctypes.byref(which)) == -1
    assert re.search(reason, tl.lib.pkt_create_error().decode())


def test_verify_refuses_elements_that_do_not_match_the_statement():
    from provekit_amd import tuplelookup as tl
    from provekit_amd._lib import ProveKitHipError

    too_big = np.array([[2**64 - 1] * 4], dtype=np.uint64)
    st, r = tl.Statement(3, 2, 2, 1, 1).struct(), tl.ResultStruct()
    assert tl.lib.pkt_verify(ctypes.addressof(st), None, 0, None, None, 0, None, None, None, ctypes.byref(r)) == -1
    assert b"binds elements: pass" in tl.lib.pkt_create_error()  # NULL where elements are due
    with pytest.raises(ProveKitHipError, match="bind element 0 is not below p") as e:  # a non-canonical bind
        tl.verify(tl.Statement(3, 2, 2, 1, 1), b"", bind=too_big)
    assert e.value.code == -1


SIZES = [(1, 1, 1, 1), (3, 2, 2, 1), (3, 2, 4, 2), (4, 3, 3, 4), (2, 5, 2, 4)]


def _outside_row(t):
    have = set(T.rows(t))
    row = tuple((v + 1) % P for v in T.rows(t)[0])
    while row in have:
        row = tuple((v + 1) % P for v in row)
    return row


class Case:
    def __init__(self, n, k, w, c):
        self.n, self.k, self.w, self.c = n, k, w, c
        self.f, self.t, self.m, self.idx = T.random_case(n, k, w, c, seed=1000 * n + 100 * k + 10 * w + c)
        self.bind = K.random_elements(3, seed=9)
        self.ref = T.prove(n, k, self.f, self.t, self.m, self.bind)
        self.len_f = F.proof_bytes(n + T.log2c(c), 1)
        outside = [[list(col) for col in cols] for cols in self.f]
        for j, v in enumerate(_outside_row(self.t)):
            outside[c - 1][j][(1 << n) - 1] = v  # one row outside t
        self.outside = T.prove(n, k, outside, self.t, self.m, self.bind, validate=False)
        wrong_m = list(self.m)
        wrong_m[0] = (wrong_m[0] + 1) % P
        self.wrong_m = T.prove(n, k, self.f, self.t, wrong_m, self.bind, validate=False)

    def stmt(self):
        from provekit_amd import tuplelookup as tl

        return tl.Statement(self.n, self.k, self.w, self.c, 3)

    def both(self, proof, bind=None, pattern=None):
        """the library's verdict, after asserting that the reference names the same check, side, layer and (where it states one) offset"""
        from provekit_amd import tuplelookup as tl

        bind = self.bind if bind is None else bind
        check, side, layer, offset, seen = T.verify(self.n, self.k, self.w, self.c, proof, bind, pattern)
        res, lib_side, lib_layer, claims = tl.verify(self.stmt(), proof, K.mont(bind), pattern)
        assert (res.check, lib_side, lib_layer) == (check, side, layer) and res.accepted == (check == "NONE"), (res, lib_side, lib_layer, check, side, layer)
        assert offset is None or res.offset == offset, (res, offset)
        return res, lib_side, lib_layer, claims, seen


@pytest.fixture(scope="module")
def cases():
    return {size: Case(*size) for size in SIZES}


def _same_claims(claims, ref):
    for name in ("alpha", "beta", "f_value", "t_value", "m_value"):
        assert K.unmont(getattr(claims, name)) == [ref[name]], name
    assert K.unmont(claims.z_lo) == ref["z_lo"] and K.unmont(claims.z_t) == ref["z_t"] and K.unmont(claims.t_coeff) == ref["t_coeff"]
    assert [K.unmont(row) for row in claims.f_coeff] == ref["f_coeff"]


@pytest.mark.parametrize("size", SIZES)
def test_reference_proofs_are_accepted_with_the_references_claims_and_the_claims_hold(cases, size):
    from provekit_amd import tuplelookup as tl

    c = cases[size]
    ref = c.ref
    res, side, layer, claims, seen = c.both(ref["proof"])
    assert res.accepted and (side, layer) == ("F", 0) and res.offset == len(ref["proof"]) == T.proof_bytes(*size) and res.message == ""
    _same_claims(claims, ref)
    _same_claims(claims, seen)
    assert (K.unmont(claims.beta) == [1]) == (c.w == 1)
    # unused slots of the struct are zero
    raw = claims.struct
    assert all(v == 0 for g in range(4) for j in range(4) if g >= c.c or j >= c.w for v in raw.f_coeff[g][j])
    (pf, qf), (pt, qt) = ref["fractions"]
    assert (pf * qt - pt * qf) % P == 0
    # the three claims are the columns' extensions at the two points, combined: what the caller opens
    f_evals, t_evals, m_eval = T.evaluations(c.f, c.t, c.m, ref)
    assert T.check_claims(ref, f_evals, t_evals, m_eval) == "NONE"
    assert tl.check_claims(c.stmt(), claims, K.mont([v for evs in f_evals for v in evs]), K.mont(t_evals), K.mont([m_eval])) == "NONE"
    # the caller's own pattern bytes
    assert c.both(ref["proof"], pattern=T.pattern(*size, 3))[0].accepted


@pytest.mark.parametrize("size", SIZES)
def test_changing_any_one_evaluation_fails_the_claim_it_belongs_to(cases, size):
    from provekit_amd import tuplelookup as tl

    c = cases[size]
    _, _, _, claims, _ = c.both(c.ref["proof"])
    f_evals, t_evals, m_eval = T.evaluations(c.f, c.t, c.m, c.ref)
    flat = [v for evs in f_evals for v in evs]
    for i in range(len(flat)):
        changed = list(flat)
        changed[i] = (changed[i] + 1) % P
        want = T.check_claims(c.ref, [changed[g * c.w : (g + 1) * c.w] for g in range(c.c)], t_evals, m_eval)
        assert tl.check_claims(c.stmt(), claims, K.mont(changed), K.mont(t_evals), K.mont([m_eval])) == want == "F", i
    for j in range(c.w):
        changed = list(t_evals)
        changed[j] = (changed[j] + 1) % P
        assert tl.check_claims(c.stmt(), claims, K.mont(flat), K.mont(changed), K.mont([m_eval])) == T.check_claims(c.ref, f_evals, changed, m_eval) == "T", j
    assert tl.check_claims(c.stmt(), claims, K.mont(flat), K.mont(t_evals), K.mont([(m_eval + 1) % P])) == T.check_claims(c.ref, f_evals, t_evals, m_eval + 1) == "M"
    # the first failing claim is named
    assert tl.check_claims(c.stmt(), claims, K.mont([(v + 1) % P for v in flat]), K.mont(t_evals), K.mont([(m_eval + 1) % P])) == "F"
    from provekit_amd._lib import ProveKitHipError

    with pytest.raises(ProveKitHipError, match="m_eval element 0 is not below p"):
        tl.check_claims(c.stmt(), claims, K.mont(flat), K.mont(t_evals), np.array([[2**64 - 1] * 4], dtype=np.uint64))


def _bump(proof, element, delta=1):
    t = bytearray(proof)
    v = (int.from_bytes(t[32 * element : 32 * element + 32], "little") + delta) % P
    t[32 * element : 32 * element + 32] = v.to_bytes(32, "little")
    return bytes(t)


def _set(proof, element, value):
    t = bytearray(proof)
    t[32 * element : 32 * element + 32] = (value % P).to_bytes(32, "little")
    return bytes(t)


@pytest.mark.parametrize("size", SIZES)
def test_every_tampering_is_rejected_at_the_named_check_side_layer_and_offset(cases, size):
    c = cases[size]
    n, k, w, groups = size
    nf, len_f, ref = n + T.log2c(groups), c.len_f, c.ref
    proof = ref["proof"]
    # a row outside t, a wrong m: both fractional sums hold, the fractions differ
    for forged in (c.outside, c.wrong_m):
        (pf, qf), (pt, qt) = forged["fractions"]
        assert (pf * qt - pt * qf) % P != 0
        res, side, layer, _, _ = c.both(forged["proof"])
        assert (res.check, side, layer, res.offset) == ("FRACTION", "T", 0, len_f + 128)
    # swapped groups: the same multiset of rows, so the same fraction and an accepted proof -- of other columns: the claims differ
    if groups > 1 and c.f[0] != c.f[1]:
        swapped = T.prove(n, k, [c.f[1], c.f[0]] + c.f[2:], c.t, c.m, c.bind)
        res, _, _, claims, _ = c.both(swapped["proof"])
        assert res.accepted and swapped["fractions"][1] == ref["fractions"][1]
        f_evals, t_evals, m_eval = T.evaluations(c.f, c.t, c.m, swapped)  # the honest order's evaluations at the swapped proof's points
        assert T.check_claims(swapped, f_evals, t_evals, m_eval) == "F"
        from provekit_amd import tuplelookup as tl

        assert tl.check_claims(c.stmt(), claims, K.mont([v for evs in f_evals for v in evs]), K.mont(t_evals), K.mont([m_eval])) == "F"
    # each byte class of either side: a top value, s, a round value, a final
    for side_name, at, size_side, unit in (("F", 0, nf, 1), ("T", len_f // 32, k, 0)):
        for e in range(4):
            res, side, layer, _, _ = c.both(_bump(proof, at + e))
            if size_side > 1:
                assert (res.check, side, layer) == ("SUM", side_name, 1), (side_name, e, res)
            elif unit and e < 2:
                assert (res.check, side, layer, res.offset) == ("UNIT", "F", 0, 128)
            else:  # no layer: another fraction, which is not the other side's
                assert (res.check, side, layer, res.offset) == ("FRACTION", "T", 0, len_f + 128)
        for d in range(1, size_side):
            lay = at + F.layer_at(size_side, unit, d) // 32
            end = at + F.layer_at(size_side, unit, d + 1) // 32
            res, side, layer, _, _ = c.both(_bump(proof, lay))
            assert (res.check, side, layer, res.offset) == ("SUM", side_name, d, 32 * (lay + 1))
            res, side, layer, _, _ = c.both(_bump(proof, lay + 1))
            assert (res.check, side, layer, res.offset) == ("ROUND", side_name, d, 32 * (lay + 4))
            res, side, layer, _, _ = c.both(_bump(proof, end - 1))
            assert (res.check, side, layer, res.offset) == ("FINAL", side_name, d, 32 * end)
        res, side, layer, _, _ = c.both(_set(proof, at + 3, 0))
        assert (res.check, side, layer, res.offset) == ("DENOMINATOR", side_name, 0, 32 * at + 128)
        t = bytearray(proof)  # v + p: the same value mod p, not canonical on the wire
        v = int.from_bytes(t[32 * at : 32 * at + 32], "little") + P
        if v < 1 << 256:
            t[32 * at : 32 * at + 32] = v.to_bytes(32, "little")
            res, side, layer, _, _ = c.both(bytes(t))
            assert (res.check, side, layer, res.offset) == ("NON_CANONICAL", side_name, 0, 32 * at + 32)
    # a bind element enters nothing but the challenges: alpha, beta and the seeds change
    for e in range(3):
        changed = list(c.bind)
        changed[e] = (changed[e] + 1) % P
        res, side, layer, claims, _ = c.both(proof, bind=changed)
        if nf > 1:
            assert (res.check, side, layer) == ("SUM", "F", 1)
        elif k > 1:
            assert (res.check, side, layer) == ("SUM", "T", 1)
        else:  # no layer to fail: accepted PROVIDED other claims, which the columns do not meet
            assert res.accepted and K.unmont(claims.f_value) != [ref["f_value"]]
    # framing: both parts have a fixed length
    for cut in sorted({0, 31, 128, len_f - 1, len_f, len_f + 1, len(proof) - 1}):
        res, side, layer, _, _ = c.both(proof[:cut])
        assert (res.check, side, layer, res.offset) == ("TRANSCRIPT_SHORT", "F", 0, cut)
    for extra in (b"\0", bytes(32)):
        res, side, layer, _, _ = c.both(proof + extra)
        assert (res.check, side, layer, res.offset) == ("TRAILING_BYTES", "F", 0, len(proof))
    # another statement's pattern: other operations are IO_PATTERN; the same operations under another label are other challenges
    res, side, layer, _, _ = c.both(proof, pattern=T.pattern(n, k, w, groups, 1))
    assert (res.check, side, layer, res.offset) == ("IO_PATTERN", "F", 0, 0)
    res, side, layer, _, _ = c.both(proof, pattern=T.pattern(n, k, 1 if w > 1 else 2, groups, 3))
    assert (res.check, side, layer, res.offset) == ("IO_PATTERN", "F", 0, 0)
    res, _, _, _, _ = c.both(proof, pattern=T.pattern(n, k, w, groups, 3).replace(b"/v1/", b"/v2/"))
    assert res.check == ("SUM" if nf > 1 or k > 1 else "NONE")


def _blob(head, pat, bind, proofs):
    blob = struct.pack("<%dI" % len(head), *head) + struct.pack("<I", len(pat)) + pat + K.mont(bind).tobytes()
    return blob + struct.pack("<I", len(proofs)) + b"".join(struct.pack("<Q", len(p)) + p for p in proofs)


def test_hostile_framing_and_counts_under_the_sanitizers(cases, tmp_path):
    """the host verifier alone, with the two verifiers below it, built with -fsanitize=address,undefined as a program of its own (make -C
    provekit_amd/csrc asan): proofs cut at every kind of place and grown, from exact-size heap blocks; statements whose counts would
    size buffers if they were believed"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pkt_verify_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}

    def run(blob):
        f = tmp_path / "cases.bin"
        f.write_bytes(blob)
        p = subprocess.run([ASAN, "verify", str(f)], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        return p.stdout.splitlines()

    for size in ((4, 3, 3, 4), (3, 2, 2, 1)):
        c = cases[size]
        proof, boundary = c.ref["proof"], c.len_f
        rng = np.random.default_rng(1)
        hostile = {"honest": proof, "zero length": b"", "one byte": b"\1", "all ones": b"\xff" * len(proof), "extended": proof + bytes(64),
                   "random bytes": rng.integers(0, 256, size=len(proof), dtype=np.uint8).tobytes(),
                   "random layers": proof[:128] + rng.integers(0, 256, size=len(proof) - 128, dtype=np.uint8).tobytes(),
                   "random tail": proof[:boundary] + rng.integers(0, 256, size=len(proof) - boundary, dtype=np.uint8).tobytes(),
                   "halves swapped": proof[boundary:] + proof[:boundary], "a row outside the table": c.outside["proof"], "a wrong m": c.wrong_m["proof"]}
        for cut in (1, 31, 127, 129, boundary - 1, boundary, boundary + 1, len(proof) - 1):
            hostile[f"cut at {cut}"] = proof[:cut]
        for pat in (b"", T.pattern(*size, 3)):
            lines = run(_blob(list(size) + [3], pat, c.bind, list(hostile.values())))
            assert len(lines) == len(hostile)
            for (name, bad), line in zip(hostile.items(), lines):
                rc, accepted, check, side, layer, offset = line.split()[:6]
                want = T.verify(*size, bad, c.bind)
                assert (rc, check, accepted, side, layer) == ("0", want[0], "1" if want[0] == "NONE" else "0", str("FT".index(want[1])), str(want[2])), (name, line)
                assert int(offset) <= max(len(bad), len(proof))
    for bad in ([2**31, 1, 1, 1, 0], [5, 2**32 - 1, 1, 1, 0], [5, 2, 2**31, 1, 0], [5, 2, 1, 2**30, 0], [5, 2, 1, 1, 2**30], [28, 2, 1, 4, 0], [0, 0, 0, 0, 0]):
        # nothing after the statement: a count that was believed would read past the block
        lines = run(struct.pack("<5I", *bad))
        assert lines and lines[0].startswith("-1 0 REFUSED"), (bad, lines)
