"""CPU: libprovekit_sumcheck.so's host side.  The header/library/binding symbol match; pks_io_pattern against the reference's pattern
for every shape; every refusal with its reason; pks_verify on proofs the Python reference prover builds (tests/prodcheck_refs.py):
acceptance, and every tampering with the check both verifiers must name; the kernel's lane arithmetic compiled for the host at the
value bound, and for every (D, m) the round kernel dispatches with every coefficient kind (the statements of K.FORMS next to K.SHAPES;
the catalogue is held to round.hip's dispatch list); the one-round reference the device tests use; hostile framing through the sanitizer build of the host verifier (a program of its own, run as a subprocess)."""
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
HEADER = os.path.join(ROOT, "include", "provekit_sumcheck.h")
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pks_verify_asan")

import prodcheck_refs as K  # noqa: E402

P = K.P
SIZES = {"inner": 5, "r1cs": 6, "eval": 4, "triple": 5, "mixed": 5, "four": 6,  # a few variables each: the verifier's work is per round
         "lin2": 4, "lin3": 5, "lin4": 6, "lin2rep": 4, "deg3low": 6, "pair2": 5}
ROUND_HIP = os.path.join(ROOT, "provekit_amd", "csrc", "sumcheck", "round.hip")
EVERY_SHAPE = list(K.SHAPES) + list(K.FORMS)


def test_the_catalogue_reaches_every_instantiation_the_round_kernel_dispatches():
    """the (D, m) pairs of the twelve statements against the PKS_CASE uses of round.hip's launch(): an instantiation added there has no
    statement that launches it until one is added here"""
    dispatched = {(int(d), int(m)) for d, m in re.findall(r"PKS_CASE\((\d+),\s*(\d+)\)", open(ROUND_HIP).read())}
    reached = {(s.D, s.m) for s in (K.Shape(name, 1) for name in EVERY_SHAPE)}
    nine = {(1, 1), (1, 2), (1, 3), (1, 4), (2, 2), (2, 3), (2, 4), (3, 3), (3, 4)}
    assert dispatched == nine and reached == nine, (sorted(dispatched), sorted(reached))
    assert not set(K.SHAPES) & set(K.FORMS) and len(EVERY_SHAPE) == 12


def test_the_header_declares_what_the_library_exports_and_the_binding_binds():
    from provekit_amd import prodcheck, verify

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pks_[a-z0-9_]+)\s*\(", src)))
    nm = subprocess.run(["nm", "-D", "--defined-only", prodcheck.SUMCHECK_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" [A-Za-z] (pks_[a-z0-9_]+)$", nm, flags=re.M)))
    assert declared == exported == sorted(prodcheck.SIGNATURES) and len(exported) == 11
    assert ctypes.CDLL(prodcheck.SUMCHECK_LIB_PATH).pks_abi_version() == 1
    assert [prodcheck.lib.pks_check_name(i).decode() for i in range(len(prodcheck.CHECKS))] == list(prodcheck.CHECKS)
    assert prodcheck.CHECKS[: len(verify.CHECKS)] == verify.CHECKS and prodcheck.CHECKS[-3:] == ("ROUND", "FINAL", "SUM")
    # the library calls the product only through its C ABI, and neither of the other libraries above it
    und = subprocess.run(["nm", "-D", "--undefined-only", prodcheck.SUMCHECK_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\b_ZN2pk\w+", und) and not re.findall(r"\bpk[vw]_\w+", und), und
    assert set(re.findall(r"\bpk_\w+", und)) <= set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "provekit_hip.h")).read()))


def test_io_pattern_is_the_references_for_every_shape_and_differs_between_shapes():
    from provekit_amd import prodcheck

    pats = {}
    for name in K.SHAPES:
        for n, n_bind in ((1, 0), (SIZES[name], 0), (SIZES[name], 2), (28, 16)):
            shape = K.Shape(name, n, n_bind)
            pat = prodcheck.io_pattern(shape.statement())
            assert pat == shape.pattern(), (name, n, n_bind)
            assert prodcheck.proof_bytes(shape.statement()) == shape.proof_bytes()
            pats[(name, n, n_bind)] = pat
    assert len(set(pats.values())) == len(pats)
    head = pats[("r1cs", 6, 2)].split(b"\0")
    assert head[0] == prodcheck.LABEL + b"/n6/m3/T2/tau1/masks3.4"
    assert head[1:6] == [b"A2bind", b"A6tau", b"A2coefficients", b"A1sum", b"A3round_values"] and head[-1] == b"A3final_values"
    # the same operations under another term structure: the label alone tells them apart
    a = prodcheck.Statement(5, 3, [(1, 0b011), (1, 0b100)])
    b = prodcheck.Statement(5, 3, [(1, 0b101), (1, 0b010)])
    pa, pb = prodcheck.io_pattern(a), prodcheck.io_pattern(b)
    assert pa != pb and pa.split(b"\0")[1:] == pb.split(b"\0")[1:]


def test_io_pattern_is_the_references_for_the_forms_too_and_differs_between_all_twelve():
    """a mask in two terms is spelled twice (lin2rep: masks1.2.1.2); a zero coefficient is a coefficient"""
    from provekit_amd import prodcheck

    pats = {}
    for name in EVERY_SHAPE:
        for n, n_bind in ((1, 0), (SIZES[name], 0), (SIZES[name], 2), (28, 16)):
            shape = K.Shape(name, n, n_bind)
            pat = prodcheck.io_pattern(shape.statement())
            assert pat == shape.pattern(), (name, n, n_bind)
            assert prodcheck.proof_bytes(shape.statement()) == shape.proof_bytes()
            pats[(name, n, n_bind)] = pat
    assert len(set(pats.values())) == len(pats)
    assert pats[("lin2rep", 4, 0)].split(b"\0")[:3] == [prodcheck.LABEL + b"/n4/m2/T4/tau0/masks1.2.1.2", b"A4coefficients", b"A1sum"]
    assert pats[("lin4", 6, 2)].split(b"\0")[1:6] == [b"A2bind", b"A6tau", b"A4coefficients", b"A1sum", b"A2round_values"]


@pytest.mark.parametrize("stmt, reason", [
    ((0, 2, [(1, 3)]), "n must be"), ((29, 2, [(1, 3)]), "n must be"),
    ((4, 0, [(1, 1)]), "m must be"), ((4, 5, [(1, 3)]), "m must be"),
    ((4, 2, []), "T must be"), ((4, 2, [(1, 3)] * 5), "T must be"),
    ((4, 2, [(1, 3)], False, 17), "n_bind must be"),
    ((4, 2, [(1, 3), (1, 0)]), "empty mask"),
    ((4, 2, [(1, 0b111)]), "names a table >= m"),
    ((4, 3, [(1, 0b011)]), "used by no term"),
    ((4, 4, [(1, 0b1111)]), "more than 3 tables"),
    ((4, 2, [([(P >> (64 * i)) & (2**64 - 1) for i in range(4)], 3)]), "not below p"),
    ((4, 2, [([2**64 - 1] * 4, 3)]), "not below p"),
])
def test_every_refusal_is_made_with_a_reason(stmt, reason):
    from provekit_amd import prodcheck
    from provekit_amd._lib import ProveKitHipError

    s = prodcheck.Statement(*stmt)
    for call in (prodcheck.io_pattern, prodcheck.proof_bytes):
        with pytest.raises(ProveKitHipError, match=reason) as e:
            call(s)
        assert e.value.code == -1
    st, r = s.struct(), prodcheck.ResultStruct()  # the verifier refuses the statement before it looks at anything else
    assert prodcheck.lib.pks_verify(ctypes.addressof(st), None, 0, None, None, None, None, 0, None, None, ctypes.byref(r)) == -1
    assert re.search(reason, prodcheck.lib.pks_create_error().decode())


def test_verify_refuses_a_tau_or_bind_that_does_not_match_the_statement():
    from provekit_amd import prodcheck
    from provekit_amd._lib import ProveKitHipError

    s = prodcheck.Statement(3, 1, [(1, 1)], has_tau=True, n_bind=1)
    st, r = s.struct(), prodcheck.ResultStruct()
    one = K.mont([1, 1, 1])
    for tau, bind, reason in ((None, one.ctypes.data, b"has a tau"), (one.ctypes.data, None, b"binds elements")):
        assert prodcheck.lib.pks_verify(ctypes.addressof(st), None, 0, tau, bind, None, None, 0, None, None, ctypes.byref(r)) == -1
        assert reason in prodcheck.lib.pks_create_error()
    too_big = np.array([[2**64 - 1] * 4] * 3, dtype=np.uint64)
    with pytest.raises(ProveKitHipError, match="not below p"):
        prodcheck.verify(s, b"", tau=too_big, bind=one[:1])


class Case:
    def __init__(self, name):
        self.shape = K.Shape(name, SIZES[name], n_bind=2)
        self.stmt = self.shape.statement()
        self.tables = K.random_tables(self.shape.m, self.shape.n, seed=len(name))
        self.tau = K.random_elements(self.shape.n, seed=7) if self.shape.has_tau else None
        self.bind = K.random_elements(2, seed=9)
        self.proof, self.point, self.finals, self.s = K.prove(self.shape, self.tables, self.tau, self.bind)

    def both(self, proof=None, tau="own", bind=None, expected_sum=None, pattern=None):
        """the library's verdict, after asserting that the reference's is the same check"""
        from provekit_amd import prodcheck

        proof = self.proof if proof is None else proof
        tau = self.tau if tau == "own" else tau
        bind = self.bind if bind is None else bind
        ref, _, _ = K.verify(self.shape, proof, tau, bind, expected_sum, pattern)
        res, point, finals = prodcheck.verify(self.stmt, proof, K.mont(tau) if tau is not None else None, K.mont(bind),
                                              K.mont([expected_sum]) if expected_sum is not None else None, pattern)
        assert res.check == ref and res.accepted == (ref == "NONE"), (res, ref)
        return res, point, finals


@pytest.fixture(scope="module")
def cases():
    return {name: Case(name) for name in K.SHAPES}


@pytest.mark.parametrize("name", list(K.SHAPES))
def test_reference_proofs_are_accepted_with_the_references_point_and_finals(cases, name):
    c = cases[name]
    assert len(c.proof) == c.shape.proof_bytes() and int.from_bytes(c.proof[:32], "little") == c.s
    # the reference proves what it says: s is the sum, the finals are the tables' extensions at the point
    w = K.pr.eq_table(c.tau) if c.tau is not None else [1] * (1 << c.shape.n)
    assert c.s == sum(w[x] * c.shape.terms_at([t[x] for t in c.tables]) for x in range(1 << c.shape.n)) % P
    eq_r = K.pr.eq_table(c.point)
    assert c.finals == [sum(e * v for e, v in zip(eq_r, t)) % P for t in c.tables]
    for kw in ({}, {"pattern": c.shape.pattern()}, {"expected_sum": c.s}):
        res, point, finals = c.both(**kw)
        assert res.accepted and res.check == "NONE" and res.offset == len(c.proof) and res.message == ""
        assert K.unmont(point) == c.point and K.unmont(finals) == c.finals


def _bump(proof, element, delta=1):
    t = bytearray(proof)
    v = (int.from_bytes(t[32 * element : 32 * element + 32], "little") + delta) % P
    t[32 * element : 32 * element + 32] = v.to_bytes(32, "little")
    return bytes(t)


@pytest.mark.parametrize("name", list(K.SHAPES))
def test_every_tampering_is_rejected_at_the_named_check(cases, name):
    every_tampering(cases[name], name)


def every_tampering(c, name, cancelled=()):
    """cancelled: the tables whose value the statement's terms do not depend on (none in SHAPES): a changed final value of such a table
    is no tampering with the claim, and both verifiers must accept it"""
    n, D, m = c.shape.n, c.shape.D, c.shape.m
    for i in range(n):  # one changed value in each round: h_i(0) enters round i's own check
        res, _, _ = c.both(_bump(c.proof, 1 + i * (D + 1)))
        assert res.check == "ROUND" and f"round {i}:" in res.message and res.offset == 32 * (1 + (i + 1) * (D + 1))
    # ... and h_i(D) only the next claim: the round after it fails, or the final check after the last round
    if D > 1:  # (at D = 1 every value enters its own round's check)
        res, _, _ = c.both(_bump(c.proof, 1 + D))
        assert res.check == "ROUND" and "round 1:" in res.message
        assert c.both(_bump(c.proof, 1 + (n - 1) * (D + 1) + D))[0].check == "FINAL"
    for j in range(m):
        assert c.both(_bump(c.proof, 1 + n * (D + 1) + j))[0].check == ("NONE" if j in cancelled else "FINAL")
    # a changed s: against the expected sum, and without one against round 0
    assert c.both(expected_sum=(c.s + 1) % P)[0].check == "SUM"
    res, _, _ = c.both(_bump(c.proof, 0))
    assert res.check == "ROUND" and "round 0:" in res.message
    assert c.both(_bump(c.proof, 0), expected_sum=c.s)[0].check == "SUM"
    if c.tau is not None:  # a changed tau_0 changes round 0's weights; a later coordinate only the challenges and a later round's
        for i in (0, n - 1):
            tau = list(c.tau)
            tau[i] = (tau[i] + 1) % P
            assert c.both(tau=tau)[0].check == "ROUND"
    for k in range(2):  # bind elements enter nothing but the challenges
        bind = list(c.bind)
        bind[k] = (bind[k] + 1) % P
        res, _, _ = c.both(bind=bind)
        assert res.check == "ROUND" and "round 1:" in res.message
    for cut in (0, 31, 32, 32 * (2 + D), len(c.proof) - 1):
        assert c.both(c.proof[:cut])[0].check == "TRANSCRIPT_SHORT"
    res, _, _ = c.both(c.proof + b"\0")
    assert res.check == "TRAILING_BYTES" and res.offset == len(c.proof)
    for element in (0, 2, 1 + n * (D + 1)):  # v + p: the same value mod p, not canonical on the wire
        t = bytearray(c.proof)
        v = int.from_bytes(t[32 * element : 32 * element + 32], "little") + P
        if v < 1 << 256:
            t[32 * element : 32 * element + 32] = v.to_bytes(32, "little")
            res, _, _ = c.both(bytes(t))
            assert res.check == "NON_CANONICAL" and res.offset == 32 * (element + 1)
    # another statement's pattern: other operations are IO_PATTERN, the same operations under another label other challenges
    other = K.Shape("eval" if name != "eval" else "inner", c.shape.n, 2)
    assert c.both(pattern=other.pattern())[0].check == "IO_PATTERN"
    assert c.both(pattern=K.Shape(name, c.shape.n + 1, 2).pattern())[0].check in ("IO_PATTERN", "ROUND")
    relabelled = c.shape.pattern().replace(b"/v1/", b"/v2/")
    assert c.both(pattern=relabelled)[0].check == "ROUND"


@pytest.fixture(scope="module")
def form_cases():
    return {name: Case(name) for name in K.FORMS}


@pytest.mark.parametrize("name", list(K.FORMS))
def test_reference_proofs_of_the_forms_are_accepted_with_the_references_point_and_finals(form_cases, name):
    test_reference_proofs_are_accepted_with_the_references_point_and_finals(form_cases, name)


@pytest.mark.parametrize("name", list(K.FORMS))
def test_every_tampering_of_the_forms_is_rejected_at_the_named_check(form_cases, name):
    """lin2rep is f0 + 0 f1 - f0 + 9 f1 = 9 f1: f0's final value enters no check, whatever it is"""
    c = form_cases[name]
    cancelled = (0,) if name == "lin2rep" else ()
    for j in range(c.shape.m):  # ... which is the statement's property, not an allowance: its terms at the changed finals say so
        changed = [(v + 1) % P if k == j else v for k, v in enumerate(c.finals)]
        assert (c.shape.terms_at(changed) == c.shape.terms_at(c.finals)) == (j in cancelled)
    every_tampering(c, name, cancelled)


def _round_of(proof, D, i):
    at = 32 * (1 + i * (D + 1))
    return [int.from_bytes(proof[at + 32 * k : at + 32 * k + 32], "little") for k in range(D + 1)]


@pytest.mark.parametrize("name", EVERY_SHAPE)
def test_round_values_are_the_reference_provers_rounds_0_and_1(name):
    """K.round_values -- the one-round reference the device tests of pks_round compare with -- against the round values inside
    K.prove's bytes at n = 5: round 0 on the tables as they stand, round 1 after the fold by point[0], which also gives the folded tables"""
    n = 5
    shape = K.Shape(name, n)
    tables = K.random_tables(shape.m, n, seed=40 + len(name))
    tau = K.random_elements(n, seed=41) if shape.has_tau else None
    proof, point, finals, _ = K.prove(shape, tables, tau)
    assert K.round_values(shape, tables, tau[1:] if tau else None) == _round_of(proof, shape.D, 0)
    h, folded = K.round_values(shape, tables, tau[2:] if tau else None, fold=point[0])
    assert h == _round_of(proof, shape.D, 1)
    half = 1 << (n - 1)
    assert folded == [[(t[x] + point[0] * (t[x + half] - t[x])) % P for x in range(half)] for t in tables]
    # ... and those are the tables the rest of the proof is about: bound by the other challenges they give the final values
    eq_rest = K.pr.eq_table(point[1:])
    assert finals == [sum(e * v for e, v in zip(eq_rest, t)) % P for t in folded]
    # tau_rest None is weight 1 whatever the shape says: h(0) is then the plain sum of the terms over the lower half
    assert K.round_values(shape, tables, None)[0] == sum(shape.terms_at([t[x] for t in tables]) for x in range(half)) % P


def _hex(v):
    return "%064x" % v


@pytest.mark.parametrize("name", EVERY_SHAPE)
def test_the_lane_arithmetic_on_the_host_for_every_instantiation_and_coefficient_kind(name):
    """lane_accumulate<D, m> of every (D, m) the kernel is instantiated for (pks_verify_asan lanes), on each statement's own masks and
    coefficients -- their kinds taken by lane.hpp's coeff_kind, as round.hip's launch() takes them -- weighted and not, against Python
    ints: per-table random values, and the value bound with a stepped value that wraps (every lo = p - 1 and every hi = 0, and the reverse)"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pks_verify_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    shape = K.Shape(name, 1)
    m, D, R, R_INV = shape.m, shape.D, K.R, K.R_INV
    rnd = K.random_elements(2 * m + 1, seed=50 + len(name))
    # raw 256-bit values as the lane holds them (Montgomery images): (lo per table, hi per table, weight)
    values = [(rnd[:m], rnd[m : 2 * m], rnd[2 * m]), ([P - 1] * m, [0] * m, P - 1), ([0] * m, [P - 1] * m, P - 1)]
    terms = [a for c, mask in shape.terms for a in (str(mask), _hex(c * R % P))]
    for lo, hi, w in values:
        for weighted in (True, False):
            for repeats in (1, 3):
                pairs = [_hex(v) for lh in zip(lo, hi) for v in lh]
                p = subprocess.run([ASAN, "lanes", str(D), str(m), str(len(shape.terms)), str(int(weighted)), _hex(w), str(repeats)] + terms + pairs,
                                   capture_output=True, text=True, env=env, timeout=120)
                assert p.returncode == 0, p.stderr[-3000:]
                got = [int(line, 16) for line in p.stdout.split()]
                # an image x stands for x R^-1; the sums come back as images
                weight = w * R_INV % P if weighted else 1
                want = [repeats * weight * shape.terms_at([(a + X * (b - a)) * R_INV % P for a, b in zip(lo, hi)]) * R % P for X in range(D + 1)]
                assert got == want, (name, lo[0], hi[0], weighted, repeats)


@pytest.mark.parametrize("D", [1, 2, 3])
def test_the_lane_arithmetic_on_the_host_at_the_value_bound(D):
    """lane.hpp -- the kernel's stepping, products, coefficient, weight and running sums -- compiled for the host (pks_verify_asan lane):
    every table entry p - 1, coefficient p - 1, weight p - 1; then entries that make the stepped value wrap (p - 1 -> 0 and 0 -> p - 1)"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pks_verify_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    R_INV = K.R_INV
    for lo, hi in ((P - 1, P - 1), (P - 1, 0), (0, P - 1), (P - 2, 5)):
        for repeats in (1, 3):
            c = w = P - 1
            p = subprocess.run([ASAN, "lane", str(D), _hex(lo), _hex(hi), _hex(c), _hex(w), str(repeats)], capture_output=True, text=True, env=env, timeout=120)
            assert p.returncode == 0, p.stderr[-3000:]
            got = [int(line, 16) for line in p.stdout.split()]
            # Montgomery images: a product of k images carries R^-(k-1); D factors, the coefficient and the weight
            want = [repeats * pow(lo + X * (hi - lo), D, P) * c * w * pow(R_INV, D + 1, P) % P for X in range(D + 1)]
            assert got == want, (D, lo, hi, repeats)


def test_hostile_framing_and_counts_under_the_sanitizers(cases, tmp_path):
    """the host verifier alone, built with -fsanitize=address,undefined as a program of its own (make -C provekit_amd/csrc asan): proofs cut
    at every kind of place and grown, from exact-size heap blocks; statements whose counts would size buffers if they were believed"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pks_verify_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    c = cases["four"]
    sh = c.shape

    def blob(head, coeffs, rest=b""):
        return struct.pack("<9I", *head) + b"".join(K.mont([v]).tobytes() for v in coeffs) + rest

    head = [sh.n, sh.m, len(sh.terms), 1, 2] + [mask for _, mask in sh.terms]
    coeffs = [v for v, _ in sh.terms]
    hostile = {"honest": c.proof, "zero length": b"", "one byte": b"\1", "random bytes": np.random.default_rng(1).integers(0, 256, size=len(c.proof), dtype=np.uint8).tobytes(),
               "all ones": b"\xff" * len(c.proof), "extended": c.proof + bytes(64)}
    for cut in (1, 31, 33, 32 * (1 + sh.D), len(c.proof) - 32 * sh.m, len(c.proof) - 1):
        hostile[f"cut at {cut}"] = c.proof[:cut]
    for pattern in (b"", sh.pattern()):
        rest = struct.pack("<II", 1, len(pattern)) + pattern + K.mont(c.tau).tobytes() + K.mont(c.bind).tobytes() + K.mont([c.s]).tobytes()
        rest += struct.pack("<I", len(hostile)) + b"".join(struct.pack("<Q", len(p)) + p for p in hostile.values())
        f = tmp_path / "cases.bin"
        f.write_bytes(blob(head, coeffs, rest))
        p = subprocess.run([ASAN, "verify", str(f)], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = p.stdout.splitlines()
        assert len(lines) == len(hostile)
        for (name, proof), line in zip(hostile.items(), lines):
            rc, accepted, check, offset = line.split()[:4]
            want = K.verify(sh, proof, c.tau, c.bind, c.s)[0]
            assert (rc, check, accepted) == ("0", want, "1" if want == "NONE" else "0"), (name, line)
            assert int(offset) <= len(proof)
    for bad in ([2**31, 3, 2, 1, 2, 3, 4, 0, 0], [6, 2**32 - 1, 2, 1, 2, 3, 4, 0, 0], [6, 3, 2**30, 1, 2, 3, 4, 0, 0], [6, 3, 2, 7, 2, 3, 4, 0, 0],
                [6, 3, 2, 1, 2**32 - 1, 3, 4, 0, 0], [6, 3, 2, 1, 2, 2**32 - 1, 4, 0, 0], [6, 3, 2, 1, 2, 0, 7, 0, 0]):
        f = tmp_path / "refused.bin"
        f.write_bytes(blob(bad, [1, 1, 1, 1]))  # nothing after the statement: a count that was believed would read past the block
        p = subprocess.run([ASAN, "verify", str(f)], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0 and p.stdout.startswith("-1 0 REFUSED"), (bad, p.stdout, p.stderr[-2000:])
