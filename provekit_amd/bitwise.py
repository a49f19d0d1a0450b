"""AND / XOR / OR of device columns by digit lookups (libprovekit_bitwise.so, include/provekit_bitwise.h): prove that column c is
a op b, entry by entry, on words of L digits of d bits (up to 48 bits), by looking every digit row (a_i, b_i, c_i) up in the operation's
table of 2^(2d) rows with one tuple-lookup proof, and tying the digits back to the columns by three recomposition claims.
`Prover.decompose` is the fused device pass: c, the 3 L digit columns and the multiplicities from a and b.

An accepted proof is accepted PROVIDED the five claims of `Claims`: whir_pcs.Scheme.open / whir_pcs.verify give the evaluations of a, b,
c and the digit columns at z_lo and m's at z_t, `check_claims` forms the combinations.

A thirteenth library above the product's C ABI, with its own loader and one signature table (as provekit_amd.rangecheck).  `plan`,
`verify`, `check_claims`, the pattern and the lengths are host only; the prover needs a Context.  A rejected proof is a Result, not an
exception; only a failed CALL raises.  There is no fallback: without the built library the import raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import tuplelookup  # loads libprovekit_tuplelookup.so (and the libraries under it), which this library links
from ._lib import ProveKitHipError, sz, vp
from .prodcheck import _fe, _ptr
from .runtime import Context, DeviceBuffer
from .verify import Result, ResultStruct

BITWISE_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libprovekit_bitwise.so")
MAX_VARS, MAX_BIND, MAX_DIGIT_BITS, MAX_DIGITS, MAX_GRID = 28, 16, 12, 4, 1024
AND, XOR, OR = 0, 1, 2
OPS = ("and", "xor", "or")
CHECKS = tuplelookup.CHECKS + ("TABLE",)
SIDES = tuplelookup.SIDES
WHICH = ("NONE", "DIGITS", "RECOMPOSE_A", "RECOMPOSE_B", "RECOMPOSE_C", "M")  # check_claims
LABEL = b"provekit-hip/bitwise/v1"
ERR_BAD_ARG, ERR_UNSATISFIED = -1, -6
NO_BAD_ENTRY = 2**64 - 1


class StatementStruct(C.Structure):
    """pkb_statement"""

    _fields_ = [("n", C.c_uint), ("op", C.c_uint), ("d", C.c_uint), ("L", C.c_uint), ("n_bind", C.c_uint)]


class PlanStruct(C.Structure):
    """pkb_digit_plan"""

    _fields_ = [("bits", C.c_uint), ("k", C.c_uint), ("c_groups", C.c_uint), ("digit_of", C.c_uint * MAX_DIGITS)]


class ClaimsStruct(C.Structure):
    """pkb_claims"""

    _fields_ = [("z_lo", (C.c_uint64 * 4) * MAX_VARS), ("z_t", (C.c_uint64 * 4) * MAX_VARS), ("digit_coeff", ((C.c_uint64 * 4) * MAX_DIGITS) * 3),
                ("digits_value", C.c_uint64 * 4), ("pow2", (C.c_uint64 * 4) * MAX_DIGITS), ("m_value", C.c_uint64 * 4)]


# name -> (restype, argtypes); kept in the same order as include/provekit_bitwise.h
SIGNATURES = {
    "pkb_abi_version": (C.c_int, []),
    "pkb_check_name": (C.c_char_p, [C.c_int]),
    "pkb_create_error": (C.c_char_p, []),
    "pkb_plan": (C.c_int, [vp, vp]),
    "pkb_io_pattern": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
    "pkb_proof_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkb_prover_arena_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkb_count_lds_max_d": (C.c_uint, []),
    "pkb_prover_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pkb_prover_destroy": (C.c_int, [vp]),
    "pkb_last_error": (C.c_char_p, [vp]),
    "pkb_decompose": (C.c_int, [vp, vp, vp, vp, C.c_int, vp, vp, C.POINTER(C.c_uint64)]),
    "pkb_prove": (C.c_int, [vp, vp, vp, vp, vp, sz, C.POINTER(sz), vp]),
    "pkb_verify": (C.c_int, [vp, vp, sz, vp, vp, sz, vp, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(ResultStruct)]),
    "pkb_check_claims": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(C.c_int)]),
}


def _load():
    if not os.path.exists(BITWISE_LIB_PATH):
        raise ImportError(
            f"{BITWISE_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C provekit_amd/csrc`). provekit_amd has no CPU fallback."
        )
    return C.CDLL(BITWISE_LIB_PATH)  # the libraries it links are the ones already loaded (same files, next to it)


lib = _load()
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


class Statement:
    """columns a, b, c of 2^n entries with c = a op b on words of L digits of d bits; n_bind caller elements (the roots) are absorbed
    first"""

    def __init__(self, n: int, op: int, d: int, L: int, n_bind: int = 0):
        self.n, self.op, self.d, self.L, self.n_bind = n, op, d, L, n_bind

    def struct(self) -> StatementStruct:
        return StatementStruct(self.n, self.op, self.d, self.L, self.n_bind)


class Plan:
    """pkb_plan's answer: bits = L d, k = 2 d, the lookup's c groups, and per group g < c the digit it looks up"""

    def __init__(self, p: PlanStruct):
        self.bits, self.k, self.c = p.bits, p.k, p.c_groups
        self.digit_of = list(p.digit_of)[: p.c_groups]


class Claims:
    """what an accepted proof is accepted PROVIDED of, Montgomery [.., 4] uint64: the points z_lo [n, 4] and z_t [2 d, 4], digit_coeff
    [3, L, 4] with digits_value [4], pow2 [L, 4] = 2^(d i), m_value [4]"""

    def __init__(self, stmt: Statement, c: ClaimsStruct):
        self.struct = c
        a = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731
        self.z_lo = a([list(c.z_lo[i]) for i in range(stmt.n)])
        self.z_t = a([list(c.z_t[i]) for i in range(2 * stmt.d)])
        self.digit_coeff = a([[list(c.digit_coeff[j][i]) for i in range(stmt.L)] for j in range(3)])
        self.pow2 = a([list(c.pow2[i]) for i in range(stmt.L)])
        self.digits_value, self.m_value = a(c.digits_value), a(c.m_value)


def _refused(rc: int):
    raise ProveKitHipError(rc, lib.pkb_create_error().decode())


def _sized(call, stmt) -> int:
    s = stmt.struct()
    n = sz()
    rc = call(C.addressof(s), C.byref(n))
    if rc:
        _refused(rc)
    return n.value


def plan(stmt: Statement) -> Plan:
    """the digits and groups of a statement; a statement the library does not take raises with the reason (pkb_plan; host only)"""
    s, p = stmt.struct(), PlanStruct()
    rc = lib.pkb_plan(C.addressof(s), C.addressof(p))
    if rc:
        _refused(rc)
    return Plan(p)


def io_pattern(stmt: Statement) -> bytes:
    """the spongefish operation list (domain separator) of the outer transcript (host only)"""
    s = stmt.struct()
    n = sz()
    rc = lib.pkb_io_pattern(C.addressof(s), None, 0, C.byref(n))
    if rc:
        _refused(rc)
    buf = (C.c_uint8 * n.value)()
    lib.pkb_io_pattern(C.addressof(s), buf, n.value, C.byref(n))
    return bytes(buf)


def proof_bytes(stmt: Statement) -> int:
    return _sized(lib.pkb_proof_bytes, stmt)


def arena_bytes(stmt: Statement) -> int:
    """the device memory a prover of this statement holds, its lookup prover included (host only)"""
    return _sized(lib.pkb_prover_arena_bytes, stmt)


def count_lds_max_d() -> int:
    """digits of up to this many bits are counted in a workgroup's LDS histogram"""
    return int(lib.pkb_count_lds_max_d())


def _result(r: ResultStruct) -> Result:
    return Result(bool(r.accepted), CHECKS[r.check] if 0 <= r.check < len(CHECKS) else str(r.check), int(r.offset), r.message.decode(errors="replace"))


def _bytes_arg(b):
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


def verify(stmt: Statement, proof: bytes, bind=None, io_pattern: bytes | None = None):
    """(Result, side, layer, Claims or None): side is "F" or "T", the lookup's (pkb_verify; host only)"""
    s = stmt.struct()
    bind_a = _fe(bind, stmt.n_bind, "bind") if (bind is not None or stmt.n_bind) else None
    claims, r, side, layer = ClaimsStruct(), ResultStruct(), C.c_int(0), C.c_uint(0)
    pat = _bytes_arg(io_pattern) if io_pattern else None
    pbuf = _bytes_arg(proof)
    rc = lib.pkb_verify(C.addressof(s), C.cast(pat, vp) if pat is not None else None, len(io_pattern) if io_pattern else 0, _ptr(bind_a), C.cast(pbuf, vp), len(proof),
                        C.addressof(claims), C.byref(side), C.byref(layer), C.byref(r))
    if rc:
        _refused(rc)
    res = _result(r)
    return res, SIDES[side.value], layer.value, Claims(stmt, claims) if res.accepted else None


def check_claims(stmt: Statement, claims: Claims, abc_evals, digit_evals, m_eval) -> str:
    """abc_evals [3, 4] = a, b, c at z_lo, digit_evals [3 L, 4] = digit_{j,i}(z_lo) at [j L + i], m_eval [4] = m(z_t), Montgomery ->
    "NONE" when the five claims hold, else the first that does not, in WHICH's order (pkb_check_claims; host only)"""
    s = stmt.struct()
    abc = _fe(np.asarray(abc_evals, dtype=np.uint64).reshape(-1, 4), 3, "abc_evals")
    dig = _fe(np.asarray(digit_evals, dtype=np.uint64).reshape(-1, 4), 3 * max(stmt.L, 1), "digit_evals")
    m_a = _fe(np.asarray(m_eval, dtype=np.uint64).reshape(-1, 4), 1, "m_eval")
    which = C.c_int(-1)
    rc = lib.pkb_check_claims(C.addressof(s), C.addressof(claims.struct), _ptr(abc), _ptr(dig), _ptr(m_a), C.byref(which))
    if rc:
        _refused(rc)
    return WHICH[which.value]


def _dev(buf):
    return None if buf is None else buf.ptr if isinstance(buf, DeviceBuffer) else int(buf)


class Prover:
    """one statement's prover on a context: owns the operation's table, the counts and the lookup prover, made at creation; a proof
    allocates no device memory and never writes the caller's tables"""

    fill = None  # a byte the proof buffer (`buffer`) is filled with before a proof, to see afterwards what a refused call wrote: nothing

    def __init__(self, ctx: Context, stmt: Statement):
        self.ctx, self.stmt = ctx, stmt
        s = stmt.struct()
        h = vp()
        rc = lib.pkb_prover_create(ctx.handle, C.addressof(s), C.byref(h))
        if rc:
            _refused(rc)
        self.handle = h
        self.proof_bytes = proof_bytes(stmt)
        self.plan = plan(stmt)
        self.first_bad = NO_BAD_ENTRY

    def close(self):
        if getattr(self, "handle", None):
            lib.pkb_prover_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return lib.pkb_last_error(self.handle).decode()

    def _check(self, rc: int):
        if rc:
            raise ProveKitHipError(rc, self.last_error())

    def _digits(self, d_digits):
        """three lists (a's, b's, c's) of L columns each, or one flat list of 3 L, [j L + i]"""
        flat = [b for part in d_digits for b in part] if len(d_digits) == 3 and isinstance(d_digits[0], (list, tuple)) else list(d_digits)
        if len(flat) != 3 * self.stmt.L:
            raise ValueError(f"{3 * self.stmt.L} digit columns expected, {len(flat)} given")
        return (vp * len(flat))(*[_dev(b) for b in flat])

    def decompose(self, d_a, d_b, d_c, d_digits, d_m, c_given: bool = False) -> None:
        """d_a, d_b: 2^n elements -> d_c = a op b (c_given: d_c is read and compared instead), the 3 L digit columns d_digits (2^n
        elements each) and the multiplicities d_m (2^(2d) elements).  An operand >= 2^bits or a given c that differs raises with code -6
        (PK_ERR_UNSATISFIED), `first_bad` is the smallest such entry (NO_BAD_ENTRY otherwise) and the outputs are not meaningful"""
        bad = C.c_uint64(0)
        rc = lib.pkb_decompose(self.handle, _dev(d_a), _dev(d_b), _dev(d_c), 1 if c_given else 0, self._digits(d_digits), _dev(d_m), C.byref(bad))
        self.first_bad = bad.value
        self._check(rc)

    def prove(self, d_digits, d_m, bind=None, capacity: int | None = None):
        """-> (proof bytes, Claims).  A digit row outside the table or a wrong m raises with code -6 (PK_ERR_UNSATISFIED) and a reason
        that names the digit and the entry; nothing is written then and the prover stays usable"""
        st = self.stmt
        bind_a = _fe(bind, st.n_bind, "bind") if (bind is not None or st.n_bind) else None
        cap = self.proof_bytes if capacity is None else capacity
        buf = (C.c_uint8 * max(cap, 1))()
        if self.fill is not None:
            C.memset(buf, self.fill, max(cap, 1))
        self.buffer = buf
        n = sz()
        claims = ClaimsStruct()
        rc = lib.pkb_prove(self.handle, self._digits(d_digits), _dev(d_m), _ptr(bind_a), C.cast(buf, vp), cap, C.byref(n), C.addressof(claims))
        self.last_len = n.value
        self._check(rc)
        return bytes(buf[: n.value]), Claims(st, claims)
