"""Limb-decomposed range checks of up to 64 bits over device tables (libprovekit_rangecheck.so, include/provekit_rangecheck.h): prove
that every entry of a column is below 2^bits by splitting it into limbs of k bits, looking the limbs (and, when the top limb is
shorter, the top limb scaled) up in the identity table 0 .. 2^k - 1 with one tuple-lookup proof, and tying the limbs back to the column
by the recomposition claim.  `Prover.decompose` is the fused device pass: the limb columns and the multiplicities from the column.

An accepted proof is accepted PROVIDED the three claims of `Claims`: whir_pcs.Scheme.open / whir_pcs.verify give f's and the limbs'
evaluations at z_lo and m's at z_t, `check_claims` forms the combinations.

A twelfth library above the product's C ABI, with its own loader and one signature table (as provekit_amd.spark).  `plan`, `verify`,
`check_claims`, the pattern and the lengths are host only; the prover needs a Context.  A rejected proof is a Result, not an exception;
only a failed CALL raises.  There is no fallback: without the built library the import raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import tuplelookup  # loads libprovekit_tuplelookup.so (and the libraries under it), which this library links
from ._lib import ProveKitHipError, sz, vp
from .prodcheck import _fe, _ptr
from .runtime import Context, DeviceBuffer
from .verify import Result, ResultStruct

RANGECHECK_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libprovekit_rangecheck.so")
MAX_VARS, MAX_BIND, MAX_BITS, MAX_LIMB_BITS, MAX_GROUPS, MAX_GRID = 28, 16, 64, 28, 4, 1024
CHECKS = tuplelookup.CHECKS + ("TABLE",)
SIDES = tuplelookup.SIDES
WHICH = ("NONE", "LIMBS", "RECOMPOSE", "M")  # check_claims
LABEL = b"provekit-hip/range/v1"
ERR_BAD_ARG, ERR_UNSATISFIED = -1, -6
NO_BAD_ENTRY = 2**64 - 1


class StatementStruct(C.Structure):
    """pkr_statement"""

    _fields_ = [("n", C.c_uint), ("bits", C.c_uint), ("k", C.c_uint), ("n_bind", C.c_uint)]


class PlanStruct(C.Structure):
    """pkr_limb_plan"""

    _fields_ = [("limbs", C.c_uint), ("top_bits", C.c_uint), ("groups", C.c_uint), ("c", C.c_uint), ("limb_of", C.c_uint * MAX_GROUPS), ("shift_of", C.c_uint * MAX_GROUPS)]


class ClaimsStruct(C.Structure):
    """pkr_claims"""

    _fields_ = [("z_lo", (C.c_uint64 * 4) * MAX_VARS), ("z_t", (C.c_uint64 * 4) * MAX_VARS), ("limb_coeff", (C.c_uint64 * 4) * MAX_GROUPS), ("limbs_value", C.c_uint64 * 4),
                ("pow2", (C.c_uint64 * 4) * MAX_GROUPS), ("m_value", C.c_uint64 * 4)]


# name -> (restype, argtypes); kept in the same order as include/provekit_rangecheck.h
SIGNATURES = {
    "pkr_abi_version": (C.c_int, []),
    "pkr_check_name": (C.c_char_p, [C.c_int]),
    "pkr_create_error": (C.c_char_p, []),
    "pkr_plan": (C.c_int, [vp, vp]),
    "pkr_io_pattern": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
    "pkr_proof_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkr_prover_arena_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkr_count_lds_max_k": (C.c_uint, []),
    "pkr_prover_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pkr_prover_destroy": (C.c_int, [vp]),
    "pkr_last_error": (C.c_char_p, [vp]),
    "pkr_decompose": (C.c_int, [vp, vp, vp, vp, C.POINTER(C.c_uint64)]),
    "pkr_prove": (C.c_int, [vp, vp, vp, vp, vp, sz, C.POINTER(sz), vp]),
    "pkr_verify": (C.c_int, [vp, vp, sz, vp, vp, sz, vp, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(ResultStruct)]),
    "pkr_check_claims": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(C.c_int)]),
}


def _load():
    if not os.path.exists(RANGECHECK_LIB_PATH):
        raise ImportError(
            f"{RANGECHECK_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C provekit_amd/csrc`). provekit_amd has no CPU fallback."
        )
    return C.CDLL(RANGECHECK_LIB_PATH)  # the libraries it links are the ones already loaded (same files, next to it)


lib = _load()
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


class Statement:
    """a column of 2^n entries, each below 2^bits, in limbs of k bits; n_bind caller elements (the roots) are absorbed first"""

    def __init__(self, n: int, bits: int, k: int, n_bind: int = 0):
        self.n, self.bits, self.k, self.n_bind = n, bits, k, n_bind

    def struct(self) -> StatementStruct:
        return StatementStruct(self.n, self.bits, self.k, self.n_bind)


class Plan:
    """pkr_plan's answer: limbs L, top_bits r, groups G, the lookup's c, and per group g < c the limb it looks up and its shift"""

    def __init__(self, p: PlanStruct):
        self.limbs, self.top_bits, self.groups, self.c = p.limbs, p.top_bits, p.groups, p.c
        self.limb_of, self.shift_of = list(p.limb_of)[: p.c], list(p.shift_of)[: p.c]


class Claims:
    """what an accepted proof is accepted PROVIDED of, Montgomery [.., 4] uint64: the points z_lo [n, 4] and z_t [k, 4], limb_coeff
    [L, 4] with limbs_value [4], pow2 [L, 4] = 2^(k i), m_value [4]"""

    def __init__(self, stmt: Statement, c: ClaimsStruct):
        self.struct = c
        L = -(-stmt.bits // stmt.k)
        a = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731
        self.z_lo = a([list(c.z_lo[i]) for i in range(stmt.n)])
        self.z_t = a([list(c.z_t[i]) for i in range(stmt.k)])
        self.limb_coeff = a([list(c.limb_coeff[i]) for i in range(L)])
        self.pow2 = a([list(c.pow2[i]) for i in range(L)])
        self.limbs_value, self.m_value = a(c.limbs_value), a(c.m_value)


def _refused(rc: int):
    raise ProveKitHipError(rc, lib.pkr_create_error().decode())


def _sized(call, stmt) -> int:
    s = stmt.struct()
    n = sz()
    rc = call(C.addressof(s), C.byref(n))
    if rc:
        _refused(rc)
    return n.value


def plan(stmt: Statement) -> Plan:
    """the limbs and groups of a statement; a statement the library does not take raises with the reason (pkr_plan; host only)"""
    s, p = stmt.struct(), PlanStruct()
    rc = lib.pkr_plan(C.addressof(s), C.addressof(p))
    if rc:
        _refused(rc)
    return Plan(p)


def io_pattern(stmt: Statement) -> bytes:
    """the spongefish operation list (domain separator) of the outer transcript (host only)"""
    s = stmt.struct()
    n = sz()
    rc = lib.pkr_io_pattern(C.addressof(s), None, 0, C.byref(n))
    if rc:
        _refused(rc)
    buf = (C.c_uint8 * n.value)()
    lib.pkr_io_pattern(C.addressof(s), buf, n.value, C.byref(n))
    return bytes(buf)


def proof_bytes(stmt: Statement) -> int:
    return _sized(lib.pkr_proof_bytes, stmt)


def arena_bytes(stmt: Statement) -> int:
    """the device memory a prover of this statement holds, its lookup prover included (host only)"""
    return _sized(lib.pkr_prover_arena_bytes, stmt)


def count_lds_max_k() -> int:
    """limbs of up to this many bits are counted in a workgroup's LDS histogram"""
    return int(lib.pkr_count_lds_max_k())


def _result(r: ResultStruct) -> Result:
    return Result(bool(r.accepted), CHECKS[r.check] if 0 <= r.check < len(CHECKS) else str(r.check), int(r.offset), r.message.decode(errors="replace"))


def _bytes_arg(b):
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


def verify(stmt: Statement, proof: bytes, bind=None, io_pattern: bytes | None = None):
    """(Result, side, layer, Claims or None): side is "F" or "T", the lookup's (pkr_verify; host only)"""
    s = stmt.struct()
    bind_a = _fe(bind, stmt.n_bind, "bind") if (bind is not None or stmt.n_bind) else None
    claims, r, side, layer = ClaimsStruct(), ResultStruct(), C.c_int(0), C.c_uint(0)
    pat = _bytes_arg(io_pattern) if io_pattern else None
    pbuf = _bytes_arg(proof)
    rc = lib.pkr_verify(C.addressof(s), C.cast(pat, vp) if pat is not None else None, len(io_pattern) if io_pattern else 0, _ptr(bind_a), C.cast(pbuf, vp), len(proof),
                        C.addressof(claims), C.byref(side), C.byref(layer), C.byref(r))
    if rc:
        _refused(rc)
    res = _result(r)
    return res, SIDES[side.value], layer.value, Claims(stmt, claims) if res.accepted else None


def check_claims(stmt: Statement, claims: Claims, f_eval, limb_evals, m_eval) -> str:
    """f_eval [4] = f(z_lo), limb_evals [L, 4] = limb_i(z_lo), m_eval [4] = m(z_t), Montgomery -> "NONE" when the three claims hold,
    else the first that does not: "LIMBS", "RECOMPOSE" or "M" (pkr_check_claims; host only)"""
    s = stmt.struct()
    L = -(-stmt.bits // stmt.k) if stmt.k else 1
    f_a = _fe(np.asarray(f_eval, dtype=np.uint64).reshape(-1, 4), 1, "f_eval")
    l_a = _fe(np.asarray(limb_evals, dtype=np.uint64).reshape(-1, 4), L, "limb_evals")
    m_a = _fe(np.asarray(m_eval, dtype=np.uint64).reshape(-1, 4), 1, "m_eval")
    which = C.c_int(-1)
    rc = lib.pkr_check_claims(C.addressof(s), C.addressof(claims.struct), _ptr(f_a), _ptr(l_a), _ptr(m_a), C.byref(which))
    if rc:
        _refused(rc)
    return WHICH[which.value]


def _dev(buf):
    return None if buf is None else buf.ptr if isinstance(buf, DeviceBuffer) else int(buf)


class Prover:
    """one statement's prover on a context: owns the table 0 .. 2^k - 1, the scaled top column, the counts and the lookup prover, made
    at creation; a proof allocates no device memory and never writes the caller's tables"""

    fill = None  # a byte the proof buffer (`buffer`) is filled with before a proof, to see afterwards what a refused call wrote: nothing

    def __init__(self, ctx: Context, stmt: Statement):
        self.ctx, self.stmt = ctx, stmt
        s = stmt.struct()
        h = vp()
        rc = lib.pkr_prover_create(ctx.handle, C.addressof(s), C.byref(h))
        if rc:
            _refused(rc)
        self.handle = h
        self.proof_bytes = proof_bytes(stmt)
        self.plan = plan(stmt)
        self.first_bad = NO_BAD_ENTRY

    def close(self):
        if getattr(self, "handle", None):
            lib.pkr_prover_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return lib.pkr_last_error(self.handle).decode()

    def _check(self, rc: int):
        if rc:
            raise ProveKitHipError(rc, self.last_error())

    def _limbs(self, d_limbs):
        if len(d_limbs) != self.plan.limbs:
            raise ValueError(f"{self.plan.limbs} limb columns expected, {len(d_limbs)} given")
        return (vp * self.plan.limbs)(*[_dev(b) for b in d_limbs])

    def decompose(self, d_f, d_limbs, d_m) -> None:
        """d_f: 2^n elements -> the L limb columns d_limbs (2^n elements each) and the multiplicities d_m (2^k elements).  An entry
        >= 2^bits raises with code -6 (PK_ERR_UNSATISFIED), `first_bad` is the smallest such entry (NO_BAD_ENTRY otherwise) and the
        outputs are not meaningful"""
        bad = C.c_uint64(0)
        rc = lib.pkr_decompose(self.handle, _dev(d_f), self._limbs(d_limbs), _dev(d_m), C.byref(bad))
        self.first_bad = bad.value
        self._check(rc)

    def prove(self, d_limbs, d_m, bind=None, capacity: int | None = None):
        """-> (proof bytes, Claims).  A limb outside 0 .. 2^k - 1, a top limb outside 0 .. 2^r - 1 or a wrong m raises with code -6
        (PK_ERR_UNSATISFIED) and a reason that names the group and the entry; nothing is written then and the prover stays usable"""
        st = self.stmt
        bind_a = _fe(bind, st.n_bind, "bind") if (bind is not None or st.n_bind) else None
        cap = self.proof_bytes if capacity is None else capacity
        buf = (C.c_uint8 * max(cap, 1))()
        if self.fill is not None:
            C.memset(buf, self.fill, max(cap, 1))
        self.buffer = buf
        n = sz()
        claims = ClaimsStruct()
        rc = lib.pkr_prove(self.handle, self._limbs(d_limbs), _dev(d_m), _ptr(bind_a), C.cast(buf, vp), cap, C.byref(n), C.addressof(claims))
        self.last_len = n.value
        self._check(rc)
        return bytes(buf[: n.value]), Claims(st, claims)
