"""GKR fractional sums and LogUp lookups without helper columns (libprovekit_fracsum.so, include/provekit_fracsum.h): prove that
sum_x p[x] / q[x] = P / Q over device tables, or that every entry of a device column f is an entry of a table t with multiplicities m,
and verify such proofs on the host.  A proof costs no commitment beyond the input tables and no field inversion.

An accepted fractional sum is accepted PROVIDED q(point) = value_q and, with numerators, p(point) = value_p; an accepted lookup
PROVIDED the three values of `LookupClaims`: whir_pcs.Scheme.open / whir_pcs.verify establish them for committed tables.

An eighth library above the product's C ABI, with its own loader and one signature table (as provekit_amd.grandproduct, whose
sumcheck library it links too).  `verify`, `lookup_verify`, the patterns and the sizes are host only; the provers need a Context.  A
rejected proof is a Result, not an exception; only a failed CALL raises.  There is no fallback: without the built library the import
raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import prodcheck  # loads libprovekit_sumcheck.so, which this library links
from ._lib import ProveKitHipError, sz, vp
from .prodcheck import _fe, _ptr
from .runtime import Context, DeviceBuffer
from .verify import Result, ResultStruct

FRACSUM_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libprovekit_fracsum.so")
MAX_VARS, MAX_BIND, MAX_GRID = 28, 16, 1024
CHECKS = prodcheck.CHECKS + ("FRACTION", "DENOMINATOR", "UNIT")
SIDES = ("F", "T")
LABEL = b"provekit-hip/fracsum/v1"
LOOKUP_LABEL = b"provekit-hip/logup-gkr/v1"
ERR_UNSATISFIED = -6


class StatementStruct(C.Structure):
    """pkf_statement"""

    _fields_ = [("n", C.c_uint), ("n_bind", C.c_uint), ("unit", C.c_uint)]


class LookupStatementStruct(C.Structure):
    """pkf_lookup_statement"""

    _fields_ = [("n", C.c_uint), ("k", C.c_uint), ("n_bind", C.c_uint)]


class LookupClaimsStruct(C.Structure):
    """pkf_lookup_claims"""

    _fields_ = [("alpha", C.c_uint64 * 4), ("z_f", (C.c_uint64 * 4) * MAX_VARS), ("z_t", (C.c_uint64 * 4) * MAX_VARS), ("f_value", C.c_uint64 * 4),
                ("t_value", C.c_uint64 * 4), ("m_value", C.c_uint64 * 4)]


# name -> (restype, argtypes); kept in the same order as include/provekit_fracsum.h
SIGNATURES = {
    "pkf_abi_version": (C.c_int, []),
    "pkf_check_name": (C.c_char_p, [C.c_int]),
    "pkf_create_error": (C.c_char_p, []),
    "pkf_io_pattern": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
    "pkf_proof_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkf_prover_arena_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkf_tail_max_n": (C.c_uint, []),
    "pkf_prover_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pkf_prover_destroy": (C.c_int, [vp]),
    "pkf_last_error": (C.c_char_p, [vp]),
    "pkf_tree": (C.c_int, [vp, C.c_uint, vp, vp, vp, vp, vp]),
    "pkf_prove": (C.c_int, [vp, vp, vp, vp, vp, sz, C.POINTER(sz), vp, vp, vp, vp]),
    "pkf_verify": (C.c_int, [vp, vp, sz, vp, vp, vp, sz, vp, vp, vp, vp, C.POINTER(C.c_uint), C.POINTER(ResultStruct)]),
    "pkf_lookup_io_pattern": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
    "pkf_lookup_proof_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkf_lookup_prover_arena_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkf_lookup_prover_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pkf_lookup_prover_destroy": (C.c_int, [vp]),
    "pkf_lookup_last_error": (C.c_char_p, [vp]),
    "pkf_lookup_prove": (C.c_int, [vp, vp, vp, vp, vp, vp, sz, C.POINTER(sz), vp]),
    "pkf_lookup_verify": (C.c_int, [vp, vp, sz, vp, vp, sz, vp, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(ResultStruct)]),
}


def _load():
    if not os.path.exists(FRACSUM_LIB_PATH):
        raise ImportError(
            f"{FRACSUM_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C provekit_amd/csrc`). provekit_amd has no CPU fallback."
        )
    return C.CDLL(FRACSUM_LIB_PATH)  # its libprovekit_sumcheck.so and libprovekit_hip.so are the ones already loaded (same files, next to it)


lib = _load()
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


class Statement:
    """tables of 2^n entries; unit: no numerator table, every numerator is 1; n_bind caller elements are absorbed first"""

    def __init__(self, n: int, n_bind: int = 0, unit: int = 0):
        self.n, self.n_bind, self.unit = n, n_bind, int(unit)

    def struct(self) -> StatementStruct:
        return StatementStruct(self.n, self.n_bind, self.unit)


class LookupStatement:
    """a column f of 2^n entries, a table t and multiplicities m of 2^k; n_bind caller elements (the roots) are absorbed first"""

    def __init__(self, n: int, k: int, n_bind: int = 0):
        self.n, self.k, self.n_bind = n, k, n_bind

    def struct(self) -> LookupStatementStruct:
        return LookupStatementStruct(self.n, self.k, self.n_bind)


class LookupClaims:
    """what an accepted lookup proof is accepted PROVIDED of, Montgomery [.., 4] uint64: alpha, the points z_f [n, 4] and z_t [k, 4] and
    the values f(z_f), t(z_t) and m(z_t) must take"""

    def __init__(self, stmt: LookupStatement, c: LookupClaimsStruct):
        for name in ("alpha", "f_value", "t_value", "m_value"):
            setattr(self, name, np.array(getattr(c, name), dtype=np.uint64))
        self.z_f = np.array([list(c.z_f[i]) for i in range(stmt.n)], dtype=np.uint64)
        self.z_t = np.array([list(c.z_t[i]) for i in range(stmt.k)], dtype=np.uint64)


def _refused(rc: int):
    raise ProveKitHipError(rc, lib.pkf_create_error().decode())


def _sized(call, stmt) -> int:
    s = stmt.struct()
    n = sz()
    rc = call(C.addressof(s), C.byref(n))
    if rc:
        _refused(rc)
    return n.value


def _pattern(call, stmt) -> bytes:
    s = stmt.struct()
    n = sz()
    rc = call(C.addressof(s), None, 0, C.byref(n))
    if rc:
        _refused(rc)
    buf = (C.c_uint8 * n.value)()
    call(C.addressof(s), buf, n.value, C.byref(n))
    return bytes(buf)


def io_pattern(stmt) -> bytes:
    """the spongefish operation list (domain separator) of the outer transcript of a Statement or a LookupStatement (host only)"""
    return _pattern(lib.pkf_lookup_io_pattern if isinstance(stmt, LookupStatement) else lib.pkf_io_pattern, stmt)


def proof_bytes(stmt) -> int:
    return _sized(lib.pkf_lookup_proof_bytes if isinstance(stmt, LookupStatement) else lib.pkf_proof_bytes, stmt)


def arena_bytes(stmt) -> int:
    """the device memory a prover of this statement holds, its sumcheck provers included (host only)"""
    return _sized(lib.pkf_lookup_prover_arena_bytes if isinstance(stmt, LookupStatement) else lib.pkf_prover_arena_bytes, stmt)


def tail_max_n() -> int:
    """t: a layer of at most 2^t entries is finished by one workgroup out of LDS"""
    return int(lib.pkf_tail_max_n())


def _result(r: ResultStruct) -> Result:
    return Result(bool(r.accepted), CHECKS[r.check] if 0 <= r.check < len(CHECKS) else str(r.check), int(r.offset), r.message.decode(errors="replace"))


def _bytes_arg(b):
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


def verify(stmt: Statement, proof: bytes, bind=None, expected_fraction=None, io_pattern: bytes | None = None):
    """expected_fraction: [2, 4] (num, den) or None.  -> (Result, layer, (fraction [2, 4], point [n, 4], value_p [4] or None, value_q [4])
    or None): the layer the verdict is about, 0 for the outer framing, the top and the transcript (pkf_verify; host only)"""
    s = stmt.struct()
    bind_a = _fe(bind, stmt.n_bind, "bind") if (bind is not None or stmt.n_bind) else None
    exp_a = _fe(expected_fraction, 2, "expected_fraction") if expected_fraction is not None else None
    r, layer = ResultStruct(), C.c_uint(0)
    fraction, point = np.zeros((2, 4), dtype=np.uint64), np.zeros((max(stmt.n, 1), 4), dtype=np.uint64)
    value_p, value_q = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    pat = _bytes_arg(io_pattern) if io_pattern else None
    pbuf = _bytes_arg(proof)
    rc = lib.pkf_verify(C.addressof(s), C.cast(pat, vp) if pat is not None else None, len(io_pattern) if io_pattern else 0, _ptr(bind_a), _ptr(exp_a),
                        C.cast(pbuf, vp), len(proof), fraction.ctypes.data, point.ctypes.data, value_p.ctypes.data, value_q.ctypes.data, C.byref(layer), C.byref(r))
    if rc:
        _refused(rc)
    res = _result(r)
    return res, layer.value, (fraction, point[: stmt.n], None if stmt.unit else value_p, value_q) if res.accepted else None


def lookup_verify(stmt: LookupStatement, proof: bytes, bind=None, io_pattern: bytes | None = None):
    """(Result, side, layer, LookupClaims or None): side is "F" or "T" (pkf_lookup_verify; host only)"""
    s = stmt.struct()
    bind_a = _fe(bind, stmt.n_bind, "bind") if (bind is not None or stmt.n_bind) else None
    claims, r, side, layer = LookupClaimsStruct(), ResultStruct(), C.c_int(0), C.c_uint(0)
    pat = _bytes_arg(io_pattern) if io_pattern else None
    pbuf = _bytes_arg(proof)
    rc = lib.pkf_lookup_verify(C.addressof(s), C.cast(pat, vp) if pat is not None else None, len(io_pattern) if io_pattern else 0, _ptr(bind_a),
                               C.cast(pbuf, vp), len(proof), C.addressof(claims), C.byref(side), C.byref(layer), C.byref(r))
    if rc:
        _refused(rc)
    res = _result(r)
    return res, SIDES[side.value], layer.value, LookupClaims(stmt, claims) if res.accepted else None


def _dev(buf):
    return None if buf is None else buf.ptr if isinstance(buf, DeviceBuffer) else int(buf)


def tree(ctx: Context, n: int, d_p, d_q, d_ptree_out, d_qtree_out) -> np.ndarray:
    """the tree kernels by themselves: every layer of the leaves (d_p, d_q) (2^n elements each; d_p None: unit) into the two trees in
    heap layout (2^n elements each, element 0 not written) -> (P, Q) [2, 4] (pkf_tree)"""
    fraction = np.zeros((2, 4), dtype=np.uint64)
    rc = lib.pkf_tree(ctx.handle, n, _dev(d_p), _dev(d_q), _dev(d_ptree_out), _dev(d_qtree_out), fraction.ctypes.data)
    if rc:
        _refused(rc)
    return fraction


class _Prover:
    _destroy = _last_error = None

    def close(self):
        if getattr(self, "handle", None):
            self._destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return self._last_error(self.handle).decode()

    def _check(self, rc: int):
        if rc:
            raise ProveKitHipError(rc, self.last_error())


class FractionalSumProver(_Prover):
    """one statement's prover on a context: owns both trees' arena and n - 1 sumcheck provers, made at creation; a proof allocates no
    device memory and never writes the caller's tables"""

    _destroy, _last_error = lib.pkf_prover_destroy, lib.pkf_last_error

    def __init__(self, ctx: Context, stmt: Statement):
        self.ctx, self.stmt = ctx, stmt
        s = stmt.struct()
        h = vp()
        rc = lib.pkf_prover_create(ctx.handle, C.addressof(s), C.byref(h))
        if rc:
            _refused(rc)
        self.handle = h
        self.proof_bytes = proof_bytes(stmt)

    def prove(self, d_p, d_q, bind=None, capacity: int | None = None):
        """d_p None exactly for a unit statement -> (proof bytes, fraction [2, 4], point [n, 4], value_p [4] or None, value_q [4]).  A
        zero denominator raises with code -6 (PK_ERR_UNSATISFIED); nothing is written then and the prover stays usable"""
        bind_a = _fe(bind, self.stmt.n_bind, "bind") if (bind is not None or self.stmt.n_bind) else None
        cap = self.proof_bytes if capacity is None else capacity
        buf = (C.c_uint8 * max(cap, 1))()
        self.buffer = buf
        n = sz()
        fraction, point = np.zeros((2, 4), dtype=np.uint64), np.zeros((self.stmt.n, 4), dtype=np.uint64)
        value_p, value_q = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        rc = lib.pkf_prove(self.handle, _dev(d_p), _dev(d_q), _ptr(bind_a), C.cast(buf, vp), cap, C.byref(n), fraction.ctypes.data, point.ctypes.data,
                           value_p.ctypes.data, value_q.ctypes.data)
        self.last_len = n.value
        self._check(rc)
        return bytes(buf[: n.value]), fraction, point, None if self.stmt.unit else value_p, value_q


class LookupProver(_Prover):
    """one statement's prover on a context: a fractional-sum prover and a leaf table per side"""

    _destroy, _last_error = lib.pkf_lookup_prover_destroy, lib.pkf_lookup_last_error

    def __init__(self, ctx: Context, stmt: LookupStatement):
        self.ctx, self.stmt = ctx, stmt
        s = stmt.struct()
        h = vp()
        rc = lib.pkf_lookup_prover_create(ctx.handle, C.addressof(s), C.byref(h))
        if rc:
            _refused(rc)
        self.handle = h
        self.proof_bytes = proof_bytes(stmt)

    def prove(self, d_f, d_t, d_m, bind=None, capacity: int | None = None):
        """-> (proof bytes, LookupClaims).  A column that is not inside the table under m, or an alpha that is an entry, raises with code
        -6 (PK_ERR_UNSATISFIED); nothing is written then and the prover stays usable"""
        bind_a = _fe(bind, self.stmt.n_bind, "bind") if (bind is not None or self.stmt.n_bind) else None
        cap = self.proof_bytes if capacity is None else capacity
        buf = (C.c_uint8 * max(cap, 1))()
        self.buffer = buf
        n = sz()
        claims = LookupClaimsStruct()
        rc = lib.pkf_lookup_prove(self.handle, _dev(d_f), _dev(d_t), _dev(d_m), _ptr(bind_a), C.cast(buf, vp), cap, C.byref(n), C.addressof(claims))
        self.last_len = n.value
        self._check(rc)
        return bytes(buf[: n.value]), LookupClaims(self.stmt, claims)
