"""GKR grand products and multiset equality over device tables (libprovekit_grandproduct.so, include/provekit_grandproduct.h): prove
that the 2^n entries of a device table multiply to P, or that two sides of w columns hold the same rows as multisets, and verify such
proofs on the host.  A proof costs no commitment beyond the input tables.

An accepted grand product is accepted PROVIDED v(point) = value; an accepted multiset proof PROVIDED the two combinations of
`MultisetClaims`: whir_pcs.Scheme.open / whir_pcs.verify establish them for committed tables.

A seventh library above the product's C ABI, with its own loader and one signature table (as provekit_amd.lookup, whose sumcheck
library it links too).  `verify`, `multiset_verify`, the patterns and the sizes are host only; the provers need a Context.  A rejected
proof is a Result, not an exception; only a failed CALL raises.  There is no fallback: without the built library the import raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import prodcheck  # loads libprovekit_sumcheck.so, which this library links
from ._lib import ProveKitHipError, sz, vp
from .prodcheck import _fe, _ptr, _ptr_array
from .runtime import Context, DeviceBuffer
from .verify import Result, ResultStruct

GRANDPRODUCT_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libprovekit_grandproduct.so")
MAX_VARS, MAX_BIND, MAX_COLUMNS, MAX_GRID = 28, 16, 4, 1024
CHECKS = prodcheck.CHECKS + ("PRODUCT",)
SIDES = ("A", "B")
LABEL = b"provekit-hip/grandproduct/v1"
MULTISET_LABEL = b"provekit-hip/multiset/v1"
ERR_UNSATISFIED = -6


class StatementStruct(C.Structure):
    """pkg_statement"""

    _fields_ = [("n", C.c_uint), ("n_bind", C.c_uint)]


class MultisetStatementStruct(C.Structure):
    """pkg_multiset_statement"""

    _fields_ = [("n", C.c_uint), ("w", C.c_uint), ("n_bind", C.c_uint)]


class MultisetClaimsStruct(C.Structure):
    """pkg_multiset_claims"""

    _fields_ = [("gamma", C.c_uint64 * 4), ("beta", C.c_uint64 * 4), ("z_a", (C.c_uint64 * 4) * MAX_VARS), ("z_b", (C.c_uint64 * 4) * MAX_VARS),
                ("comb_a", C.c_uint64 * 4), ("comb_b", C.c_uint64 * 4)]


# name -> (restype, argtypes); kept in the same order as include/provekit_grandproduct.h
SIGNATURES = {
    "pkg_abi_version": (C.c_int, []),
    "pkg_check_name": (C.c_char_p, [C.c_int]),
    "pkg_create_error": (C.c_char_p, []),
    "pkg_io_pattern": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
    "pkg_proof_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkg_prover_arena_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkg_tail_max_n": (C.c_uint, []),
    "pkg_prover_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pkg_prover_destroy": (C.c_int, [vp]),
    "pkg_last_error": (C.c_char_p, [vp]),
    "pkg_tree": (C.c_int, [vp, C.c_uint, vp, vp, vp]),
    "pkg_prove": (C.c_int, [vp, vp, vp, vp, sz, C.POINTER(sz), vp, vp, vp]),
    "pkg_verify": (C.c_int, [vp, vp, sz, vp, vp, vp, sz, vp, vp, vp, C.POINTER(C.c_uint), C.POINTER(ResultStruct)]),
    "pkg_multiset_io_pattern": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
    "pkg_multiset_proof_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkg_multiset_prover_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pkg_multiset_prover_destroy": (C.c_int, [vp]),
    "pkg_multiset_last_error": (C.c_char_p, [vp]),
    "pkg_multiset_prove": (C.c_int, [vp, vp, vp, vp, vp, sz, C.POINTER(sz), vp]),
    "pkg_multiset_verify": (C.c_int, [vp, vp, sz, vp, vp, sz, vp, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(ResultStruct)]),
}


def _load():
    if not os.path.exists(GRANDPRODUCT_LIB_PATH):
        raise ImportError(
            f"{GRANDPRODUCT_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C provekit_amd/csrc`). provekit_amd has no CPU fallback."
        )
    return C.CDLL(GRANDPRODUCT_LIB_PATH)  # its libprovekit_sumcheck.so and libprovekit_hip.so are the ones already loaded (same files, next to it)


lib = _load()
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


class Statement:
    """a table of 2^n values; n_bind caller elements are absorbed first"""

    def __init__(self, n: int, n_bind: int = 0):
        self.n, self.n_bind = n, n_bind

    def struct(self) -> StatementStruct:
        return StatementStruct(self.n, self.n_bind)


class MultisetStatement:
    """two sides of w columns of 2^n values; n_bind caller elements (the columns' roots) are absorbed first"""

    def __init__(self, n: int, w: int = 1, n_bind: int = 0):
        self.n, self.w, self.n_bind = n, w, n_bind

    def struct(self) -> MultisetStatementStruct:
        return MultisetStatementStruct(self.n, self.w, self.n_bind)


class MultisetClaims:
    """what an accepted multiset proof is accepted PROVIDED of, Montgomery [.., 4] uint64: gamma, beta, the points z_a and z_b [n, 4]
    and the values comb_a, comb_b that sum_j beta^j column_j must take at them"""

    def __init__(self, stmt: MultisetStatement, c: MultisetClaimsStruct):
        for name in ("gamma", "beta", "comb_a", "comb_b"):
            setattr(self, name, np.array(getattr(c, name), dtype=np.uint64))
        self.z_a = np.array([list(c.z_a[i]) for i in range(stmt.n)], dtype=np.uint64)
        self.z_b = np.array([list(c.z_b[i]) for i in range(stmt.n)], dtype=np.uint64)


def _refused(rc: int):
    raise ProveKitHipError(rc, lib.pkg_create_error().decode())


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
    """the spongefish operation list (domain separator) of the outer transcript of a Statement or a MultisetStatement (host only)"""
    return _pattern(lib.pkg_multiset_io_pattern if isinstance(stmt, MultisetStatement) else lib.pkg_io_pattern, stmt)


def proof_bytes(stmt) -> int:
    return _sized(lib.pkg_multiset_proof_bytes if isinstance(stmt, MultisetStatement) else lib.pkg_proof_bytes, stmt)


def arena_bytes(stmt: Statement) -> int:
    """the device memory a GrandProductProver of this statement holds, its sumcheck provers included (host only)"""
    return _sized(lib.pkg_prover_arena_bytes, stmt)


def tail_max_n() -> int:
    """t: a layer of at most 2^t entries is finished by one workgroup out of LDS"""
    return int(lib.pkg_tail_max_n())


def _result(r: ResultStruct) -> Result:
    return Result(bool(r.accepted), CHECKS[r.check] if 0 <= r.check < len(CHECKS) else str(r.check), int(r.offset), r.message.decode(errors="replace"))


def _bytes_arg(b):
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


def verify(stmt: Statement, proof: bytes, bind=None, expected_product=None, io_pattern: bytes | None = None):
    """(Result, layer, (P [4], point [n, 4], value [4]) or None): the layer the verdict is about, 0 for the outer framing and
    transcript; accepted means accepted provided v(point) = value (pkg_verify; host only)"""
    s = stmt.struct()
    bind_a = _fe(bind, stmt.n_bind, "bind") if (bind is not None or stmt.n_bind) else None
    exp_a = _fe(expected_product, 1, "expected_product") if expected_product is not None else None
    r, layer = ResultStruct(), C.c_uint(0)
    product, value, point = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros((max(stmt.n, 1), 4), dtype=np.uint64)
    pat = _bytes_arg(io_pattern) if io_pattern else None
    pbuf = _bytes_arg(proof)
    rc = lib.pkg_verify(C.addressof(s), C.cast(pat, vp) if pat is not None else None, len(io_pattern) if io_pattern else 0, _ptr(bind_a), _ptr(exp_a),
                        C.cast(pbuf, vp), len(proof), product.ctypes.data, point.ctypes.data, value.ctypes.data, C.byref(layer), C.byref(r))
    if rc:
        _refused(rc)
    res = _result(r)
    return res, layer.value, (product, point[: stmt.n], value) if res.accepted else None


def multiset_verify(stmt: MultisetStatement, proof: bytes, bind=None, io_pattern: bytes | None = None):
    """(Result, side, layer, MultisetClaims or None): side is "A" or "B" (pkg_multiset_verify; host only)"""
    s = stmt.struct()
    bind_a = _fe(bind, stmt.n_bind, "bind") if (bind is not None or stmt.n_bind) else None
    claims, r, side, layer = MultisetClaimsStruct(), ResultStruct(), C.c_int(0), C.c_uint(0)
    pat = _bytes_arg(io_pattern) if io_pattern else None
    pbuf = _bytes_arg(proof)
    rc = lib.pkg_multiset_verify(C.addressof(s), C.cast(pat, vp) if pat is not None else None, len(io_pattern) if io_pattern else 0, _ptr(bind_a),
                                 C.cast(pbuf, vp), len(proof), C.addressof(claims), C.byref(side), C.byref(layer), C.byref(r))
    if rc:
        _refused(rc)
    res = _result(r)
    return res, SIDES[side.value], layer.value, MultisetClaims(stmt, claims) if res.accepted else None


def _dev(buf) -> int:
    return buf.ptr if isinstance(buf, DeviceBuffer) else int(buf)


def tree(ctx: Context, n: int, d_v, d_tree_out) -> np.ndarray:
    """the tree kernels by themselves: every layer of d_v (2^n elements) into d_tree_out in heap layout (2^n elements, element 0 not
    written) -> P [4] (pkg_tree)"""
    product = np.zeros(4, dtype=np.uint64)
    rc = lib.pkg_tree(ctx.handle, n, _dev(d_v), _dev(d_tree_out), product.ctypes.data)
    if rc:
        _refused(rc)
    return product


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


class GrandProductProver(_Prover):
    """one statement's prover on a context: owns the tree's arena and n - 1 sumcheck provers, made at creation; a proof allocates no
    device memory and never writes the caller's table"""

    _destroy, _last_error = lib.pkg_prover_destroy, lib.pkg_last_error

    def __init__(self, ctx: Context, stmt: Statement):
        self.ctx, self.stmt = ctx, stmt
        s = stmt.struct()
        h = vp()
        rc = lib.pkg_prover_create(ctx.handle, C.addressof(s), C.byref(h))
        if rc:
            _refused(rc)
        self.handle = h
        self.proof_bytes = proof_bytes(stmt)

    def prove(self, d_v, bind=None, capacity: int | None = None):
        """-> (proof bytes, P [4], point [n, 4], value [4])"""
        bind_a = _fe(bind, self.stmt.n_bind, "bind") if (bind is not None or self.stmt.n_bind) else None
        cap = self.proof_bytes if capacity is None else capacity
        buf = (C.c_uint8 * max(cap, 1))()
        n = sz()
        product, value, point = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros((self.stmt.n, 4), dtype=np.uint64)
        rc = lib.pkg_prove(self.handle, _dev(d_v), _ptr(bind_a), C.cast(buf, vp), cap, C.byref(n), product.ctypes.data, point.ctypes.data, value.ctypes.data)
        self.last_len = n.value
        self._check(rc)
        return bytes(buf[: n.value]), product, point, value


class MultisetProver(_Prover):
    """one statement's prover on a context: ONE grand-product prover and ONE leaf table serve both sides, one after the other"""

    _destroy, _last_error = lib.pkg_multiset_prover_destroy, lib.pkg_multiset_last_error

    def __init__(self, ctx: Context, stmt: MultisetStatement):
        self.ctx, self.stmt = ctx, stmt
        s = stmt.struct()
        h = vp()
        rc = lib.pkg_multiset_prover_create(ctx.handle, C.addressof(s), C.byref(h))
        if rc:
            _refused(rc)
        self.handle = h
        self.proof_bytes = proof_bytes(stmt)

    def prove(self, d_a, d_b, bind=None, capacity: int | None = None):
        """d_a, d_b: w device columns each -> (proof bytes, MultisetClaims).  Sides that are not equal as multisets raise with code -6
        (PK_ERR_UNSATISFIED); nothing is written then and the prover stays usable"""
        assert len(d_a) == len(d_b) == self.stmt.w
        bind_a = _fe(bind, self.stmt.n_bind, "bind") if (bind is not None or self.stmt.n_bind) else None
        cap = self.proof_bytes if capacity is None else capacity
        buf = (C.c_uint8 * max(cap, 1))()
        self.buffer = buf
        n = sz()
        claims = MultisetClaimsStruct()
        rc = lib.pkg_multiset_prove(self.handle, _ptr_array(d_a), _ptr_array(d_b), _ptr(bind_a), C.cast(buf, vp), cap, C.byref(n), C.addressof(claims))
        self.last_len = n.value
        self._check(rc)
        return bytes(buf[: n.value]), MultisetClaims(self.stmt, claims)
