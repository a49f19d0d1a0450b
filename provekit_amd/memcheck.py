"""Read-write memory checking over device tables (libprovekit_memcheck.so, include/provekit_memcheck.h): prove that a trace of 2^n
operations on a memory of 2^k cells is consistent -- every read returns what the last write to that address left there -- and verify
such proofs on the host.  `Prover.trace` builds the columns rv, rt, fin, ft and m of a trace on the device from its addresses, written
values and initial contents.

An accepted proof is accepted PROVIDED the four values of `Claims`: whir_pcs.Scheme.open / whir_pcs.verify give the columns'
evaluations at z_ops, z_mem, z_f and z_t, `check_claims` forms the four combinations.

A tenth library above the product's C ABI, with its own loader and one signature table (as provekit_amd.tuplelookup).  `verify`,
`check_claims`, the pattern and the proof's length are host only; the prover and `leaves` need a Context.  A rejected proof is a Result,
not an exception; only a failed CALL raises.  There is no fallback: without the built library the import raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import fracsum  # loads libprovekit_fracsum.so (and the sumcheck library under it), which this library links
from ._lib import ProveKitHipError, sz, vp
from .prodcheck import _fe, _ptr
from .runtime import Context, DeviceBuffer
from .verify import Result, ResultStruct

MEMCHECK_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libprovekit_memcheck.so")
MAX_VARS, MAX_BIND, MAX_GRID = 27, 16, 1024
CHECKS = fracsum.CHECKS + ("SIGN", "BALANCE", "TIME_TABLE")
SIDES = ("OPS", "MEM", "TIME")
WHICH = ("NONE", "OPS", "MEM", "RT", "M")  # check_claims
COLUMNS = ("a", "wv", "rv", "rt", "init", "fin", "ft", "m")
LABEL = b"provekit-hip/memcheck/v1"
ERR_BAD_ARG, ERR_UNSATISFIED = -1, -6
NO_BAD_INDEX = 2**64 - 1


class StatementStruct(C.Structure):
    """pkm_statement"""

    _fields_ = [("n", C.c_uint), ("k", C.c_uint), ("n_bind", C.c_uint)]


class ColumnsStruct(C.Structure):
    """pkm_columns"""

    _fields_ = [(name, vp) for name in COLUMNS]


class ClaimsStruct(C.Structure):
    """pkm_claims"""

    _fields_ = [("gamma", C.c_uint64 * 4), ("beta", C.c_uint64 * 4), ("z_ops", (C.c_uint64 * 4) * MAX_VARS), ("z_mem", (C.c_uint64 * 4) * MAX_VARS),
                ("z_f", (C.c_uint64 * 4) * MAX_VARS), ("z_t", (C.c_uint64 * 4) * MAX_VARS), ("ops_coeff", (C.c_uint64 * 4) * 4), ("mem_coeff", (C.c_uint64 * 4) * 3),
                ("ops_value", C.c_uint64 * 4), ("mem_value", C.c_uint64 * 4), ("rt_value", C.c_uint64 * 4), ("m_value", C.c_uint64 * 4)]


# name -> (restype, argtypes); kept in the same order as include/provekit_memcheck.h
SIGNATURES = {
    "pkm_abi_version": (C.c_int, []),
    "pkm_check_name": (C.c_char_p, [C.c_int]),
    "pkm_create_error": (C.c_char_p, []),
    "pkm_io_pattern": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
    "pkm_proof_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkm_prover_arena_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkm_prover_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pkm_prover_destroy": (C.c_int, [vp]),
    "pkm_last_error": (C.c_char_p, [vp]),
    "pkm_trace": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_uint64)]),
    "pkm_leaves": (C.c_int, [vp, C.c_uint, C.c_uint, vp, vp, vp, vp, vp, vp]),
    "pkm_prove": (C.c_int, [vp, vp, vp, vp, sz, C.POINTER(sz), vp]),
    "pkm_verify": (C.c_int, [vp, vp, sz, vp, vp, sz, vp, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(ResultStruct)]),
    "pkm_check_claims": (C.c_int, [vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int)]),
}


def _load():
    if not os.path.exists(MEMCHECK_LIB_PATH):
        raise ImportError(
            f"{MEMCHECK_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C provekit_amd/csrc`). provekit_amd has no CPU fallback."
        )
    return C.CDLL(MEMCHECK_LIB_PATH)  # the libraries it links are the ones already loaded (same files, next to it)


lib = _load()
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


class Statement:
    """2^n operations on a memory of 2^k cells; n_bind caller elements (the roots) are absorbed first"""

    def __init__(self, n: int, k: int, n_bind: int = 0):
        self.n, self.k, self.n_bind = n, k, n_bind

    def struct(self) -> StatementStruct:
        return StatementStruct(self.n, self.k, self.n_bind)


class Claims:
    """what an accepted proof is accepted PROVIDED of, Montgomery [.., 4] uint64: gamma, beta, the points z_ops [n, 4], z_mem [k, 4],
    z_f [n, 4] and z_t [n, 4], the coefficients ops_coeff [4, 4] (of a, wv, rv, rt) and mem_coeff [3, 4] (of init, fin, ft), and the four
    required values"""

    def __init__(self, stmt: Statement, c: ClaimsStruct):
        self.struct = c
        for name in ("gamma", "beta", "ops_value", "mem_value", "rt_value", "m_value"):
            setattr(self, name, np.array(getattr(c, name), dtype=np.uint64))
        for name, count in (("z_ops", stmt.n), ("z_mem", stmt.k), ("z_f", stmt.n), ("z_t", stmt.n), ("ops_coeff", 4), ("mem_coeff", 3)):
            setattr(self, name, np.array([list(getattr(c, name)[i]) for i in range(count)], dtype=np.uint64))


def _refused(rc: int):
    raise ProveKitHipError(rc, lib.pkm_create_error().decode())


def _sized(call, stmt) -> int:
    s = stmt.struct()
    n = sz()
    rc = call(C.addressof(s), C.byref(n))
    if rc:
        _refused(rc)
    return n.value


def io_pattern(stmt: Statement) -> bytes:
    """the spongefish operation list (domain separator) of the outer transcript (host only)"""
    s = stmt.struct()
    n = sz()
    rc = lib.pkm_io_pattern(C.addressof(s), None, 0, C.byref(n))
    if rc:
        _refused(rc)
    buf = (C.c_uint8 * n.value)()
    lib.pkm_io_pattern(C.addressof(s), buf, n.value, C.byref(n))
    return bytes(buf)


def proof_bytes(stmt: Statement) -> int:
    return _sized(lib.pkm_proof_bytes, stmt)


def arena_bytes(stmt: Statement) -> int:
    """the device memory a prover of this statement holds, its three inner provers included (asks the sort for its temporary storage)"""
    return _sized(lib.pkm_prover_arena_bytes, stmt)


def _result(r: ResultStruct) -> Result:
    return Result(bool(r.accepted), CHECKS[r.check] if 0 <= r.check < len(CHECKS) else str(r.check), int(r.offset), r.message.decode(errors="replace"))


def _bytes_arg(b):
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


def verify(stmt: Statement, proof: bytes, bind=None, io_pattern: bytes | None = None):
    """(Result, side, layer, Claims or None): side is "OPS", "MEM" or "TIME" (pkm_verify; host only)"""
    s = stmt.struct()
    bind_a = _fe(bind, stmt.n_bind, "bind") if (bind is not None or stmt.n_bind) else None
    claims, r, side, layer = ClaimsStruct(), ResultStruct(), C.c_int(0), C.c_uint(0)
    pat = _bytes_arg(io_pattern) if io_pattern else None
    pbuf = _bytes_arg(proof)
    rc = lib.pkm_verify(C.addressof(s), C.cast(pat, vp) if pat is not None else None, len(io_pattern) if io_pattern else 0, _ptr(bind_a), C.cast(pbuf, vp),
                        len(proof), C.addressof(claims), C.byref(side), C.byref(layer), C.byref(r))
    if rc:
        _refused(rc)
    res = _result(r)
    return res, SIDES[side.value], layer.value, Claims(stmt, claims) if res.accepted else None


def check_claims(stmt: Statement, claims: Claims, ops_evals, mem_evals, rt_eval, m_eval) -> str:
    """ops_evals [4, 4] = (a, wv, rv, rt)(z_ops), mem_evals [3, 4] = (init, fin, ft)(z_mem), rt_eval [4] = rt(z_f), m_eval [4] = m(z_t),
    Montgomery -> "NONE" when the four claims hold, else the first that does not: "OPS", "MEM", "RT" or "M" (pkm_check_claims; host only)"""
    s = stmt.struct()
    o_a = _fe(np.asarray(ops_evals, dtype=np.uint64).reshape(-1, 4), 4, "ops_evals")
    m_a = _fe(np.asarray(mem_evals, dtype=np.uint64).reshape(-1, 4), 3, "mem_evals")
    r_a = _fe(np.asarray(rt_eval, dtype=np.uint64).reshape(-1, 4), 1, "rt_eval")
    e_a = _fe(np.asarray(m_eval, dtype=np.uint64).reshape(-1, 4), 1, "m_eval")
    which = C.c_int(-1)
    rc = lib.pkm_check_claims(C.addressof(s), C.addressof(claims.struct), _ptr(o_a), _ptr(m_a), _ptr(r_a), _ptr(e_a), C.byref(which))
    if rc:
        _refused(rc)
    return WHICH[which.value]


def _dev(buf):
    return None if buf is None else buf.ptr if isinstance(buf, DeviceBuffer) else int(buf)


def columns(cols) -> ColumnsStruct:
    """cols: a dict (or an object with attributes) of the device columns a, wv, rv, rt, init, fin, ft and m (m may be absent for `leaves`)"""
    get = cols.get if isinstance(cols, dict) else lambda name: getattr(cols, name, None)
    return ColumnsStruct(*[_dev(get(name)) for name in COLUMNS])


def leaves(ctx: Context, n: int, k: int, cols, gamma, beta, d_ops_out, d_mem_out, d_f_out=None) -> None:
    """the two leaf kernels by themselves: the stacked denominator tables of sides OPS (2^(n+1)) and MEM (2^(k+1)), and f = i - rt
    (pkm_leaves)"""
    g, b = _fe(gamma, 1, "gamma"), _fe(beta, 1, "beta")
    c = columns(cols)
    rc = lib.pkm_leaves(ctx.handle, n, k, C.addressof(c), _ptr(g), _ptr(b), _dev(d_ops_out), _dev(d_mem_out), _dev(d_f_out))
    if rc:
        _refused(rc)


class Prover:
    """one statement's prover on a context: owns the two stacked tables, the sign tables, the time side's column and table, the sort's
    storage and the three inner provers, made at creation; a proof allocates no device memory and never writes the caller's tables"""

    fill = None  # a byte the proof buffer (`buffer`) is filled with before a proof, to see afterwards what a refused call wrote: nothing

    def __init__(self, ctx: Context, stmt: Statement):
        self.ctx, self.stmt = ctx, stmt
        s = stmt.struct()
        h = vp()
        rc = lib.pkm_prover_create(ctx.handle, C.addressof(s), C.byref(h))
        if rc:
            _refused(rc)
        self.handle = h
        self.proof_bytes = proof_bytes(stmt)

    def close(self):
        if getattr(self, "handle", None):
            lib.pkm_prover_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return lib.pkm_last_error(self.handle).decode()

    def _check(self, rc: int):
        if rc:
            raise ProveKitHipError(rc, self.last_error())

    def trace(self, d_addr, d_wv, d_init, d_a, d_rv, d_rt, d_fin, d_ft, d_m) -> None:
        """d_addr: 2^n uint32; d_wv: 2^n elements; d_init: 2^k elements -> the caller's tables a, rv, rt, m (2^n) and fin, ft (2^k).  An
        address >= 2^k raises with code -1 (PK_ERR_BAD_ARG) and `first_bad` is the smallest such operation (NO_BAD_INDEX otherwise)"""
        bad = C.c_uint64(0)
        rc = lib.pkm_trace(self.handle, _dev(d_addr), _dev(d_wv), _dev(d_init), _dev(d_a), _dev(d_rv), _dev(d_rt), _dev(d_fin), _dev(d_ft), _dev(d_m), C.byref(bad))
        self.first_bad = bad.value
        self._check(rc)

    def prove(self, cols, bind=None, capacity: int | None = None):
        """cols: the eight device columns (see `columns`) -> (proof bytes, Claims).  An inconsistent trace raises with code -6
        (PK_ERR_UNSATISFIED) and a reason that names the case; nothing is written then and the prover stays usable"""
        st = self.stmt
        bind_a = _fe(bind, st.n_bind, "bind") if (bind is not None or st.n_bind) else None
        cap = self.proof_bytes if capacity is None else capacity
        buf = (C.c_uint8 * max(cap, 1))()
        if self.fill is not None:
            C.memset(buf, self.fill, max(cap, 1))
        self.buffer = buf
        n = sz()
        claims = ClaimsStruct()
        c = columns(cols)
        rc = lib.pkm_prove(self.handle, C.addressof(c), _ptr(bind_a), C.cast(buf, vp), cap, C.byref(n), C.addressof(claims))
        self.last_len = n.value
        self._check(rc)
        return bytes(buf[: n.value]), Claims(st, claims)
