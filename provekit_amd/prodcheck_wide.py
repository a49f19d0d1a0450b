"""Wide product sumchecks over device tables (libprovekit_sumcheck.so, include/provekit_sumcheck_wide.h): prove that
sum_x eq(tau, x) * sum_t c_t * prod_i f_{t,i}(x) = s for up to 16 device-resident tables, 16 terms and powers of a table up to degree
5 -- a Plonk gate, an x^5 S-box, a custom gate -- and verify such a proof on the host.

The sibling of provekit_amd.prodcheck (pks_*) in the same library: the same protocol and proof layout under another label, so the two
are not interchangeable on the wire.  Where a statement fits both, prodcheck is the faster prover.  An accepted proof is accepted
PROVIDED f_j(point) = finals[j].  `verify`, `io_pattern`, `proof_bytes` and `arena_bytes` are host only; `Prover` and `round` need a
Context.  A rejected proof is a Result, not an exception; only a failed CALL raises.  There is no fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import prodcheck as _pks
from ._lib import ProveKitHipError, sz, vp
from .prodcheck import CHECKS, MAX_BIND, MAX_GRID, MAX_VARS, P, Proof, _fe, _mont_limbs, _ptr, _ptr_array, lib
from .runtime import Context
from .verify import Result, ResultStruct

MAX_TABLES, MAX_TERMS, MAX_DEGREE = 16, 16, 5
LABEL = b"provekit-hip/sumcheck-wide/v1"


class StatementStruct(C.Structure):
    """pksw_statement"""

    _fields_ = [("n", C.c_uint), ("m", C.c_uint), ("T", C.c_uint), ("has_tau", C.c_uint), ("n_bind", C.c_uint), ("lens", C.c_uint * MAX_TERMS),
                ("factors", (C.c_uint * MAX_DEGREE) * MAX_TERMS), ("coeffs", (C.c_uint64 * 4) * MAX_TERMS)]


# name -> (restype, argtypes); kept in the same order as include/provekit_sumcheck_wide.h
SIGNATURES = {
    "pksw_abi_version": (C.c_int, []),
    "pksw_create_error": (C.c_char_p, []),
    "pksw_io_pattern": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
    "pksw_proof_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pksw_arena_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pksw_prover_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pksw_prover_destroy": (C.c_int, [vp]),
    "pksw_last_error": (C.c_char_p, [vp]),
    "pksw_prove": (C.c_int, [vp, vp, vp, vp, vp, sz, C.POINTER(sz), vp, vp]),
    "pksw_verify": (C.c_int, [vp, vp, sz, vp, vp, vp, vp, sz, vp, vp, C.POINTER(ResultStruct)]),
    "pksw_round": (C.c_int, [vp, vp, vp, sz, vp, vp, vp, C.c_uint, vp]),
}

for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


class Statement:
    """n variables, m tables, terms = [(coefficient, [table, table, ...]), ...]: the coefficient an int (taken mod p) or 4 Montgomery
    limbs as they are, the list the term's factors, a repeated table a power.  Nothing is checked here: the library refuses"""

    def __init__(self, n: int, m: int, terms, has_tau: bool = False, n_bind: int = 0):
        self.n, self.m, self.has_tau, self.n_bind = n, m, bool(has_tau), n_bind
        self.terms = [(coeff, list(factors)) for coeff, factors in terms]

    @property
    def degree(self) -> int:
        return max(len(factors) for _, factors in self.terms)

    def struct(self) -> StatementStruct:
        s = StatementStruct()
        s.n, s.m, s.T, s.has_tau, s.n_bind = self.n, self.m, len(self.terms), int(self.has_tau), self.n_bind
        for t, (coeff, factors) in enumerate(self.terms[:MAX_TERMS]):
            s.lens[t] = len(factors)  # a list of 6 keeps its length: the library refuses it
            for i, j in enumerate(factors[:MAX_DEGREE]):
                s.factors[t][i] = j
            limbs = _mont_limbs(coeff) if isinstance(coeff, int) else [int(x) for x in coeff]
            for i in range(4):
                s.coeffs[t][i] = limbs[i]
        return s


def _refused(rc: int):
    raise ProveKitHipError(rc, lib.pksw_create_error().decode())


def _size(fn, stmt: Statement) -> int:
    s = stmt.struct()
    n = sz()
    rc = fn(C.addressof(s), C.byref(n))
    if rc:
        _refused(rc)
    return n.value


def io_pattern(stmt: Statement) -> bytes:
    """the spongefish operation list (domain separator) of a proof of this statement (pksw_io_pattern; host only)"""
    s = stmt.struct()
    n = sz()
    rc = lib.pksw_io_pattern(C.addressof(s), None, 0, C.byref(n))
    if rc:
        _refused(rc)
    buf = (C.c_uint8 * n.value)()
    lib.pksw_io_pattern(C.addressof(s), buf, n.value, C.byref(n))
    return bytes(buf)


def proof_bytes(stmt: Statement) -> int:
    return _size(lib.pksw_proof_bytes, stmt)


def arena_bytes(stmt: Statement) -> int:
    """the device memory a Prover of this statement allocates (pksw_arena_bytes; host only)"""
    return _size(lib.pksw_arena_bytes, stmt)


def verify(stmt: Statement, proof: bytes, tau=None, bind=None, expected_sum=None, io_pattern: bytes | None = None):
    """(Result, point [n, 4], finals [m, 4]) -- Montgomery; accepted means accepted provided f_j(point) = finals[j] (pksw_verify; host only)"""
    s = stmt.struct()
    tau_a = _fe(tau, stmt.n if stmt.has_tau else 0, "tau") if (tau is not None or stmt.has_tau) else None
    bind_a = _fe(bind, stmt.n_bind, "bind") if (bind is not None or stmt.n_bind) else None
    exp_a = _fe(expected_sum, 1, "expected_sum") if expected_sum is not None else None
    point = np.zeros((stmt.n, 4), dtype=np.uint64)
    finals = np.zeros((stmt.m, 4), dtype=np.uint64)
    r = ResultStruct()
    pat = (C.c_uint8 * len(io_pattern)).from_buffer_copy(io_pattern) if io_pattern else None
    pbuf = (C.c_uint8 * max(len(proof), 1)).from_buffer_copy(bytes(proof) or b"\0")
    rc = lib.pksw_verify(C.addressof(s), C.cast(pat, vp) if pat is not None else None, len(io_pattern) if io_pattern else 0, _ptr(tau_a), _ptr(bind_a),
                         _ptr(exp_a), C.cast(pbuf, vp), len(proof), point.ctypes.data, finals.ctypes.data, C.byref(r))
    if rc:
        _refused(rc)
    res = Result(bool(r.accepted), CHECKS[r.check] if 0 <= r.check < len(CHECKS) else str(r.check), int(r.offset), r.message.decode(errors="replace"))
    return res, point, finals


class Prover(_pks.Prover):
    """one wide statement's prover on a context: owns one device arena sized at creation (arena_bytes); prove() allocates no device
    memory and never writes the caller's tables"""

    def __init__(self, ctx: Context, stmt: Statement):
        self.ctx, self.stmt = ctx, stmt
        s = stmt.struct()
        h = vp()
        rc = lib.pksw_prover_create(ctx.handle, C.addressof(s), C.byref(h))
        if rc:
            _refused(rc)
        self.handle = h
        self.proof_bytes = proof_bytes(stmt)

    def close(self):
        if getattr(self, "handle", None):
            lib.pksw_prover_destroy(self.handle)
            self.handle = None

    def last_error(self) -> str:
        return lib.pksw_last_error(self.handle).decode()

    def prove(self, d_tables, tau=None, bind=None, capacity: int | None = None) -> Proof:
        """d_tables: m DeviceBuffers (or device addresses) of 2^n Montgomery elements"""
        return self._prove_with(lib.pksw_prove, d_tables, tau, bind, capacity)


def round(ctx: Context, stmt: Statement, d_tables, length: int, tau_rest=None, fold=None, d_out_tables=None, grid: int = 0) -> np.ndarray:
    """[D + 1, 4] Montgomery: h(0) .. h(D) of ONE round on tables of current length `length`, folded first by `fold` into d_out_tables if
    given (pksw_round).  grid = 0: the library's rule; the bits do not depend on it"""
    s = stmt.struct()
    out = np.zeros((stmt.degree + 1, 4), dtype=np.uint64)
    tau_a = np.ascontiguousarray(tau_rest, dtype=np.uint64).reshape(-1, 4) if tau_rest is not None else None
    fold_a = _fe(fold, 1, "fold") if fold is not None else None
    outs = C.cast(_ptr_array(d_out_tables), vp) if d_out_tables is not None else None
    rc = lib.pksw_round(ctx.handle, C.addressof(s), C.cast(_ptr_array(d_tables), vp), length, tau_a.ctypes.data if tau_a is not None else None, _ptr(fold_a),
                        outs, grid, out.ctypes.data)
    if rc:
        _refused(rc)
    return out
