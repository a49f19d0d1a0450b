"""Product sumchecks over device tables (libprovekit_sumcheck.so, include/provekit_sumcheck.h): prove that
sum_x eq(tau, x) * sum_t c_t * prod_{j in S_t} f_j(x) = s for up to 4 device-resident tables, and verify such a proof on the host.

An accepted proof is accepted PROVIDED f_j(point) = finals[j]: the sumcheck reduces the sum to those evaluation claims, which
whir_pcs.Scheme.open / whir_pcs.verify at `point` establish for committed tables (the coordinate order is already theirs).

A fifth library above the product's C ABI, with its own loader and one signature table (as provekit_amd.whir_pcs).  `verify`,
`io_pattern` and `proof_bytes` are host only; `Prover` and `round` need a Context.  A rejected proof is a Result, not an exception;
only a failed CALL raises.  There is no fallback: without the built library the import raises.  (provekit_amd.sumcheck is the
product's own two round kernels, a different thing.)"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._lib import ProveKitHipError, sz, vp
from .runtime import Context, DeviceBuffer
from .verify import CHECKS as WALK_CHECKS
from .verify import Result, ResultStruct

SUMCHECK_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libprovekit_sumcheck.so")
MAX_TABLES, MAX_TERMS, MAX_TERM_TABLES, MAX_VARS, MAX_BIND, MAX_GRID = 4, 4, 3, 28, 16, 1024
CHECKS = WALK_CHECKS + ("ROUND", "FINAL", "SUM")
LABEL = b"provekit-hip/sumcheck/v1"

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
_R = (1 << 256) % P


class StatementStruct(C.Structure):
    """pks_statement"""

    _fields_ = [("n", C.c_uint), ("m", C.c_uint), ("T", C.c_uint), ("has_tau", C.c_uint), ("n_bind", C.c_uint), ("masks", C.c_uint * 4),
                ("coeffs", (C.c_uint64 * 4) * 4)]


# name -> (restype, argtypes); kept in the same order as include/provekit_sumcheck.h
SIGNATURES = {
    "pks_abi_version": (C.c_int, []),
    "pks_check_name": (C.c_char_p, [C.c_int]),
    "pks_create_error": (C.c_char_p, []),
    "pks_io_pattern": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
    "pks_proof_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pks_prover_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pks_prover_destroy": (C.c_int, [vp]),
    "pks_last_error": (C.c_char_p, [vp]),
    "pks_prove": (C.c_int, [vp, vp, vp, vp, vp, sz, C.POINTER(sz), vp, vp]),
    "pks_verify": (C.c_int, [vp, vp, sz, vp, vp, vp, vp, sz, vp, vp, C.POINTER(ResultStruct)]),
    "pks_round": (C.c_int, [vp, vp, vp, sz, vp, vp, vp, C.c_uint, vp]),
}


def _load():
    if not os.path.exists(SUMCHECK_LIB_PATH):
        raise ImportError(
            f"{SUMCHECK_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C provekit_amd/csrc`). provekit_amd has no CPU fallback."
        )
    return C.CDLL(SUMCHECK_LIB_PATH)  # its libprovekit_hip.so is the one _lib has loaded (same file, found next to it)


lib = _load()
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


def _mont_limbs(value: int) -> list:
    v = value % P * _R % P
    return [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]


class Statement:
    """n variables, m tables, terms = [(coefficient, mask), ...]: the coefficient an int (taken mod p) or 4 Montgomery limbs as they
    are (which lets a test hand over a value that is not below p), the mask a bitmask of tables or a sequence of table indexes"""

    def __init__(self, n: int, m: int, terms, has_tau: bool = False, n_bind: int = 0):
        self.n, self.m, self.has_tau, self.n_bind = n, m, bool(has_tau), n_bind
        self.terms = []
        for coeff, tables in terms:
            mask = tables if isinstance(tables, int) else sum(1 << j for j in tables)
            self.terms.append((coeff, mask))

    @property
    def degree(self) -> int:
        return max(bin(mask).count("1") for _, mask in self.terms)

    def struct(self) -> StatementStruct:
        s = StatementStruct()
        s.n, s.m, s.T, s.has_tau, s.n_bind = self.n, self.m, len(self.terms), int(self.has_tau), self.n_bind
        for t, (coeff, mask) in enumerate(self.terms[:4]):
            s.masks[t] = mask
            limbs = _mont_limbs(coeff) if isinstance(coeff, int) else [int(x) for x in coeff]
            for i in range(4):
                s.coeffs[t][i] = limbs[i]
        return s


def _refused(rc: int):
    raise ProveKitHipError(rc, lib.pks_create_error().decode())


def _fe(a, rows: int, what: str):
    """[rows, 4] Montgomery limbs, or None"""
    if a is None:
        if rows:
            raise ValueError(f"{what}: {rows} elements expected")
        return None
    arr = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    if arr.shape[0] != rows:
        raise ValueError(f"{what}: {rows} elements expected, {arr.shape[0]} given")
    return arr


def _ptr(arr):
    return arr.ctypes.data if arr is not None and arr.size else None


def _ptr_array(bufs):
    return (vp * len(bufs))(*(b.ptr if isinstance(b, DeviceBuffer) else int(b) for b in bufs))


def io_pattern(stmt: Statement) -> bytes:
    """the spongefish operation list (domain separator) of a proof of this statement (pks_io_pattern; host only)"""
    s = stmt.struct()
    n = sz()
    rc = lib.pks_io_pattern(C.addressof(s), None, 0, C.byref(n))
    if rc:
        _refused(rc)
    buf = (C.c_uint8 * n.value)()
    lib.pks_io_pattern(C.addressof(s), buf, n.value, C.byref(n))
    return bytes(buf)


def proof_bytes(stmt: Statement) -> int:
    s = stmt.struct()
    n = sz()
    rc = lib.pks_proof_bytes(C.addressof(s), C.byref(n))
    if rc:
        _refused(rc)
    return n.value


def verify(stmt: Statement, proof: bytes, tau=None, bind=None, expected_sum=None, io_pattern: bytes | None = None):
    """(Result, point [n, 4], finals [m, 4]) -- Montgomery; point and finals are meaningful when the proof is accepted, and accepted means
    accepted provided f_j(point) = finals[j] (pks_verify; host only)"""
    s = stmt.struct()
    tau_a = _fe(tau, stmt.n if stmt.has_tau else 0, "tau") if (tau is not None or stmt.has_tau) else None
    bind_a = _fe(bind, stmt.n_bind, "bind") if (bind is not None or stmt.n_bind) else None
    exp_a = _fe(expected_sum, 1, "expected_sum") if expected_sum is not None else None
    point = np.zeros((stmt.n, 4), dtype=np.uint64)
    finals = np.zeros((stmt.m, 4), dtype=np.uint64)
    r = ResultStruct()
    pat = (C.c_uint8 * len(io_pattern)).from_buffer_copy(io_pattern) if io_pattern else None
    pbuf = (C.c_uint8 * max(len(proof), 1)).from_buffer_copy(bytes(proof) or b"\0")
    rc = lib.pks_verify(C.addressof(s), C.cast(pat, vp) if pat is not None else None, len(io_pattern) if io_pattern else 0, _ptr(tau_a), _ptr(bind_a),
                        _ptr(exp_a), C.cast(pbuf, vp), len(proof), point.ctypes.data, finals.ctypes.data, C.byref(r))
    if rc:
        _refused(rc)
    res = Result(bool(r.accepted), CHECKS[r.check] if 0 <= r.check < len(CHECKS) else str(r.check), int(r.offset), r.message.decode(errors="replace"))
    return res, point, finals


class Proof:
    """what Prover.prove returns: the proof bytes (s first), the challenge point [n, 4] and the final values [m, 4], Montgomery"""

    def __init__(self, data: bytes, point: np.ndarray, finals: np.ndarray):
        self.bytes, self.point, self.finals = data, point, finals

    @property
    def sum_canonical(self) -> int:
        return int.from_bytes(self.bytes[:32], "little")


class Prover:
    """one statement's prover on a context: owns one device arena sized at creation; prove() allocates no device memory and never
    writes the caller's tables"""

    _create = lib.pks_prover_create  # prodcheck_sharded.Prover: the device set's

    def __init__(self, ctx: Context, stmt: Statement):
        self.ctx, self.stmt = ctx, stmt
        s = stmt.struct()
        h = vp()
        rc = self._create(ctx.handle, C.addressof(s), C.byref(h))
        if rc:
            _refused(rc)
        self.handle = h
        self.proof_bytes = proof_bytes(stmt)

    def close(self):
        if getattr(self, "handle", None):
            lib.pks_prover_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return lib.pks_last_error(self.handle).decode()

    def prove(self, d_tables, tau=None, bind=None, capacity: int | None = None) -> Proof:
        """d_tables: m DeviceBuffers (or device addresses) of 2^n Montgomery elements.  capacity: the proof buffer's size, the proof's
        own by default"""
        return self._prove_with(lib.pks_prove, d_tables, tau, bind, capacity)

    def _prove_with(self, fn, d_tables, tau, bind, capacity) -> Proof:
        """pks_prove, or pkss_prove on a prover of a device set: each class's prove() names its own call"""
        st = self.stmt
        if len(d_tables) != st.m:
            raise ValueError(f"{st.m} tables expected")
        tau_a = _fe(tau, st.n if st.has_tau else 0, "tau") if (tau is not None or st.has_tau) else None
        bind_a = _fe(bind, st.n_bind, "bind") if (bind is not None or st.n_bind) else None
        cap = self.proof_bytes if capacity is None else capacity
        buf = (C.c_uint8 * max(cap, 1))()
        n = sz()
        point = np.zeros((st.n, 4), dtype=np.uint64)
        finals = np.zeros((st.m, 4), dtype=np.uint64)
        rc = fn(self.handle, C.cast(_ptr_array(d_tables), vp), _ptr(tau_a), _ptr(bind_a), C.cast(buf, vp), cap, C.byref(n), point.ctypes.data, finals.ctypes.data)
        self.last_len = n.value
        if rc:
            raise ProveKitHipError(rc, self.last_error())
        return Proof(bytes(buf[: n.value]), point, finals)


def _round(fn, ctx: Context, stmt: Statement, d_tables, length: int, tau_rest, fold, d_out_tables, *slice_and_grid) -> np.ndarray:
    """pks_round, or pkss_round_shard with (world, rank) in front of the grid"""
    s = stmt.struct()
    out = np.zeros((stmt.degree + 1, 4), dtype=np.uint64)
    tau_a = np.ascontiguousarray(tau_rest, dtype=np.uint64).reshape(-1, 4) if tau_rest is not None else None
    fold_a = _fe(fold, 1, "fold") if fold is not None else None
    outs = C.cast(_ptr_array(d_out_tables), vp) if d_out_tables is not None else None
    rc = fn(ctx.handle, C.addressof(s), C.cast(_ptr_array(d_tables), vp), length, tau_a.ctypes.data if tau_a is not None else None, _ptr(fold_a), outs,
            *slice_and_grid, out.ctypes.data)
    if rc:
        _refused(rc)
    return out


def round(ctx: Context, stmt: Statement, d_tables, length: int, tau_rest=None, fold=None, d_out_tables=None, grid: int = 0) -> np.ndarray:
    """[D + 1, 4] Montgomery: h(0) .. h(D) of ONE round on tables of current length `length`, folded first by `fold` into d_out_tables if
    given (pks_round).  grid = 0: the library's rule; the bits do not depend on it"""
    return _round(lib.pks_round, ctx, stmt, d_tables, length, tau_rest, fold, d_out_tables, grid)
