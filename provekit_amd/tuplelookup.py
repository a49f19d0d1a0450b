"""Tuple and multi-column LogUp-GKR lookups (libprovekit_tuplelookup.so, include/provekit_tuplelookup.h): prove that every row
(f[g][0][x], .., f[g][w-1][x]) of c groups of w device columns is a row of a table t of w columns, with multiplicities m, and verify such
proofs on the host.  A ROM read is w = 2, a binop table w = 3; c columns range-checked against one table are w = 1 and c groups.

An accepted proof is accepted PROVIDED the three values of `Claims`: whir_pcs.Scheme.open / whir_pcs.verify give the columns'
evaluations at z_lo and z_t, `check_claims` forms the three combinations.

A ninth library above the product's C ABI, with its own loader and one signature table (as provekit_amd.fracsum, whose library it
links).  `verify`, `check_claims`, the pattern and the sizes are host only; the prover and `leaves` need a Context.  A rejected proof
is a Result, not an exception; only a failed CALL raises.  There is no fallback: without the built library the import raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import fracsum  # loads libprovekit_fracsum.so (and the sumcheck library under it), which this library links
from ._lib import ProveKitHipError, sz, vp
from .prodcheck import _fe, _ptr
from .runtime import Context, DeviceBuffer
from .verify import Result, ResultStruct

TUPLELOOKUP_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libprovekit_tuplelookup.so")
MAX_VARS, MAX_BIND, MAX_WIDTH, MAX_GROUPS, MAX_GRID = 28, 16, 4, 4, 1024
CHECKS = fracsum.CHECKS
SIDES = ("F", "T")
WHICH = ("NONE", "F", "T", "M")  # check_claims
LABEL = b"provekit-hip/tuple-lookup/v1"
ERR_UNSATISFIED = -6
NO_BAD_ROW = 2**64 - 1


class StatementStruct(C.Structure):
    """pkt_statement"""

    _fields_ = [("n", C.c_uint), ("k", C.c_uint), ("w", C.c_uint), ("c", C.c_uint), ("n_bind", C.c_uint)]


class ClaimsStruct(C.Structure):
    """pkt_claims"""

    _fields_ = [("alpha", C.c_uint64 * 4), ("beta", C.c_uint64 * 4), ("z_lo", (C.c_uint64 * 4) * MAX_VARS), ("z_t", (C.c_uint64 * 4) * MAX_VARS),
                ("f_coeff", ((C.c_uint64 * 4) * MAX_WIDTH) * MAX_GROUPS), ("t_coeff", (C.c_uint64 * 4) * MAX_WIDTH), ("f_value", C.c_uint64 * 4),
                ("t_value", C.c_uint64 * 4), ("m_value", C.c_uint64 * 4)]


# name -> (restype, argtypes); kept in the same order as include/provekit_tuplelookup.h
SIGNATURES = {
    "pkt_abi_version": (C.c_int, []),
    "pkt_check_name": (C.c_char_p, [C.c_int]),
    "pkt_create_error": (C.c_char_p, []),
    "pkt_io_pattern": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
    "pkt_proof_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkt_prover_arena_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkt_count_lds_max_k": (C.c_uint, []),
    "pkt_prover_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pkt_prover_destroy": (C.c_int, [vp]),
    "pkt_last_error": (C.c_char_p, [vp]),
    "pkt_multiplicities": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(C.c_uint64)]),
    "pkt_leaves": (C.c_int, [vp, C.c_uint, C.c_uint, C.c_uint, vp, vp, vp, vp]),
    "pkt_prove": (C.c_int, [vp, vp, vp, vp, vp, vp, sz, C.POINTER(sz), vp]),
    "pkt_verify": (C.c_int, [vp, vp, sz, vp, vp, sz, vp, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(ResultStruct)]),
    "pkt_check_claims": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(C.c_int)]),
}


def _load():
    if not os.path.exists(TUPLELOOKUP_LIB_PATH):
        raise ImportError(
            f"{TUPLELOOKUP_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C provekit_amd/csrc`). provekit_amd has no CPU fallback."
        )
    return C.CDLL(TUPLELOOKUP_LIB_PATH)  # the libraries it links are the ones already loaded (same files, next to it)


lib = _load()
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


class Statement:
    """c groups of w columns of 2^n entries looked up in a table of w columns of 2^k rows; n_bind caller elements (the roots) are
    absorbed first"""

    def __init__(self, n: int, k: int, w: int = 1, c: int = 1, n_bind: int = 0):
        self.n, self.k, self.w, self.c, self.n_bind = n, k, w, c, n_bind

    def struct(self) -> StatementStruct:
        return StatementStruct(self.n, self.k, self.w, self.c, self.n_bind)


class Claims:
    """what an accepted proof is accepted PROVIDED of, Montgomery [.., 4] uint64: alpha, beta, the points z_lo [n, 4] and z_t [k, 4], the
    coefficients f_coeff [c, w, 4] = eq(z_hi, g) beta^j and t_coeff [w, 4] = beta^j, and the three required values"""

    def __init__(self, stmt: Statement, c: ClaimsStruct):
        self.struct = c
        for name in ("alpha", "beta", "f_value", "t_value", "m_value"):
            setattr(self, name, np.array(getattr(c, name), dtype=np.uint64))
        self.z_lo = np.array([list(c.z_lo[i]) for i in range(stmt.n)], dtype=np.uint64)
        self.z_t = np.array([list(c.z_t[i]) for i in range(stmt.k)], dtype=np.uint64)
        self.f_coeff = np.array([[list(c.f_coeff[g][j]) for j in range(stmt.w)] for g in range(stmt.c)], dtype=np.uint64)
        self.t_coeff = np.array([list(c.t_coeff[j]) for j in range(stmt.w)], dtype=np.uint64)


def _refused(rc: int):
    raise ProveKitHipError(rc, lib.pkt_create_error().decode())


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
    rc = lib.pkt_io_pattern(C.addressof(s), None, 0, C.byref(n))
    if rc:
        _refused(rc)
    buf = (C.c_uint8 * n.value)()
    lib.pkt_io_pattern(C.addressof(s), buf, n.value, C.byref(n))
    return bytes(buf)


def proof_bytes(stmt: Statement) -> int:
    return _sized(lib.pkt_proof_bytes, stmt)


def arena_bytes(stmt: Statement) -> int:
    """the device memory a prover of this statement holds, its two fractional-sum provers included (host only)"""
    return _sized(lib.pkt_prover_arena_bytes, stmt)


def count_lds_max_k() -> int:
    """tables of up to 2^this rows are counted in a workgroup's LDS histogram"""
    return int(lib.pkt_count_lds_max_k())


def _result(r: ResultStruct) -> Result:
    return Result(bool(r.accepted), CHECKS[r.check] if 0 <= r.check < len(CHECKS) else str(r.check), int(r.offset), r.message.decode(errors="replace"))


def _bytes_arg(b):
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


def verify(stmt: Statement, proof: bytes, bind=None, io_pattern: bytes | None = None):
    """(Result, side, layer, Claims or None): side is "F" or "T" (pkt_verify; host only)"""
    s = stmt.struct()
    bind_a = _fe(bind, stmt.n_bind, "bind") if (bind is not None or stmt.n_bind) else None
    claims, r, side, layer = ClaimsStruct(), ResultStruct(), C.c_int(0), C.c_uint(0)
    pat = _bytes_arg(io_pattern) if io_pattern else None
    pbuf = _bytes_arg(proof)
    rc = lib.pkt_verify(C.addressof(s), C.cast(pat, vp) if pat is not None else None, len(io_pattern) if io_pattern else 0, _ptr(bind_a), C.cast(pbuf, vp),
                        len(proof), C.addressof(claims), C.byref(side), C.byref(layer), C.byref(r))
    if rc:
        _refused(rc)
    res = _result(r)
    return res, SIDES[side.value], layer.value, Claims(stmt, claims) if res.accepted else None


def check_claims(stmt: Statement, claims: Claims, f_evals, t_evals, m_eval) -> str:
    """f_evals [c, w, 4], t_evals [w, 4], m_eval [4], Montgomery: the columns' evaluations at claims.z_lo and claims.z_t -> "NONE" when
    the three claims hold, else the first that does not: "F", "T" or "M" (pkt_check_claims; host only)"""
    s = stmt.struct()
    f_a = _fe(np.asarray(f_evals, dtype=np.uint64).reshape(-1, 4), stmt.c * stmt.w, "f_evals")
    t_a = _fe(np.asarray(t_evals, dtype=np.uint64).reshape(-1, 4), stmt.w, "t_evals")
    m_a = _fe(np.asarray(m_eval, dtype=np.uint64).reshape(-1, 4), 1, "m_eval")
    which = C.c_int(-1)
    rc = lib.pkt_check_claims(C.addressof(s), C.addressof(claims.struct), _ptr(f_a), _ptr(t_a), _ptr(m_a), C.byref(which))
    if rc:
        _refused(rc)
    return WHICH[which.value]


def _dev(buf):
    return None if buf is None else buf.ptr if isinstance(buf, DeviceBuffer) else int(buf)


def _pointers(bufs, count: int, what: str):
    flat = [b for row in bufs for b in (row if isinstance(row, (list, tuple)) else [row])]
    if len(flat) != count:
        raise ValueError(f"{what}: {count} device columns expected, {len(flat)} given")
    return (vp * count)(*[_dev(b) for b in flat])


def leaves(ctx: Context, n: int, w: int, c: int, d_cols, alpha, beta, d_leaf_out) -> None:
    """the leaf kernel by itself: d_leaf_out[g 2^n + x] = alpha - sum_j beta^j d_cols[g][j][x]; d_cols: c lists of w device columns of
    2^n elements (pkt_leaves)"""
    a, b = _fe(alpha, 1, "alpha"), _fe(beta, 1, "beta")
    cols = _pointers(d_cols, c * w, "d_cols")
    rc = lib.pkt_leaves(ctx.handle, n, w, c, cols, _ptr(a), _ptr(b), _dev(d_leaf_out))
    if rc:
        _refused(rc)


class Prover:
    """one statement's prover on a context: owns the two leaf tables, the counts and a fractional-sum prover per side, made at
    creation; a proof allocates no device memory and never writes the caller's tables"""

    fill = None  # a byte the proof buffer (`buffer`) is filled with before a proof, to see afterwards what a refused call wrote: nothing

    def __init__(self, ctx: Context, stmt: Statement):
        self.ctx, self.stmt = ctx, stmt
        s = stmt.struct()
        h = vp()
        rc = lib.pkt_prover_create(ctx.handle, C.addressof(s), C.byref(h))
        if rc:
            _refused(rc)
        self.handle = h
        self.proof_bytes = proof_bytes(stmt)

    def close(self):
        if getattr(self, "handle", None):
            lib.pkt_prover_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return lib.pkt_last_error(self.handle).decode()

    def _check(self, rc: int):
        if rc:
            raise ProveKitHipError(rc, self.last_error())

    def multiplicities(self, d_f, d_t, d_idx, d_m_out) -> None:
        """d_f: c lists of w device columns; d_t: w device columns; d_idx: c device columns of 2^n uint32; d_m_out: 2^k elements.  A row
        whose index is outside t or that is not the row it names raises with code -6 (PK_ERR_UNSATISFIED) and `first_bad` is the
        smallest stacked index g 2^n + x of such a row (NO_BAD_ROW otherwise)"""
        st = self.stmt
        bad = C.c_uint64(0)
        rc = lib.pkt_multiplicities(self.handle, _pointers(d_f, st.c * st.w, "d_f"), _pointers(d_t, st.w, "d_t"), _pointers(d_idx, st.c, "d_idx"), _dev(d_m_out),
                                    C.byref(bad))
        self.first_bad = bad.value
        self._check(rc)

    def prove(self, d_f, d_t, d_m, bind=None, capacity: int | None = None):
        """-> (proof bytes, Claims).  A row outside the table, a wrong m or an alpha that is a compressed row raises with code -6
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
        rc = lib.pkt_prove(self.handle, _pointers(d_f, st.c * st.w, "d_f"), _pointers(d_t, st.w, "d_t"), _dev(d_m), _ptr(bind_a), C.cast(buf, vp), cap, C.byref(n),
                           C.addressof(claims))
        self.last_len = n.value
        self._check(rc)
        return bytes(buf[: n.value]), Claims(st, claims)
