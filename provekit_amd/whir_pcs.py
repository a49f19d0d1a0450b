"""WHIR as a polynomial commitment scheme (libprovekit_whir.so, include/provekit_whir.h): commit to up to 4 multilinear
polynomials, open them at points of the caller's choice -- or at LINEAR statements <w, f> = s over dense weight tables
(open_linear / verify_linear; the caller's tags bind the weights), or over the same weights as sparse index/value lists
(open_sparse / verify_sparse; SparseWeights) -- and verify the opening.  Those openings are PLAIN WHIR, not hiding; commit_hiding / open_hiding / verify_hiding mask the
polynomials as pk_prove masks its witness (include/provekit_whir_hiding.h states the construction and what it claims).

A Scheme on a context of a device set (Context.create_set, comm_init_rank, device_set.py) works as on a lone context: one Scheme per
rank, one thread per rank, the same calls with the same inputs on every rank, the lone scheme's root and proof bytes on every rank
(include/provekit_whir.h, "Device sets").

A fourth library above the product's C ABI, with its own loader and one signature table for its four headers (as provekit_amd.verify).  `verify` and
`io_pattern` are host only; `Scheme` needs a Context.  A rejected proof is a Result, not an exception; only a failed CALL raises.
There is no fallback: without the built library the import raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._lib import ProveKitHipError, sz, vp
from .runtime import Context, DeviceBuffer
from .scheme import WhirConfig, _cfg_struct
from .verify import CHECKS as WALK_CHECKS
from .verify import Result, ResultStruct

WHIR_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libprovekit_whir.so")
MAX_POINTS = 64
MAX_WEIGHTS = 16
CHECKS = WALK_CHECKS + ("POINTS", "ROOT", "DEFERRED")

HIDING_LABEL = b"provekit-hip/whir-pcs-hiding/v1"

# name -> (restype, argtypes); kept in the same order as the headers: include/provekit_whir.h, ...
SIGNATURES = {
    "pkw_abi_version": (C.c_int, []),
    "pkw_check_name": (C.c_char_p, [C.c_int]),
    "pkw_create_error": (C.c_char_p, []),
    "pkw_scheme_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pkw_scheme_destroy": (C.c_int, [vp]),
    "pkw_scheme_arena_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkw_last_error": (C.c_char_p, [vp]),
    "pkw_io_pattern": (C.c_int, [vp, C.c_uint, vp, sz, C.POINTER(sz)]),
    "pkw_commit": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pkw_commitment_root": (C.c_int, [vp, vp]),
    "pkw_commitment_destroy": (C.c_int, [vp]),
    "pkw_evaluate": (C.c_int, [vp, vp, C.c_uint, C.c_uint, vp, C.c_uint, vp]),
    "pkw_evaluate_low_vars": (C.c_uint, []),
    "pkw_open": (C.c_int, [vp, vp, vp, C.c_uint, vp, vp, sz, C.POINTER(sz)]),
    "pkw_verify": (C.c_int, [vp, vp, sz, C.c_int, vp, vp, C.c_uint, vp, sz, vp, C.POINTER(ResultStruct)]),
    # ... provekit_whir_linear.h: linear statements over dense weight tables
    "pkw_weighted_sums": (C.c_int, [vp, vp, C.c_uint, C.c_uint, vp, C.c_uint, vp]),
    "pkw_io_pattern_linear": (C.c_int, [vp, C.c_uint, C.c_uint, vp, sz, C.POINTER(sz)]),
    "pkw_open_linear": (C.c_int, [vp, vp, vp, C.c_uint, vp, vp, C.c_uint, vp, vp, vp, sz, C.POINTER(sz)]),
    "pkw_verify_linear": (C.c_int, [vp, vp, sz, C.c_int, vp, vp, C.c_uint, vp, vp, C.c_uint, vp, sz, vp, vp, vp, vp, C.POINTER(C.c_uint),
                                    C.POINTER(ResultStruct)]),
    # ... provekit_whir_sparse.h: the same statements over index/value lists
    "pkw_sparse_sums": (C.c_int, [vp, vp, C.c_uint, C.c_uint, vp, vp, vp, C.c_uint, vp]),
    "pkw_sparse_accumulate": (C.c_int, [vp, vp, C.c_uint, vp, vp, vp, C.c_uint, vp]),
    "pkw_sparse_evaluate": (C.c_int, [vp, C.c_uint, vp, vp, vp, C.c_uint, vp, vp]),
    "pkw_open_sparse": (C.c_int, [vp, vp, vp, C.c_uint, vp, vp, vp, vp, C.c_uint, vp, vp, vp, sz, C.POINTER(sz)]),
    "pkw_verify_sparse": (C.c_int, [vp, vp, sz, C.c_int, vp, vp, C.c_uint, vp, vp, vp, vp, C.c_uint, vp, sz, vp, vp, vp, vp, C.POINTER(ResultStruct)]),
    # ... provekit_whir_hiding.h: hiding commitments
    "pkw_hiding_scheme_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pkw_io_pattern_hiding": (C.c_int, [vp, C.c_uint, vp, sz, C.POINTER(sz)]),
    "pkw_commit_hiding": (C.c_int, [vp, vp, vp, C.POINTER(vp)]),
    "pkw_hiding_commitment_root": (C.c_int, [vp, vp]),
    "pkw_hiding_commitment_destroy": (C.c_int, [vp]),
    "pkw_open_hiding": (C.c_int, [vp, vp, vp, C.c_uint, vp, vp, sz, C.POINTER(sz)]),
    "pkw_verify_hiding": (C.c_int, [vp, vp, sz, C.c_int, vp, vp, C.c_uint, vp, sz, vp, C.POINTER(ResultStruct)]),
}


def _load():
    if not os.path.exists(WHIR_LIB_PATH):
        raise ImportError(
            f"{WHIR_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C provekit_amd/csrc`). provekit_amd has no CPU fallback."
        )
    return C.CDLL(WHIR_LIB_PATH)  # its libprovekit_hip.so is the one _lib has loaded (same file, found next to it)


lib = _load()
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


def _result(r: ResultStruct) -> Result:
    return Result(bool(r.accepted), CHECKS[r.check] if 0 <= r.check < len(CHECKS) else str(r.check), int(r.offset), r.message.decode(errors="replace"))


def _points(points, n_vars: int) -> np.ndarray:
    """[q, n_vars, 4] Montgomery limbs; variable 0 <-> the most significant index bit"""
    p = np.ascontiguousarray(points, dtype=np.uint64)
    if p.ndim != 3 or p.shape[1:] != (n_vars, 4) or p.shape[0] < 1:
        raise ValueError(f"points must have shape [q, {n_vars}, 4]")
    return p


def _points_or_none(points, n_vars: int) -> np.ndarray:
    """a linear statement may have no points: None or an empty sequence -> [0, n_vars, 4]"""
    if points is None or len(points) == 0:
        return np.zeros((0, n_vars, 4), dtype=np.uint64)
    return _points(points, n_vars)


def _tags(tags) -> np.ndarray:
    t = np.ascontiguousarray(tags, dtype=np.uint64)
    if t.ndim != 2 or t.shape[1] != 4:
        raise ValueError("tags must have shape [l, 4]")
    return t


def _ptr_array(bufs):
    return (vp * len(bufs))(*(b.ptr if isinstance(b, DeviceBuffer) else int(b) for b in bufs))


def low_vars() -> int:
    """the evaluation kernel's tile: 2^low_vars contiguous evaluations per workgroup step"""
    return int(lib.pkw_evaluate_low_vars())


def _io_pattern(fn, cfg: WhirConfig, *counts) -> bytes:
    """a pattern entry point called twice: for the length, then into a buffer of that length"""
    c = _cfg_struct(cfg)
    n = sz()
    rc = fn(C.addressof(c), *counts, None, 0, C.byref(n))
    if rc:
        raise ProveKitHipError(rc, lib.pkw_create_error().decode())
    buf = (C.c_uint8 * n.value)()
    fn(C.addressof(c), *counts, buf, n.value, C.byref(n))
    return bytes(buf)


def io_pattern(cfg: WhirConfig, q: int) -> bytes:
    """the spongefish operation list (domain separator) of a proof that opens q points (pkw_io_pattern; host only)"""
    return _io_pattern(lib.pkw_io_pattern, cfg, q)


def io_pattern_linear(cfg: WhirConfig, q: int, l: int) -> bytes:
    """the operation list of a proof that opens q points and l dense weights (pkw_io_pattern_linear; host only)"""
    return _io_pattern(lib.pkw_io_pattern_linear, cfg, q, l)


def io_pattern_hiding(cfg: WhirConfig, q: int) -> bytes:
    """the operation list of a hiding proof that opens q points: io_pattern(cfg, q)'s operations under HIDING_LABEL
    (pkw_io_pattern_hiding; host only; cfg describes the extended batch and must keep the two hiding rules)"""
    return _io_pattern(lib.pkw_io_pattern_hiding, cfg, q)


def arena_bytes(cfg: WhirConfig) -> int:
    c = _cfg_struct(cfg)
    n = sz()
    rc = lib.pkw_scheme_arena_bytes(C.addressof(c), C.byref(n))
    if rc:
        raise ProveKitHipError(rc, lib.pkw_create_error().decode())
    return n.value


def evaluate(ctx: Context, d_evals, n_vars: int, points) -> np.ndarray:
    """[batch, q, 4] Montgomery: the MLE of every polynomial (device buffers of 2^n_vars evaluations) at every point, each
    polynomial read once per 8 points (pkw_evaluate)"""
    p = _points(points, n_vars)
    out = np.zeros((len(d_evals), p.shape[0], 4), dtype=np.uint64)
    ctx._check(lib.pkw_evaluate(ctx.handle, C.cast(_ptr_array(d_evals), vp), len(d_evals), n_vars, p.ctypes.data, p.shape[0], out.ctypes.data))
    return out


def weighted_sums(ctx: Context, d_evals, n_vars: int, d_weights) -> np.ndarray:
    """[batch, l, 4] Montgomery: <w_i, f_b> = sum_x w_i[x] f_b[x] for device buffers of 2^n_vars elements, a 2 x 2 tile of them (1 x 4 for one polynomial) per
    pass over memory (pkw_weighted_sums)"""
    out = np.zeros((len(d_evals), len(d_weights), 4), dtype=np.uint64)
    ctx._check(lib.pkw_weighted_sums(ctx.handle, C.cast(_ptr_array(d_evals), vp), len(d_evals), n_vars, C.cast(_ptr_array(d_weights), vp),
                              len(d_weights), out.ctypes.data))
    return out


class LinearResult:
    """what pkw_verify_linear hands back next to the verdict.  `unchecked` weights had no table: the verdict then holds PROVIDED
    deferred[i] is the multilinear extension of weight i at fold_point"""

    def __init__(self, result, evals, sums, fold_point, deferred, unchecked):
        self.result, self.evals, self.sums, self.fold_point, self.deferred, self.unchecked = result, evals, sums, fold_point, deferred, unchecked


def _verify(fn, cfg: WhirConfig, p: np.ndarray, statement: tuple, l: int, proof, expected_root, io_pattern, hash_version, outputs: int) -> LinearResult:
    """One verification call: fn(config, pattern, hash version, root, points, q, *statement, proof, evaluations, ..., result).  statement:
    what the entry point takes between q and the proof; outputs: how many of (sums, fold point, deferred, unchecked) it hands back"""
    c = _cfg_struct(cfg)
    q = p.shape[0]
    proof = bytes(proof)
    evals = np.zeros((cfg.batch_size, q, 4), dtype=np.uint64)
    sums = np.zeros((cfg.batch_size, l, 4), dtype=np.uint64)
    fold = np.zeros((cfg.n_vars, 4), dtype=np.uint64)
    deferred = np.zeros((max(l, 1), 4), dtype=np.uint64)
    unchecked = C.c_uint(0)
    r = ResultStruct()
    pat = bytes(io_pattern) if io_pattern else None
    root = bytes(expected_root) if expected_root is not None else None
    if root is not None and len(root) != 32:
        raise ValueError("a root is 32 bytes")
    outs = (sums.ctypes.data, fold.ctypes.data, deferred.ctypes.data, C.byref(unchecked))[:outputs]
    rc = fn(C.addressof(c), pat, len(pat) if pat else 0, hash_version, root, p.ctypes.data if q else None, q, *statement, proof, len(proof),
            evals.ctypes.data if q else None, *outs, C.byref(r))
    if rc:
        raise ProveKitHipError(rc, lib.pkw_create_error().decode())
    return LinearResult(_result(r), evals, sums, fold, deferred[:l], unchecked.value)


def verify_linear(cfg: WhirConfig, points, tags, weights, proof: bytes, expected_root: bytes | None = None, io_pattern: bytes | None = None,
                  hash_version: int = 2) -> LinearResult:
    """Host only (pkw_verify_linear).  weights: None, or a list of l entries, each None or a HOST table [2^n_vars, 4] (Montgomery)"""
    p = _points_or_none(points, cfg.n_vars)
    t = _tags(tags)
    l = t.shape[0]
    tables = None
    if weights is not None:
        if len(weights) != l:
            raise ValueError("as many weights as tags")
        keep = [None if w is None else np.ascontiguousarray(w, dtype=np.uint64) for w in weights]
        for w in keep:
            if w is not None and w.shape != (1 << cfg.n_vars, 4):
                raise ValueError(f"a weight table has shape [{1 << cfg.n_vars}, 4]")
        tables = (vp * max(l, 1))(*(None if w is None else w.ctypes.data for w in keep))
    statement = (t.ctypes.data, C.cast(tables, vp) if tables is not None else None, l)
    return _verify(lib.pkw_verify_linear, cfg, p, statement, l, proof, expected_root, io_pattern, hash_version, outputs=4)


class SparseWeights:
    """l weights as index/value lists (include/provekit_whir_sparse.h): offsets [l + 1] uint64, index [nnz] uint32 -- strictly
    increasing within a weight, each < 2^n_vars -- and value [nnz, 4] Montgomery limbs.  Built from one (indexes, values) pair per
    weight; nothing is checked here, the library refuses what breaks the rules.  `upload` puts index and value on the device"""

    def __init__(self, weights=(), offsets=None, index=None, value=None):
        if offsets is None:
            offsets = np.cumsum([0] + [len(i) for i, _ in weights], dtype=np.uint64)
            index = np.concatenate([np.asarray(i, dtype=np.uint32).reshape(-1) for i, _ in weights] + [np.zeros(0, dtype=np.uint32)])
            value = np.concatenate([np.asarray(v, dtype=np.uint64).reshape(-1, 4) for _, v in weights] + [np.zeros((0, 4), dtype=np.uint64)])
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.index = np.ascontiguousarray(index, dtype=np.uint32)
        self.value = np.ascontiguousarray(value, dtype=np.uint64).reshape(-1, 4)
        self.l = len(self.offsets) - 1
        self.d_index = self.d_value = None

    def upload(self, ctx: Context) -> "SparseWeights":
        self.free()
        if len(self.index):
            self.d_index, self.d_value = ctx.upload(self.index), ctx.upload(self.value)
        return self

    def free(self):
        for b in (self.d_index, self.d_value):
            if b is not None:
                b.free()
        self.d_index = self.d_value = None

    def _device(self):
        """(offsets, index, value) pointers for a device entry point"""
        if len(self.index) and self.d_index is None:
            raise ValueError("upload the lists first")
        return self.offsets.ctypes.data, self.d_index.ptr if self.d_index else None, self.d_value.ptr if self.d_value else None

    def _host(self):
        return self.offsets.ctypes.data, self.index.ctypes.data if len(self.index) else None, self.value.ctypes.data if len(self.value) else None


def _sparse_check(ctx: Context, rc: int):
    """a refusal of the three pk_ctx entry points carries its reason in pkw_create_error; any other failure is the context's"""
    if rc == -1:
        raise ProveKitHipError(rc, lib.pkw_create_error().decode())
    ctx._check(rc)


def sparse_sums(ctx: Context, d_evals, n_vars: int, weights: SparseWeights) -> np.ndarray:
    """[batch, l, 4] Montgomery: sum_k value_i[k] * f_b[index_i[k]], weighted_sums on the densified tables from nnz gathers (pkw_sparse_sums)"""
    out = np.zeros((len(d_evals), max(weights.l, 1), 4), dtype=np.uint64)
    _sparse_check(ctx, lib.pkw_sparse_sums(ctx.handle, C.cast(_ptr_array(d_evals), vp), len(d_evals), n_vars, *weights._device(), weights.l,
                                           out.ctypes.data))
    return out[:, : weights.l]


def sparse_accumulate(ctx: Context, d_table, n_vars: int, weights: SparseWeights, scales) -> None:
    """d_table[index_i[k]] += scales[i] * value_i[k] in place; scales [l, 4] Montgomery on the host (pkw_sparse_accumulate)"""
    s = np.ascontiguousarray(scales, dtype=np.uint64).reshape(-1, 4)
    if s.shape[0] != weights.l:
        raise ValueError("as many scales as weights")
    _sparse_check(ctx, lib.pkw_sparse_accumulate(ctx.handle, d_table.ptr if isinstance(d_table, DeviceBuffer) else int(d_table), n_vars,
                                                 *weights._device(), weights.l, s.ctypes.data if weights.l else None))


def sparse_evaluate(ctx: Context, n_vars: int, weights: SparseWeights, point) -> np.ndarray:
    """[l, 4] Montgomery: the multilinear extension of every weight at `point` [n_vars, 4], no dense table anywhere (pkw_sparse_evaluate)"""
    p = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 4)
    if p.shape[0] != n_vars:
        raise ValueError(f"a point has {n_vars} coordinates")
    out = np.zeros((max(weights.l, 1), 4), dtype=np.uint64)
    _sparse_check(ctx, lib.pkw_sparse_evaluate(ctx.handle, n_vars, *weights._device(), weights.l, p.ctypes.data if n_vars else None, out.ctypes.data))
    return out[: weights.l]


def verify_sparse(cfg: WhirConfig, points, tags, weights: SparseWeights, proof: bytes, expected_root: bytes | None = None,
                  io_pattern: bytes | None = None, hash_version: int = 2) -> LinearResult:
    """Host only (pkw_verify_sparse): every weight's deferred relation is judged from its entries, so `unchecked` is always 0"""
    p = _points_or_none(points, cfg.n_vars)
    t = _tags(tags)
    l = t.shape[0]
    if weights.l != l:
        raise ValueError("as many weights as tags")
    return _verify(lib.pkw_verify_sparse, cfg, p, (t.ctypes.data, *weights._host(), l), l, proof, expected_root, io_pattern, hash_version, outputs=3)


def verify(cfg: WhirConfig, points, proof: bytes, expected_root: bytes | None = None, io_pattern: bytes | None = None, hash_version: int = 2):
    """-> (Result, evaluations [batch, q, 4] Montgomery as the proof binds them).  Host only (pkw_verify)."""
    v = _verify(lib.pkw_verify, cfg, _points(points, cfg.n_vars), (), 0, proof, expected_root, io_pattern, hash_version, outputs=0)
    return v.result, v.evals


def verify_hiding(cfg: WhirConfig, points, proof: bytes, expected_root: bytes | None = None, io_pattern: bytes | None = None, hash_version: int = 2):
    """-> (Result, evaluations [batch_size - 1, q, 4] Montgomery: f_b(z_i) as the proof binds them).  points: [q, n_vars - 1, 4], the
    verifier prefixes each with 0.  Host only (pkw_verify_hiding)."""
    p = _points(points, cfg.n_vars - 1)
    v = _verify(lib.pkw_verify_hiding, cfg, p, (), 0, proof, expected_root, io_pattern, hash_version, outputs=0)
    return v.result, _first_rows(v.evals, cfg.batch_size - 1)


def _first_rows(evals: np.ndarray, rows: int) -> np.ndarray:
    """a hiding entry point fills rows * q elements of a [batch, q, 4] buffer, contiguously"""
    q = evals.shape[1]
    return evals.reshape(-1, 4)[: rows * q].reshape(rows, q, 4).copy()


class HidingCommitment:
    """What pkw_commit_hiding keeps: the commitment to (f^_0 .. f^_{B-1}, g).  It is opened ONCE."""

    def __init__(self, scheme: "Scheme", handle: int):
        self.scheme, self.handle = scheme, handle

    def root(self) -> bytes:
        buf = (C.c_uint8 * 32)()
        self.scheme._check(lib.pkw_hiding_commitment_root(self.handle, buf))
        return bytes(buf)

    def close(self):
        if self.handle is not None and self.scheme.handle is not None:
            lib.pkw_hiding_commitment_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Commitment:
    """What pkw_commit keeps: both forms of the polynomials, the codeword and its tree.  Open it any number of times."""

    def __init__(self, scheme: "Scheme", handle: int):
        self.scheme, self.handle = scheme, handle

    def root(self) -> bytes:
        buf = (C.c_uint8 * 32)()
        self.scheme._check(lib.pkw_commitment_root(self.handle, buf))
        return bytes(buf)

    def close(self):
        if self.handle is not None and self.scheme.handle is not None:
            lib.pkw_commitment_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scheme:
    """One WhirConfig (batch_size polynomials of n_vars variables) bound to a Context, with a device arena sized once."""

    def __init__(self, ctx: Context, cfg: WhirConfig, hiding: bool = False):
        """hiding: cfg describes the extended batch of hiding commitments, and must keep their two rules (pkw_hiding_scheme_create)"""
        self.handle = None
        self.ctx, self.cfg = ctx, cfg
        c = _cfg_struct(cfg)
        h = vp()
        rc = (lib.pkw_hiding_scheme_create if hiding else lib.pkw_scheme_create)(ctx.handle, C.addressof(c), C.byref(h))
        if rc:
            raise ProveKitHipError(rc, lib.pkw_create_error().decode())
        self.handle = h.value
        self._buf = None

    def _check(self, rc):
        if rc:
            raise ProveKitHipError(rc, lib.pkw_last_error(self.handle).decode())

    def commit(self, d_evals) -> Commitment:
        """d_evals: batch_size device buffers of 2^n_vars evaluations over the hypercube (Montgomery); they are copied"""
        if len(d_evals) != self.cfg.batch_size:
            raise ValueError(f"expected {self.cfg.batch_size} polynomials")
        h = vp()
        self._check(lib.pkw_commit(self.handle, C.cast(_ptr_array(d_evals), vp), C.byref(h)))
        return Commitment(self, h.value)

    def _open(self, fn, commitment: Commitment, p: np.ndarray, statement, l: int, cap):
        """One opening call: fn(scheme, commitment, points, q, *statement, evaluations[, sums], proof buffer, cap, length).  statement: what
        the entry point takes between q and the outputs, None for pkw_open, which has no sums either.  Without `cap` the proof goes
        into a buffer of 8 MiB the scheme keeps"""
        q = p.shape[0]
        evals = np.zeros((self.cfg.batch_size, q, 4), dtype=np.uint64)
        sums = np.zeros((self.cfg.batch_size, max(l, 1), 4), dtype=np.uint64)
        if cap is None:
            if self._buf is None:
                self._buf = (C.c_uint8 * (8 << 20))()
            buf = self._buf
        else:
            buf = (C.c_uint8 * max(cap, 1))()
        n = sz()
        outs = (evals.ctypes.data if q else None,) + (() if statement is None else (sums.ctypes.data,))
        self._check(fn(self.handle, commitment.handle, p.ctypes.data if q else None, q, *(statement or ()), *outs, buf, len(buf) if cap is None else cap,
                       C.byref(n)))
        return evals, sums[:, :l], C.string_at(buf, n.value)

    def open(self, commitment: Commitment, points, cap: int | None = None):
        """-> (evaluations [batch, q, 4] Montgomery, proof bytes)"""
        evals, _, proof = self._open(lib.pkw_open, commitment, _points(points, self.cfg.n_vars), None, 0, cap)
        return evals, proof

    def open_linear(self, commitment: Commitment, points, d_weights, tags, cap: int | None = None):
        """open at q >= 0 points and l >= 1 dense weights (device buffers of 2^n_vars elements) bound by `tags` [l, 4]
        -> (evaluations [batch, q, 4], sums [batch, l, 4], proof bytes)"""
        p = _points_or_none(points, self.cfg.n_vars)
        t = _tags(tags)
        l = t.shape[0]
        if len(d_weights) != l:
            raise ValueError("as many weights as tags")
        statement = (C.cast(_ptr_array(d_weights), vp) if l else None, t.ctypes.data, l)
        return self._open(lib.pkw_open_linear, commitment, p, statement, l, cap)

    def open_sparse(self, commitment: Commitment, points, weights: SparseWeights, tags, cap: int | None = None):
        """open_linear with the l weights as uploaded index/value lists: the same statement, the same bytes (pkw_open_sparse)
        -> (evaluations [batch, q, 4], sums [batch, l, 4], proof bytes)"""
        p = _points_or_none(points, self.cfg.n_vars)
        t = _tags(tags)
        l = t.shape[0]
        if weights.l != l:
            raise ValueError("as many weights as tags")
        return self._open(lib.pkw_open_sparse, commitment, p, (*weights._device(), t.ctypes.data, l), l, cap)

    def commit_hiding(self, d_evals, seed: bytes | None = None) -> HidingCommitment:
        """d_evals: batch_size - 1 device buffers of 2^(n_vars - 1) evaluations; they are copied.  seed: 32 bytes, a TEST HOOK --
        None draws the key of the masks and g from the OS (pkw_commit_hiding)"""
        if len(d_evals) != self.cfg.batch_size - 1:
            raise ValueError(f"expected {self.cfg.batch_size - 1} polynomials")
        if seed is not None and len(seed) != 32:
            raise ValueError("a seed is 32 bytes")
        h = vp()
        self._check(lib.pkw_commit_hiding(self.handle, C.cast(_ptr_array(d_evals), vp), seed, C.byref(h)))
        return HidingCommitment(self, h.value)

    def open_hiding(self, commitment: HidingCommitment, points, cap: int | None = None):
        """points: [q, n_vars - 1, 4] -> (evaluations [batch_size - 1, q, 4] Montgomery, proof bytes); once per commitment"""
        evals, _, proof = self._open(lib.pkw_open_hiding, commitment, _points(points, self.cfg.n_vars - 1), None, 0, cap)
        return _first_rows(evals, self.cfg.batch_size - 1), proof

    def close(self):
        if self.handle is not None and self.ctx.handle is not None:
            lib.pkw_scheme_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
