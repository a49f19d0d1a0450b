"""ProofEngine: many proofs in flight from one caller thread (libprovekit_engine.so, include/provekit_engine.h).

The engine is a second library above the product's C ABI: it owns K provers ("lanes": a pk_ctx, a pk_scheme and an arena each), one
worker thread per lane and a job queue.  One Python thread hands it a list of (witness, seed) jobs and gets the proofs back; which
lane ran a job never shows in its proof.  This module has its own loader and signature table (provekit_amd._lib's table is the
product header's, nothing else).  There is no fallback: without the built library the import raises, without a GPU the constructor
does."""
from __future__ import annotations

import ctypes as C
import os

from . import _lib
from ._lib import ProveKitHipError, sz, vp
from .runtime import DeviceBuffer
from .scheme import WhirConfig, WhirR1CSScheme, _cfg_struct

ENGINE_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libprovekit_engine.so")

PKE_MAX_LANES = 32
PKE_AUTO_LANES_MAX = 16
PKE_ERR_CANCELLED = -100
PKE_KEEP_HOST_WAIT = 1
PKE_NO_JOB = (1 << 64) - 1

_u64 = C.c_uint64

# name -> (restype, argtypes); kept in the same order as include/provekit_engine.h
SIGNATURES = {
    "pke_engine_create": (C.c_int, [C.c_int, vp, sz, sz, C.c_uint, C.c_uint, vp, vp, C.c_uint, C.c_uint, C.POINTER(vp)]),
    "pke_create_error": (C.c_char_p, []),
    "pke_engine_destroy": (C.c_int, [vp]),
    "pke_engine_lanes": (C.c_int, [vp]),
    "pke_engine_set_io_pattern": (C.c_int, [vp, vp, sz]),
    "pke_engine_set_hash_version": (C.c_int, [vp, C.c_int]),
    "pke_engine_set_witness_builders": (C.c_int, [vp, vp, sz, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]),
    "pke_engine_domain_separator": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
    "pke_submit": (C.c_int, [vp, vp, sz, vp, vp, sz, C.POINTER(sz), C.POINTER(C.c_int), C.POINTER(_u64)]),
    "pke_noir_submit": (C.c_int, [vp, vp, sz, vp, sz, vp, vp, sz, C.POINTER(sz), C.POINTER(C.c_int), C.POINTER(_u64)]),
    "pke_wait": (C.c_int, [vp, _u64]),
    "pke_wait_all": (C.c_int, [vp]),
    "pke_prove_many": (C.c_int, [vp, sz, vp, vp, vp, vp, vp, vp, vp, C.POINTER(_u64)]),
    "pke_noir_prove_many": (C.c_int, [vp, sz, vp, vp, vp, sz, vp, vp, vp, vp, vp, C.POINTER(_u64)]),
    "pke_engine_last_error": (C.c_char_p, [vp, _u64]),
}


def _load():
    if not os.path.exists(ENGINE_LIB_PATH):
        raise ImportError(
            f"{ENGINE_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C provekit_amd/csrc`). provekit_amd has no CPU fallback."
        )
    return C.CDLL(ENGINE_LIB_PATH)  # its libprovekit_hip.so is the one _lib has loaded (same file, found next to it)


lib = _load()
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


def _ptr(d) -> int:
    return d.ptr if isinstance(d, DeviceBuffer) else d


class Job:
    """one submitted proof (pke_submit): wait() returns the proof bytes or raises what pk_prove reported.  The buffers a lane
    writes (transcript, length, status) belong to this object, so the ENGINE holds it until the job is final -- dropping the
    result of submit() is harmless."""

    def __init__(self, engine: "ProofEngine", cap: int, keep):
        self._engine, self._keep = engine, keep  # keep: the witness / seed objects, alive until the job is final
        self._buf = (C.c_uint8 * cap)()
        self._len, self._status, self._ticket = sz(), C.c_int(), _u64()
        self._final = False

    @property
    def ticket(self) -> int:
        return self._ticket.value

    def _finalise(self):
        """the job is final (waited for, or the engine is idle or gone): nothing writes into this object any more"""
        self._final, self._keep = True, None
        self._engine._outstanding.pop(self._ticket.value, None)

    def wait(self) -> bytes:
        e = self._engine
        if not self._final:
            if e.handle is not None:
                lib.pke_wait(e.handle, self._ticket.value)  # after close() every job is final already
            self._finalise()
        self.status = self._status.value
        if self.status != 0:
            raise ProveKitHipError(self.status, e.last_error(self._ticket.value) or f"job {self._ticket.value} failed")
        return C.string_at(self._buf, self._len.value)


class ProofEngine:
    """`lanes` provers of one scheme on one GPU behind a job queue.  lanes=0 lets the library pick (at most 16, by free device
    memory).  r1cs: provekit_amd.sparse_matrix.R1CS, uploaded once by the caller and closed after the engine.
    set_host_wait=False leaves the device's host-wait mode alone (default: the engine selects the polling wait)."""

    def __init__(self, r1cs, m: int, m_0: int, whir_witness: WhirConfig, whir_for_hiding_spartan: WhirConfig, lanes: int = 0, device: int = 0,
                 set_host_wait: bool = True, cap: int = 4 << 20):
        self.handle = None
        self._outstanding = {}  # ticket -> Job, from submit() until the job is final: a lane writes into the Job's buffers
        n = C.c_int(0)
        rc = _lib.lib.pk_device_count(C.byref(n))
        if rc != 0 or n.value <= 0:
            raise ProveKitHipError(rc or -5, "no HIP device visible; provekit_amd has no CPU fallback")
        if not 0 <= lanes <= PKE_MAX_LANES:
            raise ProveKitHipError(-1, f"lanes must be 0 (pick) .. {PKE_MAX_LANES}")
        self.r1cs, self.m, self.m_0, self.cap = r1cs, m, m_0, int(cap)
        self.whir_witness, self.whir_for_hiding_spartan = whir_witness, whir_for_hiding_spartan
        cw, cb = _cfg_struct(whir_witness), _cfg_struct(whir_for_hiding_spartan)
        h = vp()
        rc = lib.pke_engine_create(device, r1cs.handle, r1cs.num_constraints, r1cs.num_witnesses, m, m_0, C.byref(cw), C.byref(cb), lanes,
                                   0 if set_host_wait else PKE_KEEP_HOST_WAIT, C.byref(h))
        if rc != 0:
            raise ProveKitHipError(rc, (lib.pke_create_error() or b"").decode() or "pke_engine_create failed")
        self.handle = h.value
        self.lanes = lib.pke_engine_lanes(self.handle)
        self.builders = None

    # -- life cycle ---------------------------------------------------------------------------------------------------
    def close(self):
        """pke_engine_destroy: jobs still queued are cancelled (PKE_ERR_CANCELLED), running ones finish, the lanes go"""
        if self.handle is not None:
            lib.pke_engine_destroy(self.handle)  # returns with every job final
            self.handle = None
        for job in list(self._outstanding.values()):
            job._finalise()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self, ticket: int = PKE_NO_JOB) -> str:
        if self.handle is None:
            return ""
        return (lib.pke_engine_last_error(self.handle, ticket) or b"").decode()

    def _check(self, rc: int):
        if rc != 0:
            raise ProveKitHipError(rc, self.last_error())

    # -- settings, forwarded to every lane ----------------------------------------------------------------------------
    @property
    def domain_separator(self) -> bytes:
        n = sz()
        lib.pke_engine_domain_separator(self.handle, None, 0, C.byref(n))
        ds = C.create_string_buffer(n.value)
        lib.pke_engine_domain_separator(self.handle, ds, n.value, C.byref(n))
        return ds.raw[: n.value]

    def set_io_pattern(self, pattern: bytes | None):
        """WhirR1CSScheme.set_io_pattern on every lane (None restores the library's restatement)"""
        pattern = pattern or b""
        self._check(lib.pke_engine_set_io_pattern(self.handle, pattern if pattern else None, len(pattern)))

    def set_hash_version(self, version: int):
        self._check(lib.pke_engine_set_hash_version(self.handle, version))

    def set_witness_builders(self, builders_or_bytes):
        """the builder list noir_prove_many runs: a list of provekit_amd.witness.WitnessBuilder tuples or its postcard bytes"""
        from .witness import encode_witness_builders

        if builders_or_bytes is None:
            data = b""
        else:
            data = bytes(builders_or_bytes) if isinstance(builders_or_bytes, (bytes, bytearray)) else encode_witness_builders(builders_or_bytes)
        nw, nch, nac = sz(), sz(), sz()
        self._check(lib.pke_engine_set_witness_builders(self.handle, data if data else None, len(data), C.byref(nw), C.byref(nch), C.byref(nac)))
        self.builders = {"n_witnesses": nw.value, "n_challenges": nch.value, "n_acir": nac.value} if data else None

    # -- proving ------------------------------------------------------------------------------------------------------
    def submit(self, d_witness, seed=None, n_witness: int | None = None, cap: int | None = None) -> Job:
        """queue one proof and return at once; Job.wait() gives the bytes.  seed as WhirR1CSScheme.prove's (None in production)."""
        s = WhirR1CSScheme._seed_arg(seed)
        job = Job(self, self.cap if cap is None else cap, (d_witness, s))
        nw = self.r1cs.num_witnesses if n_witness is None else n_witness
        self._check(lib.pke_submit(self.handle, _ptr(d_witness), nw, s, job._buf, len(job._buf), C.byref(job._len), C.byref(job._status),
                                   C.byref(job._ticket)))
        self._outstanding[job.ticket] = job  # queued: from here on the job's buffers must outlive the caller's interest in it
        return job

    def wait_all(self):
        """pke_wait_all: every job submitted so far is final when it returns (their results stay with their Job objects)"""
        waited = list(self._outstanding.values())  # submitted before the call: final after it
        self._check(lib.pke_wait_all(self.handle))
        for job in waited:
            job._finalise()

    def _many(self, call, inputs, n_in, seeds, cap):
        n = len(inputs)
        seeds = [None] * n if seeds is None else list(seeds)
        if len(seeds) != n or len(n_in) != n or len(cap) != n:
            raise ValueError("one seed, one length and one capacity per job")
        keep = [WhirR1CSScheme._seed_arg(s) for s in seeds]
        bufs = [(C.c_uint8 * c)() for c in cap]
        d_in = (vp * max(n, 1))(*[_ptr(d) for d in inputs])
        cnt = (sz * max(n, 1))(*n_in)
        sd = (vp * max(n, 1))(*[C.addressof(s) if s is not None else None for s in keep])
        out = (vp * max(n, 1))(*[C.addressof(b) for b in bufs])
        caps = (sz * max(n, 1))(*cap)
        lens, status, first = (sz * max(n, 1))(), (C.c_int * max(n, 1))(), _u64()
        rc = call(n, d_in, cnt, sd, out, caps, lens, status, C.byref(first))
        self.last_status = list(status[:n])
        self.last_first_ticket = first.value
        return rc, [C.string_at(bufs[i], lens[i]) if status[i] == 0 else None for i in range(n)]

    def prove_many(self, witnesses, seeds=None, n_witness=None, cap=None, raise_on_error: bool = True) -> list:
        """pke_prove_many: one proof per entry of `witnesses` (DeviceBuffers or device pointers; entries may repeat), blocking, from
        this thread.  -> the proofs in job order.  A failed job raises ProveKitHipError naming it -- or, with raise_on_error=False,
        leaves None in its slot; self.last_status has every job's code either way.  n_witness / cap: per-job overrides (lists)."""
        n = len(witnesses)
        n_in = [self.r1cs.num_witnesses] * n if n_witness is None else list(n_witness)
        cap = [self.cap] * n if cap is None else list(cap)

        def call(n, d_in, cnt, sd, out, caps, lens, status, first):
            return lib.pke_prove_many(self.handle, n, d_in, cnt, sd, out, caps, lens, status, first)

        rc, proofs = self._many(call, witnesses, n_in, seeds, cap)
        self._raise(rc, raise_on_error)
        return proofs

    def noir_prove_many(self, acir_maps, n_acir: int, public_acir_idx=(), seeds=None, raise_on_error: bool = True) -> list:
        """pke_noir_prove_many: WhirR1CSScheme.noir_prove per dense ACIR witness map (device), with the builders of set_witness_builders"""
        import numpy as np

        idx = np.ascontiguousarray(public_acir_idx, dtype=np.uint32)
        n = len(acir_maps)

        def call(n, d_in, cnt, sd, out, caps, lens, status, first):
            return lib.pke_noir_prove_many(self.handle, n, d_in, cnt, idx.ctypes.data if len(idx) else None, len(idx), sd, out, caps, lens, status, first)

        rc, proofs = self._many(call, acir_maps, [n_acir] * n, seeds, [self.cap] * n)
        self._raise(rc, raise_on_error)
        return proofs

    def _raise(self, rc, raise_on_error):
        if rc != 0 and raise_on_error:
            i = next(k for k, s in enumerate(self.last_status) if s != 0)
            raise ProveKitHipError(self.last_status[i], f"job {i}: " + (self.last_error(self.last_first_ticket + i) or "failed"))
