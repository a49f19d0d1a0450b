"""What the three WHIR PCS bench tools (whir_pcs_bench.py, whir_pcs_linear_bench.py, whir_pcs_sparse_bench.py) share: host wall
timing of blocking calls, and the pointer array the probes take (the device tests take `ptrs` from here too, through
tests/whir_pcs_cases.py); and HostSet, a device set over the library's host transport whose collectives the caller can see
(whir_pcs_sharded_profile.py, tests/test_gpu_whir_pcs_sharded.py).  Imports nothing of the project at module level, so it loads without a
built library."""
import ctypes as C
import statistics
import time


def timed(fn, reps):
    """warm fn once, then time it reps times -> (median, min) in seconds"""
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t)


def ab(sides, reps):
    """sides: {name: callable}; warm each once, then time them alternating -> {name: {median_ms, min_ms, spread}}"""
    for fn in sides.values():
        fn()
    t = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            t0 = time.perf_counter()
            fn()
            t[k].append(time.perf_counter() - t0)
    return {k: {"median_ms": round(1e3 * statistics.median(v), 4), "min_ms": round(1e3 * min(v), 4),
                "spread": round((max(v) - min(v)) / statistics.median(v), 3)} for k, v in t.items()}


def ptrs(bufs):
    """device buffers -> the void* array of their addresses that a probe or a C entry point takes"""
    return C.cast((C.c_void_p * len(bufs))(*(b.ptr for b in bufs)), C.c_void_p)


class HostSet:
    """G contexts on one device joined by the library's host transport (pk_comm_init_host) through a rendezvous of this process:
    what whir_pcs_sharded_profile.py and the device tests drive a device set with when they want to SEE its collectives.  `log[r]`
    lists the bytes per rank of every collective rank r made.  take_turns: a rank holds a token while it works (between `begin`
    and `end`) and hands it over while it waits in a collective, so the ranks' kernels never overlap on the one GPU and
    pk_profile_* times each rank's as if it had the chip to itself.  The project is imported here, not at module level."""

    def __init__(self, G, device=0, take_turns=False):
        import threading

        import provekit_amd
        from provekit_amd._lib import lib

        self.G, self.take_turns = G, take_turns
        self.log = [[] for _ in range(G)]
        self._slots, self._gate, self._token = [None] * G, threading.Barrier(G), threading.Lock()
        cb_type = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
        self._cbs = [cb_type(self._callback(r)) for r in range(G)]  # kept alive with the set
        self.ctxs = [provekit_amd.Context(device) for _ in range(G)]
        for r, c in enumerate(self.ctxs):
            c._check(lib.pk_comm_init_host(c.handle, G, r, self._cbs[r], None))

    def _callback(self, rank):
        def cb(_user, send, recv, nbytes):  # the library has drained the rank's stream before it calls
            self.log[rank].append(int(nbytes))
            self._slots[rank] = C.string_at(send, nbytes)
            if self.take_turns:
                self._token.release()
            try:
                self._gate.wait()
                C.memmove(recv, b"".join(self._slots), self.G * nbytes)
                self._gate.wait()
            except Exception:  # a broken barrier: another rank left
                return 1
            finally:
                if self.take_turns:
                    self._token.acquire()
            return 0

        return cb

    def begin(self, rank):
        if self.take_turns:
            self._token.acquire()

    def end(self, rank):
        if self.take_turns:
            self.ctxs[rank].sync()
            self._token.release()

    def close(self):
        for c in self.ctxs:
            c.close()
