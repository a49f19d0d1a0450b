"""What the three WHIR PCS bench tools (whir_pcs_bench.py, whir_pcs_linear_bench.py, whir_pcs_sparse_bench.py) share: host wall
timing of blocking calls, and the pointer array the probes take (the device tests take `ptrs` from here too, through
tests/whir_pcs_cases.py).  Imports nothing of the project, so it loads without a built library."""
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
