"""ctypes binding of tools/libpk_probes.so (tools/probes/pk_probes.h): measurement probes and rejected prototypes -- the lab, kept
out of the product library.  Built by `make -C tools/probes` (also by __graft_entry__.build()).  Used by
bench.py for the measured multiplier peak (roofline.alu.peak), by tests/test_gpu_selftest.py and by the tools/ scripts."""
from __future__ import annotations

import ctypes as C
import os

from provekit_amd._lib import lib as _product  # noqa: F401  (libpk_probes.so links against libprovekit_hip.so: load that first)
from provekit_amd._lib import sz, u32p, u64p, u8p, vp  # noqa: F401

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libpk_probes.so")
if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} is missing: build it with `make -C tools/probes`")
lib = C.CDLL(LIB_PATH)

SIGNATURES = {
    "pk_probe_arith_device": (C.c_int, [vp, C.c_int, vp, vp, vp, sz]),
    "pk_probe_inv30_device": (C.c_int, [vp, C.c_int, vp, vp, sz]),
    "pk_probe_modmul_rate": (C.c_int, [vp, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_double)]),
    "pk_probe_sq_round_rate": (C.c_int, [vp, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_double)]),
    "pk_probe_fp52_sqr": (C.c_int, [vp, vp, sz]),
    "pk_probe_coop_round": (C.c_int, [vp, vp, vp, C.c_uint, vp, vp]),
    "pk_probe_fp52_sqr_device": (C.c_int, [vp, vp, vp, sz]),
    "pk_probe_modmul_rate_fp52": (C.c_int, [vp, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_double)]),
    "pk_probe_constmul_rate": (C.c_int, [vp, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.POINTER(C.c_double)]),
    "pk_probe_roundtrip": (C.c_int, [vp, C.c_uint, C.c_uint, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pk_probe_launch_chain": (C.c_int, [vp, C.c_uint, C.c_uint, C.POINTER(C.c_double)]),
    "pk_probe_mfma_reduce": (C.c_int, [vp, vp, vp, sz]),
    "pk_probe_mfma_reduce_rate": (C.c_int, [vp, C.c_uint, C.c_uint, C.POINTER(C.c_double)]),
    "pk_probe_mfma_valu_rate": (C.c_int, [vp, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_double)]),
    # the leaf hash of a caller-built hash-ready codeword and the encoding's stated range, for tests/test_gpu_scaled_codeword.py
    "pk_probe_leaf_hash_scaled": (C.c_int, [vp, vp, sz, sz, vp]),
    "pk_probe_scaled32_bounds": (C.c_int, [vp, vp]),
    # csrc/mle.hip's entry points without a C ABI (csrc/internal.hpp), for tests/test_gpu_mle_edges.py
    "pk_probe_num_cus": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "pk_probe_reduction_blocks": (C.c_int, [vp, sz, C.POINTER(C.c_uint)]),
    "pk_probe_dot_rows": (C.c_int, [vp, vp, sz, C.c_uint, vp, vp, sz, vp]),
    "pk_probe_eval_univariate_multi": (C.c_int, [vp, vp, C.c_uint, sz, vp, vp]),
    "pk_probe_lincomb2": (C.c_int, [vp, vp, vp, vp, vp, sz]),
    "pk_probe_fold_pairs2": (C.c_int, [vp, vp, vp, vp, vp, sz, vp]),
    "pk_probe_sumcheck_cubic_launch": (C.c_int, [vp, vp, vp, vp, vp, sz, vp, C.POINTER(C.c_uint)]),
    "pk_probe_sumcheck_quadratic_launch": (C.c_int, [vp, vp, vp, sz, vp, vp, vp, C.POINTER(C.c_uint)]),
    "pk_probe_sumcheck_collect_spin": (C.c_int, [vp, C.c_uint, vp]),
    # ... and the fused steps of the commit and of WhirProver::start, for tests/test_gpu_commit_fused.py
    "pk_probe_lincomb2_pair": (C.c_int, [vp, vp, vp, vp, sz, vp, vp, vp, sz, vp]),
    "pk_probe_axpy3": (C.c_int, [vp, vp, vp, vp, sz, sz]),
    "pk_probe_to_coeffs_generated": (C.c_int, [vp, C.c_uint, vp, sz, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]),
    # ... and the fused steps of the WHIR opening, for tests/test_gpu_opening_fused.py
    "pk_probe_opening_first": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_uint, vp, vp, C.c_uint, C.c_int, vp, sz, C.c_uint, sz, vp, C.c_int, C.c_uint, vp]),
    "pk_probe_dot_rows_eq": (C.c_int, [vp, vp, sz, C.c_uint, vp, C.c_uint, sz, vp]),
    # libprovekit_whir.so's linear-statement kernels where its C ABI does not reach (tools/probes/whir_linear.hip)
    "pk_probe_whir_combine": (C.c_int, [vp, vp, sz, vp, vp, C.c_uint, C.c_int]),
    "pk_probe_whir_weighted_sums": (C.c_int, [vp, vp, C.c_uint, C.c_uint, vp, C.c_uint, C.c_uint, C.c_int, vp]),
    "pk_probe_whir_wsum_grid": (C.c_uint, [C.c_uint]),
    "pk_probe_wsum_tile_host": (C.c_int, [vp, vp, C.c_uint, vp]),
    # ... and the rank slices of its two reductions with the finish kernel over gathered blocks, on one context
    "pk_probe_whir_eval_grid": (C.c_uint, [C.c_uint]),
    "pk_probe_whir_eval_slice": (C.c_int, [vp, vp, C.c_uint, C.c_uint, vp, C.c_uint, C.c_uint, C.c_uint, vp, C.POINTER(C.c_float)]),
    "pk_probe_whir_wsum_slice": (C.c_int, [vp, vp, C.c_uint, C.c_uint, vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int, vp, C.POINTER(C.c_float)]),
    "pk_probe_whir_finish": (C.c_int, [vp, vp, sz, C.c_uint, C.c_uint, sz, C.c_uint, C.c_uint, C.c_uint, vp]),
    # ... and its sparse-weight code (tools/probes/whir_sparse.hip)
    "pk_probe_whir_sparse_threads": (C.c_uint, []),
    "pk_probe_whir_sparse_chunk_bits": (C.c_uint, []),
    "pk_probe_whir_sparse_grid": (C.c_uint, [C.c_uint, sz, C.c_uint]),
    "pk_probe_whir_sparse_sums": (C.c_int, [vp, vp, C.c_uint, C.c_uint, vp, vp, vp, C.c_uint, C.c_uint, vp]),
    "pk_probe_sparse_tile_host": (C.c_int, [vp, vp, C.c_uint, vp]),
    "pk_probe_sparse_eq_host": (C.c_int, [C.c_uint, vp, vp, vp, sz, vp]),
    # ... and its hiding stage (tools/probes/whir_hiding.hip)
    "pk_probe_whir_hiding_fill": (C.c_int, [vp, vp, C.c_uint, C.c_uint, vp, C.c_uint]),
    "pk_probe_whir_hiding_grid": (C.c_uint, [C.c_uint, C.c_uint]),
    "pk_probe_whir_hiding_threads": (C.c_uint, []),
    "pk_probe_whir_hiding_pairs_per_lane": (C.c_uint, []),
    # either of libprovekit_lookup.so's two gather kernels by itself (tools/probes/lookup.hip);
    "pk_probe_lookup_gather": (C.c_int, [vp, vp, vp, vp, C.c_uint, C.c_uint, vp, vp, C.c_int, C.c_uint, C.POINTER(C.c_float)]),
    # a pkl_prover's grid and the phases of its last proof
    "pk_probe_lookup_set_grid": (C.c_int, [vp, C.c_uint]),
    "pk_probe_lookup_profile": (C.c_int, [vp, C.POINTER(C.c_double)]),
    # libprovekit_grandproduct.so's tree and leaf kernels with their layers per launch and grid (tools/probes/grandproduct.hip);
    "pk_probe_grandproduct_tree": (C.c_int, [vp, C.c_uint, vp, vp, C.c_uint, C.c_uint, C.POINTER(C.c_float)]),
    "pk_probe_grandproduct_leaf_tree": (C.c_int, [vp, C.c_uint, C.c_uint, vp, vp, vp, vp, vp, C.c_uint, C.c_uint, C.POINTER(C.c_float)]),
    "pk_probe_grandproduct_default_layers": (C.c_uint, []),
    # a pkg_prover's two knobs and the phases of its last proof; the pkg_prover inside a multiset prover
    "pk_probe_grandproduct_set_knobs": (C.c_int, [vp, C.c_uint, C.c_uint]),
    "pk_probe_grandproduct_profile": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pk_probe_multiset_inner": (vp, [vp]),
    # libprovekit_fracsum.so's tree, lookup-leaf and combine kernels with their layers per launch and grid (tools/probes/fracsum.hip);
    "pk_probe_fracsum_tree": (C.c_int, [vp, C.c_uint, vp, vp, vp, vp, C.c_uint, C.c_uint, C.POINTER(C.c_float)]),
    "pk_probe_fracsum_lookup_leaf": (C.c_int, [vp, C.c_uint, vp, vp, vp, vp, vp, vp, C.c_uint, C.c_uint, C.POINTER(C.c_float)]),
    "pk_probe_fracsum_combine": (C.c_int, [vp, sz, vp, vp, vp, vp, C.c_uint, C.POINTER(C.c_float)]),
    "pk_probe_fracsum_default_layers": (C.c_uint, []),
    # a pkf_prover's two knobs and the phases of its last proof; the pkf_prover of a lookup prover's side
    "pk_probe_fracsum_set_knobs": (C.c_int, [vp, C.c_uint, C.c_uint]),
    "pk_probe_fracsum_profile": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pk_probe_fracsum_lookup_side": (vp, [vp, C.c_int]),
    # libprovekit_tuplelookup.so's leaf kernel with its grid; a pkt_prover's grid knob and the phases of its last calls (tools/probes/tuplelookup.hip)
    "pk_probe_tuple_leaves": (C.c_int, [vp, C.c_uint, C.c_uint, C.c_uint, vp, vp, vp, vp, C.c_uint, C.POINTER(C.c_float)]),
    "pk_probe_tuple_set_grid": (C.c_int, [vp, C.c_uint]),
    "pk_probe_tuple_profile": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pk_probe_tuple_leaf_items": (C.c_uint, []),
    # libprovekit_memcheck.so's two leaf kernels with their grid; a pkm_prover's grid knob and the phases of its last calls (tools/probes/memcheck.hip)
    "pk_probe_mem_leaves": (C.c_int, [vp, C.c_uint, C.c_uint, vp, vp, vp, vp, vp, vp, C.c_uint, C.POINTER(C.c_float)]),
    "pk_probe_mem_set_grid": (C.c_int, [vp, C.c_uint]),
    "pk_probe_mem_profile": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pk_probe_mem_leaf_items": (C.c_uint, []),
    "pk_probe_mem_trace_items": (C.c_uint, []),
    "pk_probe_mem_count_lds_max_n": (C.c_uint, []),
    # libprovekit_spark.so's gather kernel with its grid; a pkx_prover's grid knob and the phases of its last calls (tools/probes/spark.hip)
    "pk_probe_spark_gather": (C.c_int, [vp, C.c_uint, C.c_uint, C.c_uint, vp, vp, vp, vp, vp, vp, vp, C.c_uint, C.POINTER(C.c_float)]),
    "pk_probe_spark_set_grid": (C.c_int, [vp, C.c_uint]),
    "pk_probe_spark_profile": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pk_probe_spark_gather_items": (C.c_uint, []),
    "pk_probe_spark_matrix_items": (C.c_uint, []),
    # libprovekit_rangecheck.so's decomposition pass with its grid; a pkr_prover's grid knob, the phases of its last calls and the
    # grid of each kernel (tools/probes/rangecheck.hip)
    "pk_probe_range_decompose": (C.c_int, [vp, C.c_uint, C.c_uint, C.c_uint, vp, vp, vp, vp, vp, C.c_uint, C.POINTER(C.c_float)]),
    "pk_probe_range_set_grid": (C.c_int, [vp, C.c_uint]),
    "pk_probe_range_profile": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pk_probe_range_grids": (C.c_int, [C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_uint)]),
    "pk_probe_range_decompose_items": (C.c_uint, []),
    # libprovekit_bitwise.so's decomposition pass with its grid; a pkb_prover's grid knob, the phases of its last calls and the grid
    # of each kernel (tools/probes/bitwise.hip)
    "pk_probe_bitwise_decompose": (C.c_int, [vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_uint, C.POINTER(C.c_float)]),
    "pk_probe_bitwise_set_grid": (C.c_int, [vp, C.c_uint]),
    "pk_probe_bitwise_profile": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pk_probe_bitwise_grids": (C.c_int, [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_uint)]),
    "pk_probe_bitwise_decompose_items": (C.c_uint, []),
    # csrc/witness.hip's thresholds and the shape of a levelled builder list (tools/probes/witness.hip): host only
    "pk_probe_witness_narrow": (C.c_uint, []),
    "pk_probe_witness_sum_heavy": (C.c_uint, []),
    "pk_probe_witness_sum_chunk": (C.c_uint, []),
    "pk_probe_witness_n_ops": (C.c_uint, []),
    "pk_probe_witness_phases": (C.c_int, [C.c_char_p, sz, vp, vp, vp, sz, C.POINTER(C.c_size_t), C.c_char_p, sz]),
    # csrc/r1cs.hip's thresholds, its two sharded entry points and fe29.hpp's dot29 on the host (tools/probes/r1cs.hip)
    "pk_probe_r1cs_heavy_degree": (C.c_uint, []),
    "pk_probe_r1cs_heavy_chunk": (C.c_uint, []),
    "pk_probe_dot29_group": (C.c_uint, []),
    "pk_probe_reduction_threads": (C.c_uint, []),
    "pk_probe_r1cs_witness_bounds_strided": (C.c_int, [vp, vp, vp, C.c_uint, C.c_uint, C.c_uint, vp, vp, vp]),
    "pk_probe_r1cs_external_row_range": (C.c_int, [vp, vp, vp, sz, sz, vp]),
    "pk_probe_dot29_host": (C.c_int, [vp, vp, C.c_uint, vp]),
}
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args


def r1cs_thresholds() -> dict:
    """csrc/r1cs_shape.hpp, fe29.hpp and reduce.hpp: the line length above which a line is summed by workgroups, the entries per
    workgroup of such a line, the products per Montgomery reduction of a line's dot product, the lanes that stride a chunk"""
    return {"HEAVY_DEGREE": lib.pk_probe_r1cs_heavy_degree(), "HEAVY_CHUNK": lib.pk_probe_r1cs_heavy_chunk(),
            "DOT29_GROUP": lib.pk_probe_dot29_group(), "RED_THREADS": lib.pk_probe_reduction_threads()}


def dot29_host(a, b):
    """sum_t a[t] * b[t] * 2^-256 mod p by fe29.hpp's dot29 on the host; a, b: (terms, 4) u64 arrays -> (4,) u64"""
    import numpy as np

    a, b = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4) for x in (a, b))
    assert a.shape == b.shape
    out = np.empty(4, dtype=np.uint64)
    rc = lib.pk_probe_dot29_host(a.ctypes.data if len(a) else None, b.ctypes.data if len(b) else None, len(a), out.ctypes.data)
    if rc:
        raise ValueError(f"pk_probe_dot29_host: {rc}")
    return out


def witness_thresholds() -> dict:
    """csrc/witness_shape.hpp: the phase width up to which phases share a one-workgroup launch, the Sum length above which a sum is
    summed by workgroups, and the terms per workgroup of such a sum"""
    return {"NARROW": lib.pk_probe_witness_narrow(), "SUM_HEAVY": lib.pk_probe_witness_sum_heavy(), "SUM_CHUNK": lib.pk_probe_witness_sum_chunk()}


def witness_phases(data: bytes) -> dict:
    """postcard(Vec<WitnessBuilder>) after levelling (two phases per level): `widths[ph]` items per phase, `ops[ph]` items per phase
    and variant (csrc/witness.hip's OP_* order), `blocks_before[ph]` Spice blocks and long sums that run right before the phase.
    Raises ValueError with the library's reason for a list it refuses."""
    n, err = C.c_size_t(), C.create_string_buffer(512)
    rc = lib.pk_probe_witness_phases(data, len(data), None, None, None, 0, C.byref(n), err, 512)
    if rc:
        raise ValueError(err.value.decode() or f"pk_probe_witness_phases: {rc}")
    n_ops, cap = lib.pk_probe_witness_n_ops(), max(n.value, 1)
    w, ops, blocks = (C.c_uint32 * cap)(), (C.c_uint32 * (cap * n_ops))(), (C.c_uint32 * cap)()
    rc = lib.pk_probe_witness_phases(data, len(data), w, ops, blocks, cap, C.byref(n), err, 512)
    if rc:
        raise ValueError(err.value.decode() or f"pk_probe_witness_phases: {rc}")
    return {"widths": list(w[: n.value]), "ops": [list(ops[ph * n_ops : (ph + 1) * n_ops]) for ph in range(n.value)],
            "blocks_before": list(blocks[: n.value])}
