"""GPU: the committed polynomials f = [witness, zero padded || mask] and g assembled inside their first to_coeffs sweep
(csrc/mle.hip to_coeffs_generated), the statement weights added in one pass (axpy3) and the two batch combinations in one launch
(lincomb2_pair) -- each against the sequence of public calls it replaces, bit for bit, and whole proofs against the oracle's prover
(oracle/prover_ref.py) on statements whose witness length sits at the edges of the sweep's 2^11-element tile.

The whole proof at the one size whose to_coeffs takes the 10-bit high sweep (m = 21) is
test_gpu_prove.py::test_transcript_equals_the_oracle_provers_at_the_bench_size[21], which runs the same code; here that size is
compared table by table."""
import os
import sys

import numpy as np
import pytest

import mle_edge_refs as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
P = E.P
SEED = bytes((11 * i + 5) & 0xFF for i in range(32))
STREAM_MASK, STREAM_G = 1, 2  # csrc/internal.hpp RNG_MASK, RNG_G
SCALARS = {"zero": 0, "one": 1, "p-1": P - 1}  # stored values


def instance_of_length(nw, m_0):
    """a satisfiable R1CS over exactly nw witness entries (test_gpu_prove.satisfiable_r1cs; nw = 1: the one row z0 * z0 = z0)"""
    from test_gpu_prove import satisfiable_r1cs

    if nw == 1:
        one = ([0], [0], [0])
        return 1, 1, [1], [1, 2, 3, 5, P - 1, 7, P - 2, 11], (one, one, one)
    nc = min(1 << m_0, 300, nw - 1)
    got, z, coeffs, trips = satisfiable_r1cs(nc, nw - 1 - nc, 41)
    assert got == nw
    return nc, nw, z, coeffs, trips


# m = 12: to_coeffs is the 2^11 tile sweep and one high sweep; the witness half of f is exactly one tile.  m = 9: a single sweep.
@pytest.mark.parametrize("m,m_0,nw", [(12, 9, (1 << 11) - 5), (12, 9, 1 << 11), (12, 9, 1), (12, 9, (1 << 10) + 1), (9, 7, 161)])
def test_whole_proof_equals_the_oracle_provers(ctx, oracle, m, m_0, nw):
    import prover_ref as PR
    from test_gpu_prove import _vcfg, to_sparse

    from provekit_amd.scheme import WhirConfig, WhirR1CSScheme, blinding_config_for
    from provekit_amd.sparse_matrix import R1CS

    nc, nw, z, coeffs, trips = instance_of_length(nw, m_0)
    mats = []
    for rows, cols, vals in trips:
        rows = np.array(rows, dtype=np.int64)
        mats.append((np.searchsorted(rows, np.arange(nc)).astype(np.uint32), np.array(cols, dtype=np.uint32), np.array(vals, dtype=np.uint32)))
    interner = oracle.to_mont(oracle.ints_to_limbs(coeffs))
    zm = oracle.to_mont(oracle.ints_to_limbs(z))
    cfg_w, cfg_b = WhirConfig.for_size(m, 4.0), blinding_config_for(m_0, 4.0)
    r1cs = R1CS(ctx, *(to_sparse(nc, nw, t) for t in trips), interner)
    scheme = WhirR1CSScheme(ctx, r1cs, m, m_0, cfg_w, cfg_b)
    want = PR.prove(scheme.domain_separator, m, m_0, _vcfg(cfg_w), _vcfg(cfg_b), (nc, nw, mats, interner), zm, (5).to_bytes(32, "little"))
    got = scheme.prove(ctx.upload(zm), seed=5)
    assert len(got) == len(want)
    if got != want:
        first = next(i for i in range(len(got)) if got[i] != want[i])
        raise AssertionError(f"pk_prove's transcript differs from the oracle prover's from byte {first} of {len(got)}")
    scheme.close()
    r1cs.close()


# (m, n_wit): the boundary inside the first tile, at its end, one element, none, in the middle, a second witness tile; single sweeps
# (m <= 11) down to the two-element table; m = 21: the 10-bit high sweep, the bench's own shape
STAGE_CASES = [(12, (1 << 11) - 5), (12, 1 << 11), (12, 1), (12, 0), (12, (1 << 10) + 1), (13, (1 << 11) + 1), (13, 1 << 12), (1, 1), (1, 0), (2, 1),
               (9, 161), (11, 1000), (21, (1 << 20) - 5)]


@pytest.mark.parametrize("m,n_wit", STAGE_CASES)
def test_generated_tables_equal_the_unfused_sequence(ctx, m, n_wit):
    """f and g, evaluations and coefficients, against: zero, copy the witness, two draws, pk_to_coeffs_into twice"""
    from provekit_amd._lib import lib
    from provekit_amd.field import random_field
    from tools.pk_probes import lib as probes

    half, N = 1 << (m - 1), 1 << m
    wit = random_field(max(n_wit, 1), 70 + m)[:n_wit]
    if n_wit:
        wit[-1] = E.limbs([E.TOP])[0]
    d_wit = ctx.upload(wit) if n_wit else None
    junk = np.full((N, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)  # whatever the stage does not write shows
    fused = [ctx.upload(junk) for _ in range(4)]
    ctx._check(probes.pk_probe_to_coeffs_generated(ctx.handle, m, d_wit.ptr if n_wit else None, n_wit, SEED, STREAM_MASK, STREAM_G,
                                                   *(b.ptr for b in fused)))
    f = np.zeros((N, 4), dtype=np.uint64)
    f[:n_wit] = wit
    ref = [ctx.upload(f), ctx.upload(junk), ctx.upload(junk), ctx.upload(junk)]  # f, g, f's coefficients, g's
    ctx._check(lib.pk_selftest_random_fe(ctx.handle, SEED, STREAM_MASK, ref[0].ptr + 32 * half, half))
    ctx._check(lib.pk_selftest_random_fe(ctx.handle, SEED, STREAM_G, ref[1].ptr, N))
    ctx._check(lib.pk_to_coeffs_into(ctx.handle, ref[0].ptr, ref[2].ptr, m))
    ctx._check(lib.pk_to_coeffs_into(ctx.handle, ref[1].ptr, ref[3].ptr, m))
    for name, a, b in zip(("f", "g", "f's coefficients", "g's coefficients"), fused, ref):
        got, want = ctx.download_fe(a, N), ctx.download_fe(b, N)
        assert np.array_equal(got, want), (name, int(np.flatnonzero((got != want).any(axis=1))[0]))
    if n_wit:
        assert np.array_equal(ctx.download_fe(d_wit, n_wit), wit)  # the source is untouched
        d_wit.free()
    for b in fused + ref:
        b.free()


@pytest.mark.parametrize("n", [1, 255, 256, 257, (1 << 12) + 3])
def test_axpy3_equals_three_axpys(ctx, n):
    from provekit_amd._lib import lib
    from provekit_amd.field import random_field
    from tools.pk_probes import lib as probes

    stride = n + 5
    rows, y = random_field(3 * stride, 80 + n), random_field(n, 81 + n)
    rows[0], rows[stride], rows[2 * stride + n - 1], y[0] = (E.limbs([E.TOP])[0],) * 4  # the largest addends
    d_rows, d_y, d_ref = ctx.upload(rows), ctx.alloc_fe(n), ctx.alloc_fe(n)
    names = list(SCALARS)
    triples = [(a, a, a) for a in names] + [("zero", "one", "p-1"), ("p-1", "zero", "one"), ("one", "p-1", "zero")]
    for t in triples:
        g3 = E.limbs([SCALARS[k] for k in t])
        ctx.upload_into(d_y.ptr, y)
        ctx.upload_into(d_ref.ptr, y)
        ctx._check(probes.pk_probe_axpy3(ctx.handle, d_y.ptr, g3.ctypes.data, d_rows.ptr, stride, n))
        for k in range(3):
            ctx._check(lib.pk_fe_axpy(ctx.handle, d_ref.ptr, g3[k].ctypes.data, d_rows.ptr + 32 * k * stride, n))
        assert np.array_equal(ctx.download_fe(d_y, n), ctx.download_fe(d_ref, n)), (n, t)
    g3 = random_field(3, 82)
    ctx.upload_into(d_y.ptr, y)
    ctx._check(probes.pk_probe_axpy3(ctx.handle, d_y.ptr, g3.ctypes.data, d_rows.ptr, stride, n))
    want = y
    for k in range(3):
        want = E.axpy(want, E.ints(g3)[k], rows[k * stride: k * stride + n])
    assert np.array_equal(ctx.download_fe(d_y, n), want)  # ... and the Python-int definition
    assert np.array_equal(ctx.download_fe(d_rows, 3 * stride), rows)
    for b in (d_rows, d_y, d_ref):
        b.free()


@pytest.mark.parametrize("n", [1, 255, 256, 257, (1 << 12) + 3])
def test_lincomb2_pair_equals_two_lincombs(ctx, n):
    from provekit_amd.field import random_field
    from tools.pk_probes import lib as probes

    n1 = {1: 257, 257: 1}.get(n, n)  # the two combinations need not be of one length
    src = [random_field(k, 90 + i + n) for i, k in enumerate((n, n, n1, n1))]
    for s in src:
        s[-1] = E.limbs([E.TOP])[0]
    d_src = [ctx.upload(s) for s in src]
    out, ref = [ctx.alloc_fe(n), ctx.alloc_fe(n1)], [ctx.alloc_fe(n), ctx.alloc_fe(n1)]
    for name, beta in dict(SCALARS, random=E.ints(random_field(1, 91))[0]).items():
        bl = E.limbs([beta])[0]
        for o, k in zip(out + ref, (n, n1, n, n1)):
            ctx.zero(o, 32 * k)
        ctx._check(probes.pk_probe_lincomb2_pair(ctx.handle, out[0].ptr, d_src[0].ptr, d_src[1].ptr, n, out[1].ptr, d_src[2].ptr, d_src[3].ptr, n1,
                                                 bl.ctypes.data))
        ctx._check(probes.pk_probe_lincomb2(ctx.handle, ref[0].ptr, d_src[0].ptr, bl.ctypes.data, d_src[1].ptr, n))
        ctx._check(probes.pk_probe_lincomb2(ctx.handle, ref[1].ptr, d_src[2].ptr, bl.ctypes.data, d_src[3].ptr, n1))
        for o, r, k, a, b in zip(out, ref, (n, n1), src[0::2], src[1::2]):
            got = ctx.download_fe(o, k)
            assert np.array_equal(got, ctx.download_fe(r, k)) and np.array_equal(got, E.axpy(a, beta, b)), (n, name)
    for d, s in zip(d_src, src):
        assert np.array_equal(ctx.download_fe(d, len(s)), s)  # sources untouched
    for b in d_src + out + ref:
        b.free()
