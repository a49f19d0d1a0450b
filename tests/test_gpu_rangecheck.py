"""GPU: libprovekit_rangecheck.so on the device.  The fused decomposition -- limb columns and multiplicities -- bit for bit against
Python ints (tests/rangecheck_refs.py) at every plan shape, on both sides of the LDS histogram's bound and over more than one tile, for
edge values, random values, small values and full skew and for several grids, with nothing written past an output's end and the input
unchanged; a value outside the range refused with the smallest entry named, whichever word of it is set; the proof bytes and claims
against the Python reference; the top check and the limb bound reached through pkr_prove's refusals, with nothing written and the
prover usable afterwards; the arena's parts; the composition with libprovekit_whir.so; the C++ example."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import fracsum_refs as F  # noqa: E402
import prodcheck_refs as K  # noqa: E402
import rangecheck_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
P = K.P
BIND = K.random_elements(2, seed=53)
SENTINEL = 0xA5
KINDS = ("edges", "random", "small", "skew")
# (n, bits, k): every plan of the header's table; (5, 12, 12) and (5, 13, 13) on both sides of the LDS histogram's bound; the last two
# sweep more than one tile of 512 entries, under the LDS histogram and under device-memory atomics
SHAPES = [(1, 1, 1), (3, 8, 8), (4, 16, 8), (4, 5, 8), (4, 24, 8), (4, 7, 4), (5, 20, 8), (5, 32, 12), (6, 64, 16), (5, 12, 12), (5, 13, 13), (10, 20, 8), (11, 64, 16)]
PROOF_SHAPES = [(1, 1, 1), (3, 8, 8), (3, 16, 8), (2, 24, 8), (3, 7, 4), (2, 20, 8)]


def sentinel_fe(ctx, rows):
    """rows + 1 elements of sentinel bytes on the device: what a kernel does not write stays"""
    return ctx.upload(np.full((rows + 1, 4), int.from_bytes(bytes([SENTINEL]) * 8, "little"), dtype=np.uint64))


def untouched(ctx, buf, rows):
    """the element behind the end is the sentinel"""
    return ctx.download_fe(buf, rows + 1)[rows:].tobytes() == bytes([SENTINEL]) * 32


def grids_of(n):
    """1, 2, more workgroups than the column has tiles, and the library's rule"""
    from tools.pk_probes import lib as probes

    tiles = max(1, (1 << n) // (256 * probes.pk_probe_range_decompose_items()))
    return (1, 2, tiles + 3, 0)


class Outputs:
    """the L limb columns and m of a statement on the device, each with a sentinel element behind its end"""

    def __init__(self, ctx, shape):
        n, bits, k = shape
        self.ctx, self.n, self.k, self.L = ctx, n, k, R.plan(bits, k)["L"]
        self.limbs = [sentinel_fe(ctx, 1 << n) for _ in range(self.L)]
        self.m = sentinel_fe(ctx, 1 << k)

    def get(self):
        return [K.unmont(self.ctx.download_fe(b, 1 << self.n)) for b in self.limbs], K.unmont(self.ctx.download_fe(self.m, 1 << self.k))

    def past_the_end_untouched(self):
        return all(untouched(self.ctx, b, 1 << self.n) for b in self.limbs) and untouched(self.ctx, self.m, 1 << self.k)

    def free(self):
        for b in self.limbs + [self.m]:
            b.free()


@pytest.mark.parametrize("shape", SHAPES)
def test_decompose_is_the_references_bit_for_bit_for_every_input_and_grid(ctx, shape):
    from tools.pk_probes import lib as probes
    from provekit_amd import rangecheck as rc

    n, bits, k = shape
    assert rc.count_lds_max_k() == 12
    prover = rc.Prover(ctx, rc.Statement(n, bits, k))
    pl = R.plan(bits, k)
    assert (prover.plan.limbs, prover.plan.c) == (pl["L"], pl["c"])
    for kind in KINDS:
        f = R.column(n, bits, k, kind)
        if kind == "edges":
            assert all(v in f for v in R.edge_values(bits, k)[: 1 << n]) and 0 in f and (n < 2 or (1 << bits) - 1 in f) and (n < 3 or bits <= k or 1 << k in f)
        limbs, m = R.decompose(bits, k, f)
        assert sum(m) == pl["c"] << n
        if kind == "skew":
            assert max(m) >= 1 << n  # every entry of a group in one bin
        image = K.mont(f)
        d_f = ctx.upload(image)
        for grid in grids_of(n):
            assert probes.pk_probe_range_set_grid(prover.handle, grid) == 0
            out = Outputs(ctx, shape)
            prover.decompose(d_f, out.limbs, out.m)
            assert prover.first_bad == rc.NO_BAD_ENTRY
            got_limbs, got_m = out.get()
            assert got_limbs == limbs, (kind, grid)
            assert got_m == m, (kind, grid)
            assert out.past_the_end_untouched(), (kind, grid)
            out.free()
        assert ctx.download_fe(d_f, 1 << n).tobytes() == image.tobytes()  # the input is unchanged
        d_f.free()
    prover.close()


def test_the_probe_runs_the_decomposition_alone_and_states_the_grids(ctx):
    from tools.pk_probes import lib as probes

    n, bits, k = 10, 32, 12
    grids = (ctypes.c_uint * 4)()
    assert probes.pk_probe_range_grids(n, bits, k, grids) == 0 and list(grids) == [2, 1, 4, 4]
    assert probes.pk_probe_range_grids(20, 64, 16, grids) == 0 and list(grids) == [1024, 0, 64, 64]
    assert probes.pk_probe_range_grids(20, 63, 16, grids) == -1
    f = R.column(n, bits, k, "random")
    limbs, m = R.decompose(bits, k, f)
    d_f, out = ctx.upload(K.mont(f)), Outputs(ctx, (n, bits, k))
    d_counts, d_bad = ctx.upload(np.zeros(1 << k, dtype=np.uint32)), ctx.upload(np.zeros(1, dtype=np.uint64))
    ptrs = (ctypes.c_void_p * out.L)(*[b.ptr for b in out.limbs])
    for grid in (0, 3):
        ms = ctypes.c_float(-1)
        assert probes.pk_probe_range_decompose(ctx.handle, n, bits, k, d_f.ptr, ptrs, d_counts.ptr, d_bad.ptr, out.m.ptr, grid, ctypes.byref(ms)) == 0
        assert ms.value >= 0 and out.get() == (limbs, m) and out.past_the_end_untouched()
        assert int(ctx.download(d_bad, (1,), np.uint64)[0]) == 2**64 - 1
        assert ctx.download(d_counts, (1 << k,), np.uint32).tolist() == m
    for b in (d_f, d_counts, d_bad):
        b.free()
    out.free()


BAD_SHAPES = [(3, 8, 8), (5, 32, 12), (6, 64, 16), (5, 13, 13), (10, 20, 8)]
BAD_CASES = ["2^bits at entry 0", "2^bits at the last entry", "2^bits at two entries", "p - 1", "2^64", "only word 3 set"]


@pytest.mark.parametrize("where", BAD_CASES)
@pytest.mark.parametrize("shape", BAD_SHAPES)
def test_a_value_outside_the_range_is_refused_with_the_smallest_entry(ctx, shape, where):
    from provekit_amd import rangecheck as rc
    from provekit_amd._lib import ProveKitHipError

    n, bits, k = shape
    good = R.column(n, bits, k, "random", seed=3)
    f, entries = list(good), 1 << n
    if where == "2^bits at entry 0":
        f[0], want = 1 << bits, 0
    elif where == "2^bits at the last entry":
        f[entries - 1], want = 1 << bits, entries - 1
    elif where == "2^bits at two entries":
        f[entries - 1], f[entries // 2], want = 1 << bits, (1 << bits) + 7, entries // 2
    elif where == "p - 1":
        f[entries // 3], want = P - 1, entries // 3
    elif where == "2^64":
        f[1], want = 1 << 64, 1
    else:  # only word 3 set: the low 64 bits, and the low 192, are zero: inside every range if the high words were not read
        f[entries - 2], want = 1 << 192, entries - 2
    assert R.first_bad(bits, f) == want
    prover = rc.Prover(ctx, rc.Statement(n, bits, k))
    d_f, out = ctx.upload(K.mont(f)), Outputs(ctx, shape)
    with pytest.raises(ProveKitHipError, match="entry %d is not below 2\\^%d" % (want, bits)) as e:
        prover.decompose(d_f, out.limbs, out.m)
    assert e.value.code == rc.ERR_UNSATISFIED and prover.first_bad == want
    assert out.past_the_end_untouched()  # the outputs are not meaningful; nothing is written outside them
    # the prover stays usable
    ctx.upload_into(d_f.ptr, K.mont(good))
    prover.decompose(d_f, out.limbs, out.m)
    assert prover.first_bad == rc.NO_BAD_ENTRY and out.get() == R.decompose(bits, k, good)
    d_f.free()
    out.free()
    prover.close()


def test_arena_bytes_states_its_parts(ctx):
    from provekit_amd import rangecheck as rc, tuplelookup as tl

    def up(b):
        return (b + 63) // 64 * 64

    for n, bits, k in ((1, 1, 1), (9, 32, 12), (12, 64, 16), (7, 24, 8), (5, 5, 8)):
        pl = R.plan(bits, k)
        # the table 0 .. 2^k - 1; the scaled top column, only with a top check; the counts; the cell of the first bad entry
        own = up(32 << k) + (up(32 << n) if pl["r"] < k else 0) + up(4 << k) + 64
        assert rc.arena_bytes(rc.Statement(n, bits, k)) == own + tl.arena_bytes(tl.Statement(n, k, 1, pl["c"], 1))
        prover = rc.Prover(ctx, rc.Statement(n, bits, k))  # and a prover of it is made and given back
        prover.close()
    assert rc.arena_bytes(rc.Statement(9, 32, 16)) < rc.arena_bytes(rc.Statement(9, 31, 16))  # r = k: no scaled column


def same_claims(claims, ref):
    for name in ("z_lo", "z_t", "limb_coeff", "pow2"):
        assert K.unmont(getattr(claims, name)) == ref[name], name
    assert K.unmont(claims.limbs_value) == [ref["limbs_value"]] and K.unmont(claims.m_value) == [ref["m_value"]]


@pytest.mark.parametrize("shape", PROOF_SHAPES)
def test_proof_bytes_and_claims_are_the_references_and_a_prover_proves_two_columns(ctx, shape):
    from provekit_amd import rangecheck as rc
    from provekit_amd._lib import ProveKitHipError

    n, bits, k = shape
    stmt, bind = rc.Statement(n, bits, k, 2), K.mont(BIND)
    prover = rc.Prover(ctx, stmt)
    out = Outputs(ctx, shape)
    proofs = []
    for kind in ("edges", "random"):  # the same prover, two columns
        f = R.column(n, bits, k, kind, seed=len(proofs))
        limbs, m = R.decompose(bits, k, f)
        ref = R.prove(n, bits, k, limbs, m, BIND)
        d_f = ctx.upload(K.mont(f))
        prover.decompose(d_f, out.limbs, out.m)
        proof, claims = prover.prove(out.limbs, out.m, bind)
        assert proof == ref["proof"] and len(proof) == rc.proof_bytes(stmt) == prover.last_len
        same_claims(claims, ref)
        res, side, layer, seen = rc.verify(stmt, proof, bind)
        assert res.accepted and res.offset == len(proof) and (side, layer) == ("F", 0), res
        same_claims(seen, ref)
        # the three claims hold of the columns' true evaluations
        f_eval, limb_evals, m_eval = R.evaluations(f, limbs, m, ref)
        assert rc.check_claims(stmt, seen, K.mont([f_eval]), K.mont(limb_evals), K.mont([m_eval])) == "NONE"
        assert rc.check_claims(stmt, seen, K.mont([(f_eval + 1) % P]), K.mont(limb_evals), K.mont([m_eval])) == "RECOMPOSE"
        assert prover.prove(out.limbs, out.m, bind)[0] == proof  # again: the same bytes
        assert out.get() == (limbs, m) and out.past_the_end_untouched()  # the caller's columns are unchanged
        proofs.append(proof)
        d_f.free()
    assert proofs[0] != proofs[1]
    # a short buffer: the length is told, nothing is proved or written, the prover stays usable
    prover.fill = SENTINEL
    with pytest.raises(ProveKitHipError, match="the proof buffer holds") as e:
        prover.prove(out.limbs, out.m, bind, capacity=len(proof) - 1)
    assert e.value.code == -1 and prover.last_len == len(proof) and bytes(prover.buffer) == bytes([SENTINEL]) * (len(proof) - 1)
    assert prover.prove(out.limbs, out.m, bind)[0] == proof
    out.free()
    prover.close()


def test_the_top_check_and_the_limb_bound_are_really_there(ctx):
    """(4, 20, 8): three limbs of 8 bits, the top one of 4 bits, and the top check 2^4 limb_2.  Limbs that recompose the column but whose
    top limb is 2^4 -- inside the table 0 .. 2^8 - 1, outside 0 .. 2^4 - 1 -- are refused in the top-check group"""
    from provekit_amd import rangecheck as rc
    from provekit_amd._lib import ProveKitHipError

    n, bits, k = 4, 20, 8
    stmt, bind = rc.Statement(n, bits, k, 2), K.mont(BIND)
    f = R.column(n, bits, k, "edges")
    limbs, m = R.decompose(bits, k, f)
    honest_ref = R.prove(n, bits, k, limbs, m, BIND)
    prover = rc.Prover(ctx, stmt)
    prover.fill = SENTINEL
    d_m = ctx.upload(K.mont(m))
    good = [ctx.upload(K.mont(col)) for col in limbs]
    honest = prover.prove(good, d_m, bind)[0]
    assert honest == honest_ref["proof"]

    def refused(changed_limbs, changed_m, reason):
        bad = [ctx.upload(K.mont(col)) for col in changed_limbs]
        d_bad_m = ctx.upload(K.mont(changed_m))
        with pytest.raises(ProveKitHipError, match=reason) as e:
            prover.prove(bad, d_bad_m, bind)
        assert e.value.code == rc.ERR_UNSATISFIED
        assert bytes(prover.buffer) == bytes([SENTINEL]) * len(honest)  # nothing is written
        assert prover.prove(good, d_m, bind)[0] == honest  # and the same prover then proves the good columns
        for b in bad + [d_bad_m]:
            b.free()

    # entry 5 becomes 2^20 + its low 16 bits: the limbs (lo, mid, 2^4) recompose it, every limb is below 2^8
    x = 5
    top = [list(col) for col in limbs]
    top[2][x] = 1 << 4
    assert sum(top[i][x] << (k * i) for i in range(3)) == (1 << 20) + (f[x] & 0xFFFF) and all(top[i][x] < 1 << k for i in range(3))
    refused(top, m, r"entry 5 of the top-check group \(2\^4 times limb 2: the top limb must be below 2\^4\) is not in 0 \.\. 2\^8 - 1: .*a row is not in t: stacked index %d " % (3 * 16 + x))
    # a limb of 2^k, in limb 1 and in limb 0
    for i, x in ((1, 9), (0, 15)):
        wide = [list(col) for col in limbs]
        wide[i][x] = 1 << k
        refused(wide, m, r"entry %d of limb %d \(a limb must be below 2\^8\) is not in 0 \.\. 2\^8 - 1: .*a row is not in t: stacked index %d " % (x, i, 16 * i + x))
    # a wrong m
    refused(limbs, [(m[0] + 1) % P] + m[1:], "m is wrong")
    # with a spare group (4, 24, 8): limb 0 is looked up twice, and a limb 0 outside the table is named in its own group
    n, bits, k = 4, 24, 8
    f = R.column(n, bits, k, "random")
    limbs, m = R.decompose(bits, k, f)
    spare = rc.Prover(ctx, rc.Statement(n, bits, k, 2))
    wide = [list(col) for col in limbs]
    wide[0][3] = 1 << k
    bufs = [ctx.upload(K.mont(col)) for col in wide] + [ctx.upload(K.mont(m))]
    with pytest.raises(ProveKitHipError, match=r"entry 3 of limb 0 .*stacked index 3 ") as e:
        spare.prove(bufs[:3], bufs[3], bind)
    assert e.value.code == rc.ERR_UNSATISFIED
    for b in bufs + good + [d_m]:
        b.free()
    spare.close()
    prover.close()


def test_composition_with_the_commitment_scheme(ctx):
    """(6, 32, 12): commit {f, limb_0, limb_1, limb_2} as one batch and m, bind the two roots, decompose, prove, verify, open the batch at
    z_lo and m at z_t, verify the openings, check the claims on the opened values; with one evaluation changed the claims fail"""
    import whir_pcs_cases as W
    from provekit_amd import rangecheck as rc, whir_pcs

    n, bits, k = 6, 32, 12
    f = R.column(n, bits, k, "edges")
    d_f, out = ctx.upload(K.mont(f)), Outputs(ctx, (n, bits, k))
    plain = rc.Prover(ctx, rc.Statement(n, bits, k))
    plain.decompose(d_f, out.limbs, out.m)
    plain.close()
    assert out.get() == R.decompose(bits, k, f)
    cfgs = [W.small_config(n, 4), W.small_config(k, 1)]
    schemes = [whir_pcs.Scheme(ctx, cfg) for cfg in cfgs]
    coms = [schemes[0].commit([d_f] + out.limbs), schemes[1].commit([out.m])]
    bind = K.mont([int.from_bytes(com.root(), "little") for com in coms])
    stmt = rc.Statement(n, bits, k, 2)
    prover = rc.Prover(ctx, stmt)
    proof, _ = prover.prove(out.limbs, out.m, bind)
    res, side, layer, seen = rc.verify(stmt, proof, bind)
    assert res.accepted, res
    opened = []
    for scheme, cfg, com, points in zip(schemes, cfgs, coms, (seen.z_lo[None], seen.z_t[None])):
        _, opening = scheme.open(com, points)
        wres, wevals = whir_pcs.verify(cfg, points, opening, expected_root=com.root())
        assert wres.accepted, wres
        opened.append(wevals)
    cols, m_open = opened
    evs = [cols[0, 0], np.stack([cols[1, 0], cols[2, 0], cols[3, 0]]), m_open[0, 0]]
    assert rc.check_claims(stmt, seen, *evs) == "NONE"
    for which, name in ((0, "RECOMPOSE"), (2, "M")):
        changed = [x.copy() for x in evs]
        changed[which] = K.mont([(K.unmont(changed[which])[0] + 1) % P])[0]
        assert rc.check_claims(stmt, seen, *changed) == name
    changed = [x.copy() for x in evs]
    changed[1][2] = K.mont([(K.unmont(changed[1][2])[0] + 1) % P])[0]
    assert rc.check_claims(stmt, seen, *changed) == "LIMBS"
    # other roots: another seed, rejected
    assert not rc.verify(stmt, proof, K.mont([1, 2]))[0].accepted
    for closing in coms + [prover] + schemes:
        closing.close()
    d_f.free()
    out.free()


def test_the_cpp_demo_commits_proves_opens_checks_the_claims_and_sees_the_refusals():
    demo = os.path.join(ROOT, "examples", "rangecheck_pcs_demo")
    assert os.path.exists(demo), "examples/rangecheck_pcs_demo is built by __graft_entry__.build()"
    p = subprocess.run([demo], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "accepted" in p.stdout and "claims hold" in p.stdout
    assert "entry 7 is not below 2^32" in p.stdout and "top-check group" in p.stdout
