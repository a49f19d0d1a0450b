"""GPU: libprovekit_sumcheck.so on the device.  pks_prove's bytes against the Python reference (tests/prodcheck_refs.py) for every shape
at the sizes where the round kernel changes behaviour; edge values; the round's bits across grids; the caller's tables untouched; a
prover reused; a short proof buffer; the composition with libprovekit_whir.so; one large size against the product's own sums."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import prodcheck_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu
P = K.P

# fewer pairs than lanes (1, 2); the pair count crossing one 256-lane workgroup (8, 9, 10); several workgroups (13); a grid whose
# partials the finish kernel takes several per lane is the round test's (grid 300), 16 is the library's own rule at 64 workgroups
SIZES = [1, 2, 8, 9, 10, 13, 16]


@functools.lru_cache(maxsize=None)
def reference(name, n):
    """computed once per (shape, size) and shared: (shape, tables, tau, bind, proof, point, finals, s)"""
    shape = K.Shape(name, n, n_bind=1)
    tables = K.random_tables(shape.m, n, seed=100 * n + len(name))
    tau = K.random_elements(n, seed=n) if shape.has_tau else None
    bind = K.random_elements(1, seed=3)
    return (shape, tables, tau, bind) + K.prove(shape, tables, tau, bind)


def upload(ctx, tables):
    return [ctx.upload(K.mont(t)) for t in tables]


def run(ctx, shape, tables, tau, bind):
    from provekit_amd import prodcheck

    d = upload(ctx, tables)
    prover = prodcheck.Prover(ctx, shape.statement())
    try:
        return prover.prove(d, K.mont(tau) if tau is not None else None, K.mont(bind) if shape.n_bind else None)
    finally:
        prover.close()
        for b in d:
            b.free()


def check_against(ctx, shape, tables, tau, bind):
    from provekit_amd import prodcheck

    want, point, finals, s = K.prove(shape, tables, tau, bind)
    got = run(ctx, shape, tables, tau, bind)
    assert got.bytes == want and K.unmont(got.point) == point and K.unmont(got.finals) == finals and got.sum_canonical == s
    res, vpoint, vfinals = prodcheck.verify(shape.statement(), got.bytes, K.mont(tau) if tau is not None else None,
                                            K.mont(bind) if shape.n_bind else None, K.mont([s]))
    assert res.accepted and np.array_equal(vpoint, got.point) and np.array_equal(vfinals, got.finals), res
    return s


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_the_provers_bytes_are_the_references_and_are_accepted(ctx, name, n):
    from provekit_amd import prodcheck

    shape, tables, tau, bind, want, point, finals, s = reference(name, n)
    got = run(ctx, shape, tables, tau, bind)
    assert len(got.bytes) == shape.proof_bytes() and got.sum_canonical == s
    assert got.bytes == want
    assert K.unmont(got.point) == point and K.unmont(got.finals) == finals
    res, vpoint, vfinals = prodcheck.verify(shape.statement(), got.bytes, K.mont(tau) if tau is not None else None, K.mont(bind), K.mont([s]))
    assert res.accepted and res.check == "NONE" and res.offset == len(want), res
    assert np.array_equal(vpoint, got.point) and np.array_equal(vfinals, got.finals)


@pytest.mark.parametrize("name", ["inner", "r1cs", "four"])
def test_edge_values_all_zero_and_all_p_minus_one(ctx, name):
    n = 9
    shape = K.Shape(name, n)
    tau = K.random_elements(n, seed=1) if shape.has_tau else None
    assert check_against(ctx, shape, [[0] * (1 << n)] * shape.m, tau, ()) == 0
    check_against(ctx, shape, [[P - 1] * (1 << n)] * shape.m, [P - 1] * n if shape.has_tau else None, ())


@pytest.mark.parametrize("name", ["r1cs", "eval", "mixed"])
def test_edge_values_tau_with_coordinates_0_1_and_p_minus_one(ctx, name):
    n = 9
    shape = K.Shape(name, n)
    tables = K.random_tables(shape.m, n, seed=5)
    for tau in ([0, 1, P - 1] * 3, [1] * n, [0] * n, [P - 1, 0, 0, 1, 1, P - 1, 5, 0, 1]):
        check_against(ctx, shape, tables, tau, ())


def test_edge_values_a_statement_whose_sum_is_zero(ctx):
    n = 9
    shape = K.Shape("r1cs", n)
    a, b = K.random_tables(2, n, seed=11)
    c = [x * y % P for x, y in zip(a, b)]
    assert check_against(ctx, shape, [a, b, c], K.random_elements(n, seed=12), ()) == 0


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("name", ["r1cs", "triple", "four"])
def test_the_rounds_bits_do_not_depend_on_the_grid(ctx, name, fold):
    """pks_round at n = 13 on grids 1, 2, 7, 300 (more partials than the finish kernel has lanes; most workgroups idle) and the library's
    own: the same bits, and with a fold the same folded tables; the library's grid also against the reference's round values"""
    from provekit_amd import prodcheck

    n = 13
    shape, tables, tau, bind, proof, point, _, _ = reference(name, n)
    stmt = shape.statement()
    d = upload(ctx, tables)
    N = 1 << n
    outs = [ctx.alloc_fe(N // 2) for _ in range(shape.m)] if fold else None
    tau_rest = K.mont(tau[2:] if fold else tau[1:]) if tau is not None else None
    seen, folded = [], []
    for grid in (0, 1, 2, 7, 300):
        h = prodcheck.round(ctx, stmt, d, N, tau_rest, K.mont([point[0]]) if fold else None, outs, grid)
        seen.append(h.tobytes())
        if fold:
            folded.append(b"".join(ctx.download_fe(o.ptr, N // 2).tobytes() for o in outs))
            for o in outs:
                ctx.zero(o.ptr, 32 * (N // 2))
    assert len(set(seen)) == 1 and len(set(folded)) <= 1
    i = 1 if fold else 0  # the round this call is in the reference's proof
    at = 32 * (1 + i * (shape.D + 1))
    want = [int.from_bytes(proof[at + 32 * k : at + 32 * k + 32], "little") for k in range(shape.D + 1)]
    assert K.unmont(np.frombuffer(seen[0], dtype=np.uint64)) == want
    if fold:
        r = point[0]
        got = K.unmont(np.frombuffer(folded[0], dtype=np.uint64))
        assert got == [(t[x] + r * (t[x + N // 2] - t[x])) % P for t in tables for x in range(N // 2)]
    for b in d + (outs or []):
        b.free()


def test_the_callers_tables_are_unchanged_and_a_prover_proves_again_the_same(ctx):
    from provekit_amd import prodcheck

    shape, tables, tau, bind, want, _, _, _ = reference("r1cs", 10)
    images = [K.mont(t) for t in tables]
    d = [ctx.upload(im) for im in images]
    prover = prodcheck.Prover(ctx, shape.statement())
    first = prover.prove(d, K.mont(tau), K.mont(bind))
    for im, b in zip(images, d):
        assert np.array_equal(ctx.download_fe(b.ptr, 1 << 10).reshape(-1, 4), im)
    second = prover.prove(d, K.mont(tau), K.mont(bind))
    assert first.bytes == second.bytes == want
    assert np.array_equal(first.point, second.point) and np.array_equal(first.finals, second.finals)
    prover.close()
    for b in d:
        b.free()


def test_a_short_proof_buffer_is_refused_with_the_length_and_the_prover_stays_usable(ctx):
    from provekit_amd import prodcheck
    from provekit_amd._lib import ProveKitHipError

    shape, tables, tau, bind, want, _, _, _ = reference("mixed", 8)
    d = upload(ctx, tables)
    prover = prodcheck.Prover(ctx, shape.statement())
    for cap in (0, len(want) - 1):
        with pytest.raises(ProveKitHipError, match="proof buffer") as e:
            prover.prove(d, K.mont(tau), K.mont(bind), capacity=cap)
        assert e.value.code == -1 and prover.last_len == len(want)
    assert prover.prove(d, K.mont(tau), K.mont(bind)).bytes == want
    assert prover.prove(d, K.mont(tau), K.mont(bind), capacity=len(want) + 100).bytes == want
    prover.close()
    for b in d:
        b.free()


def test_composition_with_the_commitment_scheme(ctx):
    """commit a, b, c; prove eq (a b - c) = s with the root bound; open the commitment at the sumcheck's point; both verifiers accept and
    the opening's evaluations are the sumcheck's final values.  Under another root the sumcheck proof is rejected"""
    import whir_pcs_cases as W
    from provekit_amd import prodcheck, whir_pcs

    n = 10
    shape = K.Shape("r1cs", n, n_bind=1)
    tables = K.random_tables(3, n, seed=21)
    tau = K.random_elements(n, seed=22)
    d = upload(ctx, tables)
    cfg = W.small_config(n, 3)
    scheme = whir_pcs.Scheme(ctx, cfg)
    com = scheme.commit(d)
    root = com.root()
    bind = K.mont([int.from_bytes(root, "little")])
    prover = prodcheck.Prover(ctx, shape.statement())
    proof = prover.prove(d, K.mont(tau), bind)
    evals, opening = scheme.open(com, proof.point[None])
    res, point, finals = prodcheck.verify(shape.statement(), proof.bytes, K.mont(tau), bind)
    assert res.accepted and np.array_equal(point, proof.point)
    wres, wevals = whir_pcs.verify(cfg, point[None], opening, expected_root=root)
    assert wres.accepted, wres
    assert np.array_equal(wevals.reshape(-1, 4), finals) and np.array_equal(evals.reshape(-1, 4), proof.finals)
    other = K.mont([(int.from_bytes(root, "little") + 1) % P])
    res, _, _ = prodcheck.verify(shape.statement(), proof.bytes, K.mont(tau), other)
    assert not res.accepted and res.check == "ROUND"
    prover.close()
    com.close()
    scheme.close()
    for b in d:
        b.free()


def test_size_2_to_the_20_against_the_products_own_sums(ctx):
    """no Python proof at this size: pks_verify accepts, and s is dot(eq(tau), a * b - c) from pk_eq_table, pk_fe_mul, pk_fe_sub, pk_dot"""
    from provekit_amd import prodcheck
    from provekit_amd import sumcheck as S
    from provekit_amd._lib import lib
    from provekit_amd.field import random_field

    n = 20
    N = 1 << n
    shape = K.Shape("r1cs", n)
    d = [ctx.upload(random_field(N, seed)) for seed in (31, 32, 33)]
    tau = random_field(n, 34)
    prover = prodcheck.Prover(ctx, shape.statement())
    proof = prover.prove(d, tau)
    res, point, finals = prodcheck.verify(shape.statement(), proof.bytes, tau)
    assert res.accepted and res.check == "NONE", res
    d_eq = S.calculate_evaluations_over_boolean_hypercube_for_eq(ctx, tau)
    d_t = ctx.alloc_fe(N)
    ctx._check(lib.pk_fe_mul(ctx.handle, d[0].ptr, d[1].ptr, d_t.ptr, N))
    ctx._check(lib.pk_fe_sub(ctx.handle, d_t.ptr, d[2].ptr, d_t.ptr, N))
    s = S.weighted_sum(ctx, d_eq, d_t, N)
    assert K.unmont(s) == [proof.sum_canonical]
    # ... and the final values are the tables at the point: dot(eq(point), f_j)
    d_eq = S.calculate_evaluations_over_boolean_hypercube_for_eq(ctx, proof.point, d_eq)
    for j in range(3):
        assert np.array_equal(S.weighted_sum(ctx, d_eq, d[j], N), proof.finals[j])
    prover.close()
    for b in d + [d_eq, d_t]:
        b.free()


def test_a_creation_whose_arena_the_device_cannot_hold_leaves_nothing_behind():
    """pks_prover_create of a sound statement whose arena (n = 28, m = 4: 16 GiB of folded copies) does not fit the device: it fails
    with its reason in pks_create_error, and the next creation on the same context succeeds and proves the reference's bytes.  Where
    the device has room for 16 GiB the test holds all but 8 GiB of the free memory in one allocation while the creation is tried
    (on an MI355X: 7 s to take 279 GiB and 2.4 s to give them back, of about 9.5 s)"""
    import ctypes

    import torch

    torch.cuda.is_available()
    import provekit_amd
    from provekit_amd import prodcheck

    c = provekit_amd.Context(0)
    try:
        free, _ = torch.cuda.mem_get_info(0)
        held = torch.empty(free - (8 << 30), dtype=torch.uint8, device="cuda:0") if free > 4 * 32 << 27 else None
        s, h = K.Shape("four", 28, n_bind=1).statement().struct(), ctypes.c_void_p()
        rc = prodcheck.lib.pks_prover_create(c.handle, ctypes.addressof(s), ctypes.byref(h))
        del held
        torch.cuda.empty_cache()
        assert rc != 0 and not h.value and prodcheck.lib.pks_create_error() != b""
        shape, tables, tau, bind, want, point, finals, _ = reference("four", 3)
        got = run(c, shape, tables, tau, bind)
        assert got.bytes == want and K.unmont(got.point) == point and K.unmont(got.finals) == finals
    finally:
        c.close()


def test_the_cpp_demo_commits_proves_opens_and_sees_the_tamperings_rejected():
    import subprocess

    demo = os.path.join(ROOT, "examples", "sumcheck_pcs_demo")
    assert os.path.exists(demo), "examples/sumcheck_pcs_demo is built by __graft_entry__.build()"
    out = subprocess.run(["timeout", "-k", "10", "120", demo, "10", "7"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("ok n_vars=10 sumcheck_bytes=%d " % (32 * (1 + 10 * 3 + 3)))
    assert "check=ROUND" in lines[1] and "round 1:" in lines[1] and "check=ROUND" in lines[2] and "check=SUM" in lines[3] and "refused" in lines[4]
