"""GPU: libprovekit_grandproduct.so on the device.  Every layer of the tree bit-exact against Python ints, across the tail kernel's
limit, for every number of layers per launch and several grids; the leaf kernel the same way; the proof bytes against the Python
reference (tests/grandproduct_refs.py); a prover reused, a short buffer, the caller's table untouched; multiset equality with its error
path; one larger size against pkw_evaluate; the composition with libprovekit_whir.so and the PROVIDED contract; the C++ example."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import grandproduct_refs as G  # noqa: E402
import prodcheck_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu
P = K.P
BIND = K.random_elements(3, seed=41)
LAYERS, GRIDS = (1, 2, 3), (1, 3, 0)  # layers per launch; workgroups (0: the library's rule)


def size(n):
    """an int, or "t-1", "t", "t+3": around t = pkg_tail_max_n(), the largest layer the tail kernel takes"""
    from provekit_amd import grandproduct as gp

    return n if isinstance(n, int) else gp.tail_max_n() + int(n[1:] or 0)


def table(n, kind):
    entries = 1 << n
    if kind == "all p-1":
        return [P - 1] * entries
    v = G.random_table(n, seed=7 * n + len(kind))
    if kind != "random":
        v[{"zero first": 0, "zero last": entries - 1, "zero middle": entries // 2}[kind]] = 0
    return v


def heap(layers):
    """[V_0 .. V_{n-1}] -> the Montgomery images of heap elements 1 .. 2^n - 1"""
    return K.mont([x for layer in layers[:-1] for x in layer])


@functools.lru_cache(maxsize=None)
def reference(n, n_bind):
    """computed once per statement and shared, never changed: (the table, the reference prover's dict)"""
    v = G.random_table(n, seed=100 + n)
    return v, G.prove(n, v, BIND[:n_bind])


# below the tail's limit, at it, one and two layers above it (a launch of fewer layers than S), and four above (two launches at
# S = 3, the second of one layer)
@pytest.mark.parametrize("kind", ["all p-1", "zero first", "zero last", "zero middle", "random"])
@pytest.mark.parametrize("n", [1, 2, 3, "t-1", "t", "t+1", "t+2", "t+4"])
def test_every_layer_of_the_tree_is_bit_exact_for_every_layers_per_launch_and_grid(ctx, n, kind):
    from provekit_amd import grandproduct as gp
    from tools.pk_probes import lib as probes

    n = size(n)
    v = table(n, kind)
    layers = G.layers_of(v)
    want, d_v, d_tree = heap(layers), ctx.upload(K.mont(v)), ctx.alloc_fe(1 << n)
    product = gp.tree(ctx, n, d_v, d_tree)
    assert K.unmont(product) == layers[0] and (kind in ("all p-1", "random") or layers[0] == [0])
    assert np.array_equal(ctx.download_fe(d_tree, 1 << n)[1:], want)
    for s in LAYERS:
        for grid in GRIDS:
            ctx.zero(d_tree, 32 << n)
            assert probes.pk_probe_grandproduct_tree(ctx.handle, n, d_v.ptr, d_tree.ptr, s, grid, None) == 0
            assert np.array_equal(ctx.download_fe(d_tree, 1 << n)[1:], want), (s, grid)
    assert np.array_equal(ctx.download_fe(d_v, 1 << n), K.mont(v))
    d_v.free()
    d_tree.free()


@pytest.mark.parametrize("w", [1, 2, 4])
@pytest.mark.parametrize("n", [3, "t", "t+1", "t+3"])
def test_the_leaf_kernel_writes_the_leaves_and_their_tree_bit_exact(ctx, n, w):
    """n <= t: the leaves alone, the tail takes the tree; t + 1: one layer with the leaves whatever S is; t + 3: S layers with them"""
    from tools.pk_probes import lib as probes

    n = size(n)
    cols = [K.random_elements(1 << n, seed=10 * n + j) for j in range(w)]
    cols[0][5] = 0
    gamma, beta = K.random_elements(2, seed=n + w)
    leaf = G.leaves(cols, gamma, beta)
    want_leaf, want = K.mont(leaf), heap(G.layers_of(leaf))
    d_cols = [ctx.upload(K.mont(c)) for c in cols]
    ptrs = (C.c_void_p * w)(*(b.ptr for b in d_cols))
    d_leaf, d_tree = ctx.alloc_fe(1 << n), ctx.alloc_fe(1 << n)
    g, b = K.mont([gamma]), K.mont([beta])
    for s in (0,) + LAYERS:
        for grid in GRIDS:
            ctx.zero(d_tree, 32 << n)
            ctx.zero(d_leaf, 32 << n)
            assert probes.pk_probe_grandproduct_leaf_tree(ctx.handle, n, w, ptrs, g.ctypes.data, b.ctypes.data, d_leaf.ptr, d_tree.ptr, s, grid, None) == 0
            assert np.array_equal(ctx.download_fe(d_leaf, 1 << n), want_leaf), (s, grid)
            assert np.array_equal(ctx.download_fe(d_tree, 1 << n)[1:], want), (s, grid)
    for buf in d_cols + [d_leaf, d_tree]:
        buf.free()


@pytest.mark.parametrize("n_bind", [0, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 5, "t", "t+1"])
def test_the_provers_bytes_product_point_and_value_are_the_references(ctx, n, n_bind):
    """t and t + 1: the tail alone and one tree_kernel launch before it"""
    from provekit_amd import grandproduct as gp

    n = size(n)
    assert n <= 11, "the pure-Python reference prover is too slow above n = 11"
    v, ref = reference(n, n_bind)
    bind = K.mont(BIND[:n_bind]) if n_bind else None
    d_v, prover = ctx.upload(K.mont(v)), gp.GrandProductProver(ctx, gp.Statement(n, n_bind))
    proof, product, point, value = prover.prove(d_v, bind)
    assert proof == ref["proof"]
    assert K.unmont(product) == [ref["P"]] and K.unmont(point) == ref["point"] and K.unmont(value) == [ref["value"]]
    res, layer, seen = gp.verify(prover.stmt, proof, bind, expected_product=product)
    assert res.accepted and layer == 0 and res.offset == len(proof), res
    for a, b in zip(seen, (product, point, value)):
        assert np.array_equal(a, b)
    prover.close()
    d_v.free()


def test_a_prover_proves_two_tables_a_short_buffer_is_refused_and_the_table_is_unchanged(ctx):
    from provekit_amd import grandproduct as gp
    from provekit_amd._lib import ProveKitHipError

    n = 5
    v, ref = reference(n, 3)
    other = G.random_table(n, seed=77, zeros=(9,))
    image = K.mont(v)
    d_v, d_other, prover = ctx.upload(image), ctx.upload(K.mont(other)), gp.GrandProductProver(ctx, gp.Statement(n, 3))
    bind = K.mont(BIND)
    assert prover.prove(d_v, bind)[0] == ref["proof"]
    assert ctx.download_fe(d_v, 1 << n).tobytes() == image.tobytes()
    for cap in (0, 63, len(ref["proof"]) - 1):
        with pytest.raises(ProveKitHipError, match="proof buffer") as e:
            prover.prove(d_v, bind, capacity=cap)
        assert e.value.code == -1 and prover.last_len == len(ref["proof"]) == gp.proof_bytes(prover.stmt)
    proof, product, _, _ = prover.prove(d_other, bind, capacity=len(ref["proof"]) + 100)
    assert proof == G.prove(n, other, BIND)["proof"] and K.unmont(product) == [0]
    assert prover.prove(d_v, bind)[0] == ref["proof"]
    with pytest.raises(ProveKitHipError, match="bind element 1 is not below p"):
        prover.prove(d_v, np.array([[1, 0, 0, 0], [2**64 - 1] * 4, [1, 0, 0, 0]], dtype=np.uint64))
    prover.close()
    d_v.free()
    d_other.free()


def test_no_bit_of_a_proof_depends_on_the_layers_per_launch_or_the_grid(ctx):
    """n = t + 3 through the lab's probe of a prover: the proof, the product and the claim"""
    from provekit_amd import grandproduct as gp
    from tools.pk_probes import lib as probes

    n = size("t+3")
    v = G.random_table(n, seed=3)
    d_v, prover = ctx.upload(K.mont(v)), gp.GrandProductProver(ctx, gp.Statement(n, 0))
    outs = []
    for s, grid in [(0, 0), (1, 1), (2, 3), (3, 7), (3, 300)]:
        assert probes.pk_probe_grandproduct_set_knobs(prover.handle, s, grid) == 0
        outs.append(prover.prove(d_v))
    for got in outs[1:]:
        assert got[0] == outs[0][0] and all(np.array_equal(a, b) for a, b in zip(got[1:], outs[0][1:]))
    want = 1
    for x in v:
        want = want * x % P
    assert K.unmont(outs[0][1]) == [want] and gp.verify(prover.stmt, outs[0][0], expected_product=outs[0][1])[0].accepted
    tree_ms, layer_ms = C.c_double(), (C.c_double * 28)()
    assert probes.pk_probe_grandproduct_profile(prover.handle, C.byref(tree_ms), layer_ms) == 0
    assert tree_ms.value > 0 and all(layer_ms[d] > 0 for d in range(1, n)) and layer_ms[0] == 0 and layer_ms[n] == 0
    prover.close()
    d_v.free()


def permuted(n, w, seed):
    rng = np.random.default_rng(seed)
    a = [K.random_elements(1 << n, seed=seed + j) for j in range(w)]
    perm = rng.permutation(1 << n)
    return a, [[col[i] for i in perm] for col in a]


@pytest.mark.parametrize("w", [1, 2, 4])
def test_multiset_proofs_are_the_references_bytes(ctx, w):
    from provekit_amd import grandproduct as gp

    n = 5
    a, b = permuted(n, w, seed=20 + w)
    ref = G.multiset_prove(n, a, b, BIND[:2])
    d_a, d_b = [ctx.upload(K.mont(c)) for c in a], [ctx.upload(K.mont(c)) for c in b]
    prover = gp.MultisetProver(ctx, gp.MultisetStatement(n, w, 2))
    proof, claims = prover.prove(d_a, d_b, K.mont(BIND[:2]))
    assert proof == ref["proof"]
    for name in ("gamma", "beta", "comb_a", "comb_b"):
        assert K.unmont(getattr(claims, name)) == [ref[name]], name
    assert K.unmont(claims.z_a) == ref["z_a"] and K.unmont(claims.z_b) == ref["z_b"]
    res, side, layer, seen = gp.multiset_verify(prover.stmt, proof, K.mont(BIND[:2]))
    assert res.accepted and np.array_equal(seen.comb_b, claims.comb_b) and np.array_equal(seen.z_a, claims.z_a)
    for buf, image in zip(d_a + d_b, a + b):
        assert ctx.download_fe(buf, 1 << n).tobytes() == K.mont(image).tobytes()
        buf.free()
    prover.close()


def test_a_permutation_is_proved_a_changed_row_is_unsatisfied_and_the_prover_stays_usable(ctx):
    """n = 12, w = 2: the leaf kernel takes two layers with the leaves; the claims are the columns' extensions, combined"""
    from provekit_amd import grandproduct as gp, whir_pcs
    from provekit_amd._lib import ProveKitHipError

    n, w = 12, 2
    a, b = permuted(n, w, seed=31)
    d_a, d_b = [ctx.upload(K.mont(c)) for c in a], [ctx.upload(K.mont(c)) for c in b]
    changed = list(b[1])
    changed[1234] = (changed[1234] + 1) % P
    d_changed = ctx.upload(K.mont(changed))
    prover = gp.MultisetProver(ctx, gp.MultisetStatement(n, w, 0))
    with pytest.raises(ProveKitHipError, match="not equal as multisets") as e:
        prover.prove(d_a, [d_b[0], d_changed])
    assert e.value.code == gp.ERR_UNSATISFIED and not any(bytes(prover.buffer)), "nothing is written"
    proof, claims = prover.prove(d_a, d_b)
    res, side, layer, seen = gp.multiset_verify(prover.stmt, proof)
    assert res.accepted and res.offset == len(proof) == gp.proof_bytes(prover.stmt), res
    beta = K.unmont(claims.beta)[0]
    for cols, z, comb in ((d_a, seen.z_a, seen.comb_a), (d_b, seen.z_b, seen.comb_b)):
        ev = whir_pcs.evaluate(ctx, cols, n, z[None])
        assert (K.unmont(ev[0, 0])[0] + beta * K.unmont(ev[1, 0])[0]) % P == K.unmont(comb)[0]
    for buf in d_a + d_b + [d_changed]:
        buf.free()
    prover.close()


def test_one_larger_table_its_product_and_its_claim(ctx):
    from provekit_amd import grandproduct as gp, whir_pcs

    n = 18
    v = G.random_table(n, seed=18)
    want = 1
    for x in v:
        want = want * x % P
    d_v, prover = ctx.upload(K.mont(v)), gp.GrandProductProver(ctx, gp.Statement(n, 0))
    proof, product, point, value = prover.prove(d_v)
    assert K.unmont(product) == [want] and len(proof) == 64 + 48 * (n - 1) * (n + 2)
    res, layer, seen = gp.verify(prover.stmt, proof, expected_product=product)
    assert res.accepted and np.array_equal(seen[1], point) and np.array_equal(seen[2], value), res
    assert np.array_equal(whir_pcs.evaluate(ctx, [d_v], n, point[None])[0, 0], value)
    prover.close()
    d_v.free()


def test_composition_with_the_commitment_scheme_and_the_provided_contract(ctx):
    """commit, bind the root, prove, open at z_n, verify.  Then a table changed after its commitment: pkg_verify accepts the proof --
    accepted PROVIDED v(z_n) = c_n -- and the opening of the committed table at z_n gives another value"""
    import whir_pcs_cases as W
    from provekit_amd import grandproduct as gp, whir_pcs

    n = 12
    v = G.random_table(n, seed=12)
    d_v = ctx.upload(K.mont(v))
    cfg = W.small_config(n, 1)
    scheme, prover = whir_pcs.Scheme(ctx, cfg), gp.GrandProductProver(ctx, gp.Statement(n, 1))
    com = scheme.commit([d_v])
    bind = K.mont([int.from_bytes(com.root(), "little")])
    proof, product, point, value = prover.prove(d_v, bind)
    res, layer, seen = gp.verify(prover.stmt, proof, bind, expected_product=product)
    assert res.accepted, res
    evals, opening = scheme.open(com, seen[1][None])
    wres, wevals = whir_pcs.verify(cfg, seen[1][None], opening, expected_root=com.root())
    assert wres.accepted and np.array_equal(wevals[0, 0], seen[2]) and np.array_equal(evals[0, 0], seen[2]), wres
    # another root: other challenges, rejected at the first layer
    res, layer, _ = gp.verify(prover.stmt, proof, K.mont([1]))
    assert (res.check, layer) == ("SUM", 1)

    changed = list(v)
    changed[99] = (changed[99] + 1) % P
    d_changed = ctx.upload(K.mont(changed))
    proof, product, point, value = prover.prove(d_changed, bind)
    res, layer, seen = gp.verify(prover.stmt, proof, bind)
    assert res.accepted, res
    evals, opening = scheme.open(com, seen[1][None])
    wres, wevals = whir_pcs.verify(cfg, seen[1][None], opening, expected_root=com.root())
    assert wres.accepted and not np.array_equal(wevals[0, 0], seen[2])
    com.close()
    prover.close()
    scheme.close()
    d_v.free()
    d_changed.free()


def test_the_cpp_demo_commits_proves_opens_and_sees_the_error_path():
    import subprocess

    demo = os.path.join(ROOT, "examples", "grandproduct_pcs_demo")
    assert os.path.exists(demo), "examples/grandproduct_pcs_demo is built by __graft_entry__.build()"
    out = subprocess.run(["timeout", "-k", "10", "120", demo, "12", "7"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("ok n=12 multiset_bytes=%d " % G.multiset_proof_bytes(12))
    assert lines[1].startswith("one entry changed: refused rc=-6") and "not equal as multisets" in lines[1]
    assert "another root: rejected" in lines[2]
