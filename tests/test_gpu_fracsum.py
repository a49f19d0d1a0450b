"""GPU: libprovekit_fracsum.so on the device.  Every layer of both trees bit-exact against Python ints, across the tail kernel's limit,
for every number of layers per launch and several grids; the lookup leaf kernel and the combine kernel the same way; the proof bytes
against the Python reference (tests/fracsum_refs.py); a prover reused, a short buffer, the caller's tables untouched, a zero
denominator; the lookup with its error paths; one larger size against pkw_evaluate; the composition with libprovekit_whir.so and the
PROVIDED contract; the C++ example."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import fracsum_refs as F  # noqa: E402
import prodcheck_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu
P = K.P
BIND = K.random_elements(3, seed=41)
LAYERS, GRIDS = (1, 2, 3), (1, 3, 0)  # layers per launch; workgroups (0: the library's rule)


def size(n):
    """an int, or "t-1", "t", "t+3": around t = pkf_tail_max_n(), the largest layer the tail kernel takes"""
    from provekit_amd import fracsum as fs

    return n if isinstance(n, int) else fs.tail_max_n() + int(n[1:] or 0)


def tables(n, kind):
    """(p or None, q) of 2^n entries"""
    entries = 1 << n
    if kind == "all p-1":
        return [P - 1] * entries, [P - 1] * entries
    p, q = K.random_elements(entries, seed=11 * n + len(kind)), F.random_table(n, seed=7 * n + len(kind))
    if kind == "unit":
        return None, q
    if kind == "zero numerator":
        p[entries // 2] = 0
        p[0] = 0
    elif kind != "random":
        q[{"zero denominator first": 0, "zero denominator last": entries - 1, "zero denominator middle": entries // 2}[kind]] = 0
    return p, q


def heap(layers):
    """[L_0 .. L_{n-1}, L_n] -> the Montgomery images of heap elements 1 .. 2^n - 1"""
    return K.mont([x for layer in layers[:-1] for x in layer])


def upload_or_none(ctx, values):
    return None if values is None else ctx.upload(K.mont(values))


def ptr(buf):
    return None if buf is None else buf.ptr


@functools.lru_cache(maxsize=None)
def reference(n, unit, n_bind):
    """computed once per statement and shared, never changed: (p or None, q, the reference prover's dict)"""
    p, q = (None if unit else K.random_elements(1 << n, seed=200 + n)), F.random_table(n, seed=100 + n)
    return p, q, F.prove(n, p, q, BIND[:n_bind])


# below the tail's limit, at it, one and two layers above it (a launch of fewer layers than S), and four above (two launches at
# S = 3, the second of one layer)
@pytest.mark.parametrize("kind", ["all p-1", "zero numerator", "zero denominator first", "zero denominator middle", "zero denominator last", "random", "unit"])
@pytest.mark.parametrize("n", [1, 2, 3, "t-1", "t", "t+1", "t+2", "t+4"])
def test_every_layer_of_both_trees_is_bit_exact_for_every_layers_per_launch_and_grid(ctx, n, kind):
    from provekit_amd import fracsum as fs
    from tools.pk_probes import lib as probes

    n = size(n)
    p, q = tables(n, kind)
    ps, qs = F.layers_of(p, q)
    want_p, want_q = heap(ps), heap(qs)
    d_p, d_q, d_pt, d_qt = upload_or_none(ctx, p), ctx.upload(K.mont(q)), ctx.alloc_fe(1 << n), ctx.alloc_fe(1 << n)
    fraction = fs.tree(ctx, n, d_p, d_q, d_pt, d_qt)
    assert K.unmont(fraction) == [ps[0][0], qs[0][0]] and (qs[0][0] == 0) == kind.startswith("zero denominator")
    assert np.array_equal(ctx.download_fe(d_pt, 1 << n)[1:], want_p) and np.array_equal(ctx.download_fe(d_qt, 1 << n)[1:], want_q)
    for s in LAYERS:
        for grid in GRIDS:
            ctx.zero(d_pt, 32 << n)
            ctx.zero(d_qt, 32 << n)
            assert probes.pk_probe_fracsum_tree(ctx.handle, n, ptr(d_p), d_q.ptr, d_pt.ptr, d_qt.ptr, s, grid, None) == 0
            assert np.array_equal(ctx.download_fe(d_pt, 1 << n)[1:], want_p), (s, grid)
            assert np.array_equal(ctx.download_fe(d_qt, 1 << n)[1:], want_q), (s, grid)
    assert np.array_equal(ctx.download_fe(d_q, 1 << n), K.mont(q)) and (p is None or np.array_equal(ctx.download_fe(d_p, 1 << n), K.mont(p)))
    for buf in (d_p, d_q, d_pt, d_qt):
        if buf is not None:
            buf.free()


@pytest.mark.parametrize("side", ["F", "T"])
@pytest.mark.parametrize("n", [3, "t", "t+1", "t+3"])
def test_the_lookup_leaf_kernel_writes_the_leaves_and_their_trees_bit_exact(ctx, n, side):
    """n <= t: the leaves alone, the tail takes the trees; t + 1: one layer with the leaves whatever S is; t + 3: S layers with them.
    Side F has unit numerators, side T reads the multiplicities in place"""
    from tools.pk_probes import lib as probes

    n = size(n)
    table = K.random_elements(1 << n, seed=10 * n)
    (alpha,) = K.random_elements(1, seed=n)
    table[5] = alpha  # a zero denominator among the leaves
    m = None if side == "F" else [x % 7 for x in K.random_elements(1 << n, seed=n + 1)]
    leaf = [(alpha - v) % P for v in table]
    ps, qs = F.layers_of(m, leaf)
    want_leaf, want_p, want_q = K.mont(leaf), heap(ps), heap(qs)
    d_table, d_m = ctx.upload(K.mont(table)), upload_or_none(ctx, m)
    d_leaf, d_pt, d_qt = ctx.alloc_fe(1 << n), ctx.alloc_fe(1 << n), ctx.alloc_fe(1 << n)
    a = K.mont([alpha])
    for s in (0,) + LAYERS:
        for grid in GRIDS:
            for buf in (d_leaf, d_pt, d_qt):
                ctx.zero(buf, 32 << n)
            assert probes.pk_probe_fracsum_lookup_leaf(ctx.handle, n, d_table.ptr, ptr(d_m), a.ctypes.data, d_leaf.ptr, d_pt.ptr, d_qt.ptr, s, grid, None) == 0
            assert np.array_equal(ctx.download_fe(d_leaf, 1 << n), want_leaf), (s, grid)
            assert np.array_equal(ctx.download_fe(d_pt, 1 << n)[1:], want_p), (s, grid)
            assert np.array_equal(ctx.download_fe(d_qt, 1 << n)[1:], want_q), (s, grid)
    assert np.array_equal(ctx.download_fe(d_table, 1 << n), K.mont(table)) and (m is None or np.array_equal(ctx.download_fe(d_m, 1 << n), K.mont(m)))
    for buf in (d_table, d_m, d_leaf, d_pt, d_qt):
        if buf is not None:
            buf.free()


@pytest.mark.parametrize("count", [1, 2, 255, 256, 257, 1000])
def test_the_combine_kernel_is_bit_exact_with_and_without_numerators(ctx, count):
    from tools.pk_probes import lib as probes

    p, q = K.random_elements(count, seed=count), K.random_elements(count, seed=count + 1)
    p[0], q[count - 1] = 0, P - 1
    (lam,) = K.random_elements(1, seed=3)
    d_p, d_q, d_u, l = ctx.upload(K.mont(p)), ctx.upload(K.mont(q)), ctx.alloc_fe(count + 1), K.mont([lam])
    for numerators, want in ((d_p.ptr, [(a + lam * b) % P for a, b in zip(p, q)]), (None, [(1 + lam * b) % P for b in q])):
        for grid in GRIDS:
            ctx.zero(d_u, 32 * (count + 1))
            assert probes.pk_probe_fracsum_combine(ctx.handle, count, numerators, d_q.ptr, l.ctypes.data, d_u.ptr, grid, None) == 0
            assert K.unmont(ctx.download_fe(d_u, count + 1)) == want + [0], grid  # and nothing past the end
    for buf in (d_p, d_q, d_u):
        buf.free()


@pytest.mark.parametrize("n_bind", [0, 3])
@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 5, "t", "t+1"])
def test_the_provers_bytes_fraction_point_and_values_are_the_references(ctx, n, unit, n_bind):
    """t and t + 1: the tail alone and one frac_tree_kernel launch before it"""
    from provekit_amd import fracsum as fs

    n = size(n)
    assert n <= 11, "the pure-Python reference prover is too slow above n = 11"
    p, q, ref = reference(n, unit, n_bind)
    bind = K.mont(BIND[:n_bind]) if n_bind else None
    d_p, d_q, prover = upload_or_none(ctx, p), ctx.upload(K.mont(q)), fs.FractionalSumProver(ctx, fs.Statement(n, n_bind, unit))
    proof, fraction, point, value_p, value_q = prover.prove(d_p, d_q, bind)
    assert proof == ref["proof"]
    assert K.unmont(fraction) == [ref["P"], ref["Q"]] and K.unmont(point) == ref["point"] and K.unmont(value_q) == [ref["value_q"]]
    assert (value_p is None and ref["value_p"] is None) if unit else K.unmont(value_p) == [ref["value_p"]]
    res, layer, seen = fs.verify(prover.stmt, proof, bind, expected_fraction=fraction)
    assert res.accepted and layer == 0 and res.offset == len(proof), res
    for a, b in zip(seen, (fraction, point, value_p, value_q)):
        assert (a is None and b is None) or np.array_equal(a, b)
    prover.close()
    for buf in (d_p, d_q):
        if buf is not None:
            buf.free()


def test_a_prover_proves_two_tables_a_short_buffer_is_refused_and_the_tables_are_unchanged(ctx):
    from provekit_amd import fracsum as fs
    from provekit_amd._lib import ProveKitHipError

    n = 5
    p, q, ref = reference(n, 0, 3)
    other_p, other_q = F.random_table(n, seed=77, zeros=(9,)), F.random_table(n, seed=78)
    images = K.mont(p), K.mont(q)
    d_p, d_q, d_op, d_oq = ctx.upload(images[0]), ctx.upload(images[1]), ctx.upload(K.mont(other_p)), ctx.upload(K.mont(other_q))
    prover = fs.FractionalSumProver(ctx, fs.Statement(n, 3))
    bind = K.mont(BIND)
    assert prover.prove(d_p, d_q, bind)[0] == ref["proof"]
    assert ctx.download_fe(d_p, 1 << n).tobytes() == images[0].tobytes() and ctx.download_fe(d_q, 1 << n).tobytes() == images[1].tobytes()
    for cap in (0, 127, len(ref["proof"]) - 1):
        with pytest.raises(ProveKitHipError, match="proof buffer") as e:
            prover.prove(d_p, d_q, bind, capacity=cap)
        assert e.value.code == -1 and prover.last_len == len(ref["proof"]) == fs.proof_bytes(prover.stmt)
    proof = prover.prove(d_op, d_oq, bind, capacity=len(ref["proof"]) + 100)[0]
    assert proof == F.prove(n, other_p, other_q, BIND)["proof"]
    assert prover.prove(d_p, d_q, bind)[0] == ref["proof"]
    with pytest.raises(ProveKitHipError, match="bind element 1 is not below p"):
        prover.prove(d_p, d_q, np.array([[1, 0, 0, 0], [2**64 - 1] * 4, [1, 0, 0, 0]], dtype=np.uint64))
    with pytest.raises(ProveKitHipError, match="NULL exactly when") as e:  # the numerators and the statement's unit go together
        prover.prove(None, d_q, bind)
    assert e.value.code == -1
    prover.close()
    for buf in (d_p, d_q, d_op, d_oq):
        buf.free()


@pytest.mark.parametrize("unit", [0, 1])
def test_a_zero_denominator_is_unsatisfied_nothing_is_written_and_the_prover_stays_usable(ctx, unit):
    from provekit_amd import fracsum as fs
    from provekit_amd._lib import ProveKitHipError

    n = 5
    p, q, ref = reference(n, unit, 0)
    zeroed = list(q)
    zeroed[17] = 0
    d_p, d_q, d_zero = upload_or_none(ctx, p), ctx.upload(K.mont(q)), ctx.upload(K.mont(zeroed))
    prover = fs.FractionalSumProver(ctx, fs.Statement(n, 0, unit))
    with pytest.raises(ProveKitHipError, match="denominator is zero") as e:
        prover.prove(d_p, d_zero)
    assert e.value.code == fs.ERR_UNSATISFIED and not any(bytes(prover.buffer)), "nothing is written"
    assert prover.prove(d_p, d_q)[0] == ref["proof"]
    prover.close()
    for buf in (d_p, d_q, d_zero):
        if buf is not None:
            buf.free()


@pytest.mark.parametrize("unit", [0, 1])
def test_no_bit_of_a_proof_depends_on_the_layers_per_launch_or_the_grid(ctx, unit):
    """n = t + 3 through the lab's probe of a prover: the proof, the fraction and the claims"""
    from provekit_amd import fracsum as fs
    from tools.pk_probes import lib as probes

    n = size("t+3")
    p, q = (None if unit else K.random_elements(1 << n, seed=4)), F.random_table(n, seed=3)
    d_p, d_q, prover = upload_or_none(ctx, p), ctx.upload(K.mont(q)), fs.FractionalSumProver(ctx, fs.Statement(n, 0, unit))
    outs = []
    for s, grid in [(0, 0), (1, 1), (2, 3), (3, 7), (3, 300)]:
        assert probes.pk_probe_fracsum_set_knobs(prover.handle, s, grid) == 0
        outs.append(prover.prove(d_p, d_q))
    for got in outs[1:]:
        assert got[0] == outs[0][0] and all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(got[1:], outs[0][1:]))
    num, den = K.unmont(outs[0][1])
    assert num * pow(den, -1, P) % P == F.fraction_sum(p, q) and fs.verify(prover.stmt, outs[0][0], expected_fraction=outs[0][1])[0].accepted
    tree_ms, combine_ms, layer_ms = C.c_double(), (C.c_double * 28)(), (C.c_double * 28)()
    assert probes.pk_probe_fracsum_profile(prover.handle, C.byref(tree_ms), combine_ms, layer_ms) == 0
    assert tree_ms.value > 0 and all(layer_ms[d] > 0 and combine_ms[d] > 0 for d in range(1, n)) and layer_ms[0] == 0 and layer_ms[n] == 0
    prover.close()
    for buf in (d_p, d_q):
        if buf is not None:
            buf.free()


def lookup_case(n, k, seed):
    """(f, t, idx): t of distinct entries, f drawn from it"""
    rng = np.random.default_rng(seed)
    t = K.random_elements(1 << k, seed=seed)
    idx = rng.integers(0, 1 << k, size=1 << n)
    return [t[i] for i in idx], t, idx


def device_multiplicities(ctx, n, k, d_f, d_t, idx):
    """m as pkl_multiplicities makes and validates it"""
    from provekit_amd import lookup

    d_idx, d_m = ctx.upload(np.asarray(idx, dtype=np.uint32)), ctx.alloc_fe(1 << k)
    counter = lookup.LookupProver(ctx, lookup.Statement(n, k))
    counter.multiplicities(d_f, d_t, d_idx, d_m)
    m = ctx.download_fe(d_m, 1 << k)
    counter.close()
    d_idx.free()
    d_m.free()
    return ctx.upload(m)  # the fractional-sum library never sees the lookup library's prover


@pytest.mark.parametrize("n, k", [(3, 2), ("t+1", 4), (5, "t+1")])
def test_lookup_proofs_are_the_references_bytes_with_the_lookup_librarys_multiplicities(ctx, n, k):
    from provekit_amd import fracsum as fs

    n, k = size(n), size(k)
    f, t, idx = lookup_case(n, k, seed=20 + n + k)
    ref = F.lookup_prove(n, k, f, t, F.multiplicities(f, t), BIND)
    d_f, d_t = ctx.upload(K.mont(f)), ctx.upload(K.mont(t))
    d_m = device_multiplicities(ctx, n, k, d_f, d_t, idx)
    assert K.unmont(ctx.download_fe(d_m, 1 << k)) == F.multiplicities(f, t)
    prover = fs.LookupProver(ctx, fs.LookupStatement(n, k, 3))
    proof, claims = prover.prove(d_f, d_t, d_m, K.mont(BIND))
    assert proof == ref["proof"]
    for name in ("alpha", "f_value", "t_value", "m_value"):
        assert K.unmont(getattr(claims, name)) == [ref[name]], name
    assert K.unmont(claims.z_f) == ref["z_f"] and K.unmont(claims.z_t) == ref["z_t"]
    res, side, layer, seen = fs.lookup_verify(prover.stmt, proof, K.mont(BIND))
    assert res.accepted and np.array_equal(seen.m_value, claims.m_value) and np.array_equal(seen.z_f, claims.z_f) and np.array_equal(seen.z_t, claims.z_t)
    for buf, image in ((d_f, f), (d_t, t), (d_m, F.multiplicities(f, t))):
        assert ctx.download_fe(buf, len(image)).tobytes() == K.mont(image).tobytes()
        buf.free()
    prover.close()


def test_an_entry_outside_the_table_and_alpha_on_an_entry_are_unsatisfied_and_name_the_cause(ctx):
    from provekit_amd import fracsum as fs
    from provekit_amd._lib import ProveKitHipError

    n, k = 4, 5  # fewer lookups than entries: some entry of t is not used
    f, t, idx = lookup_case(n, k, seed=31)
    m = F.multiplicities(f, t)
    alpha, _ = F.lookup_challenges(n, k, BIND)  # what the prover will squeeze for this statement and these bind elements
    outside = list(f)
    outside[9] = (outside[9] + 1) % P
    free = next(j for j in range(1 << k) if m[j] == 0)  # an entry of t that f does not use: t may hold anything there
    t_alpha = list(t)
    t_alpha[free] = alpha
    f_alpha, t_both = list(f), list(t)
    t_both[idx[0]] = alpha
    f_alpha = [t_both[i] for i in idx]
    d = {name: ctx.upload(K.mont(v)) for name, v in (("f", f), ("t", t), ("m", m), ("outside", outside), ("t_alpha", t_alpha), ("f_alpha", f_alpha), ("t_both", t_both))}
    wrong_m = list(m)
    wrong_m[3] += 1
    d["wrong_m"] = ctx.upload(K.mont(wrong_m))
    prover = fs.LookupProver(ctx, fs.LookupStatement(n, k, 3))
    bind = K.mont(BIND)
    for args, cause in (((d["outside"], d["t"], d["m"]), "fractions differ: f is not inside t under m"), ((d["f"], d["t"], d["wrong_m"]), "fractions differ"),
                        ((d["f"], d["t_alpha"], d["m"]), "alpha is an entry of t"), ((d["f_alpha"], d["t_both"], d["m"]), "alpha is an entry of f")):
        with pytest.raises(ProveKitHipError, match=cause) as e:
            prover.prove(*args, bind)
        assert e.value.code == fs.ERR_UNSATISFIED and not any(bytes(prover.buffer)), "nothing is written"
    proof, claims = prover.prove(d["f"], d["t"], d["m"], bind)
    assert proof == F.lookup_prove(n, k, f, t, m, BIND)["proof"] and K.unmont(claims.alpha) == [alpha]
    prover.close()
    for buf in d.values():
        buf.free()


def test_one_larger_lookup_is_verified_and_its_three_claims_are_the_tables_extensions(ctx):
    from provekit_amd import fracsum as fs, whir_pcs

    n, k = 16, 12
    rng = np.random.default_rng(16)
    t = np.arange(1 << k, dtype=np.uint64)  # a range check
    idx = rng.integers(0, 1 << k, size=1 << n)
    f = t[idx]

    def image(column):
        limbs = np.zeros((len(column), 4), dtype=np.uint64)
        limbs[:, 0] = column
        return limbs

    d_f, d_t = ctx.upload(image(f)), ctx.upload(image(t))
    from provekit_amd._lib import lib as product

    for buf, count in ((d_f, 1 << n), (d_t, 1 << k)):
        assert product.pk_fe_to_mont(ctx.handle, buf.ptr, buf.ptr, count) == 0
    d_m = device_multiplicities(ctx, n, k, d_f, d_t, idx)
    prover = fs.LookupProver(ctx, fs.LookupStatement(n, k, 0))
    proof, claims = prover.prove(d_f, d_t, d_m)
    assert len(proof) == fs.proof_bytes(prover.stmt) == 128 + (n - 1) * (48 * n + 160) - 32 + 128 + (k - 1) * (48 * k + 160)
    res, side, layer, seen = fs.lookup_verify(prover.stmt, proof)
    assert res.accepted and res.offset == len(proof), res
    for name in ("alpha", "z_f", "z_t", "f_value", "t_value", "m_value"):
        assert np.array_equal(getattr(seen, name), getattr(claims, name)), name
    assert np.array_equal(whir_pcs.evaluate(ctx, [d_f], n, seen.z_f[None])[0, 0], seen.f_value)
    ev = whir_pcs.evaluate(ctx, [d_t, d_m], k, seen.z_t[None])
    assert np.array_equal(ev[0, 0], seen.t_value) and np.array_equal(ev[1, 0], seen.m_value)
    prover.close()
    for buf in (d_f, d_t, d_m):
        buf.free()


def test_composition_with_the_commitment_scheme_and_the_provided_contract(ctx):
    """commit f, t and m in one phase, bind the roots, prove, open f at z_F and {t, m} at z_T, verify.  A claim value changed by one is
    not what the opening binds"""
    import whir_pcs_cases as W
    from provekit_amd import fracsum as fs, whir_pcs

    n, k = 12, 8
    f, t, idx = lookup_case(n, k, seed=12)
    m = F.multiplicities(f, t)
    d_f, d_t, d_m = ctx.upload(K.mont(f)), ctx.upload(K.mont(t)), ctx.upload(K.mont(m))
    cfg_n, cfg_k = W.small_config(n, 1), W.small_config(k, 2)
    scheme_n, scheme_k, prover = whir_pcs.Scheme(ctx, cfg_n), whir_pcs.Scheme(ctx, cfg_k), fs.LookupProver(ctx, fs.LookupStatement(n, k, 2))
    com_f, com_tm = scheme_n.commit([d_f]), scheme_k.commit([d_t, d_m])
    bind = K.mont([int.from_bytes(com_f.root(), "little"), int.from_bytes(com_tm.root(), "little")])
    proof, _ = prover.prove(d_f, d_t, d_m, bind)
    res, side, layer, seen = fs.lookup_verify(prover.stmt, proof, bind)
    assert res.accepted, res
    evals_f, opening_f = scheme_n.open(com_f, seen.z_f[None])
    wres, wevals = whir_pcs.verify(cfg_n, seen.z_f[None], opening_f, expected_root=com_f.root())
    assert wres.accepted and np.array_equal(wevals[0, 0], seen.f_value) and np.array_equal(evals_f[0, 0], seen.f_value), wres
    evals_tm, opening_tm = scheme_k.open(com_tm, seen.z_t[None])
    wres, wevals = whir_pcs.verify(cfg_k, seen.z_t[None], opening_tm, expected_root=com_tm.root())
    assert wres.accepted and np.array_equal(wevals[0, 0], seen.t_value) and np.array_equal(wevals[1, 0], seen.m_value), wres
    # a claim changed by one is not the value the opening binds: the caller's comparison fails
    changed = K.mont([(K.unmont(seen.m_value)[0] + 1) % P])[0]
    assert not np.array_equal(wevals[1, 0], changed)
    # a column changed after its commitment (to another entry of t, with the multiplicities that go with it): pkf_lookup_verify accepts
    # the proof -- accepted PROVIDED the three claims -- and the openings of the committed f and m at the points give other values
    f2 = list(f)
    f2[99] = next(v for v in t if v != f[99])
    d_f2, d_m2 = ctx.upload(K.mont(f2)), ctx.upload(K.mont(F.multiplicities(f2, t)))
    proof2, _ = prover.prove(d_f2, d_t, d_m2, bind)
    res, side, layer, seen2 = fs.lookup_verify(prover.stmt, proof2, bind)
    assert res.accepted, res
    _, opening_f = scheme_n.open(com_f, seen2.z_f[None])
    wres, wevals = whir_pcs.verify(cfg_n, seen2.z_f[None], opening_f, expected_root=com_f.root())
    assert wres.accepted and not np.array_equal(wevals[0, 0], seen2.f_value)
    _, opening_tm = scheme_k.open(com_tm, seen2.z_t[None])
    wres, wevals = whir_pcs.verify(cfg_k, seen2.z_t[None], opening_tm, expected_root=com_tm.root())
    assert wres.accepted and np.array_equal(wevals[0, 0], seen2.t_value) and not np.array_equal(wevals[1, 0], seen2.m_value)
    d_f2.free()
    d_m2.free()
    # other roots: another alpha and other seeds, rejected at the first layer of side F
    res, side, layer, _ = fs.lookup_verify(prover.stmt, proof, K.mont([1, 2]))
    assert (res.check, side, layer) == ("SUM", "F", 1)
    for closing in (com_f, com_tm, prover, scheme_n, scheme_k):
        closing.close()
    for buf in (d_f, d_t, d_m):
        buf.free()


def test_the_cpp_demo_commits_once_proves_opens_and_sees_the_unsatisfied_path():
    import subprocess

    demo = os.path.join(ROOT, "examples", "fracsum_pcs_demo")
    assert os.path.exists(demo), "examples/fracsum_pcs_demo is built by __graft_entry__.build()"
    out = subprocess.run(["timeout", "-k", "10", "120", demo, "12", "8", "7"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("ok n=12 k=8 lookup_bytes=%d " % F.lookup_proof_bytes(12, 8))
    assert lines[1].startswith("one entry outside the table: refused rc=-6") and "fractions differ" in lines[1]
    assert "another root: rejected" in lines[2]
