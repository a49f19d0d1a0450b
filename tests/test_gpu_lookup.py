"""GPU: libprovekit_lookup.so on the device.  The proof bytes, alpha, s and the tables m, h_f, h_t against the Python reference
(tests/lookup_refs.py); the count kernel across its LDS / device-memory boundary and under skew against numpy.bincount; the bits across
grids; validation failures with the smallest bad index; alpha hitting the table; the caller's tables untouched; the order of the calls;
the composition with libprovekit_whir.so and the PROVIDED contract; the C++ example."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import lookup_refs as L  # noqa: E402
import prodcheck_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu
P = K.P

# fewer lookups / entries than one lane batch (1, 2, 3); one workgroup of lookups against a table of one lane batch (8, 8); a column
# larger than its table and several tiles of lookups (9, 4), (13, 2); a table larger than its column and past the LDS histogram (10, 13)
SIZES = [(1, 1), (2, 1), (1, 3), (8, 8), (9, 4), (13, 2), (10, 13)]
BIND, BIND2 = K.random_elements(2, seed=41), K.random_elements(1, seed=42)


@functools.lru_cache(maxsize=None)
def reference(n, k):
    """computed once per size and shared, never changed: (f, t, idx, the reference prover's dict)"""
    f, t, idx = L.random_case(n, k, seed=100 * n + k)
    return f, t, idx, L.prove(n, k, f, t, idx, BIND, BIND2)


class Device:
    """a column, its table and idx on the device, with room for m; values as Montgomery images (numpy) or canonical ints"""

    def __init__(self, ctx, k, f, t, idx):
        self.ctx = ctx
        self.images = [f if isinstance(f, np.ndarray) else K.mont(f), t if isinstance(t, np.ndarray) else K.mont(t), np.asarray(idx, dtype=np.uint32)]
        self.f, self.t, self.idx = (ctx.upload(a) for a in self.images)
        self.m = ctx.alloc_fe(1 << k)

    def free(self):
        for b in (self.f, self.t, self.idx, self.m):
            b.free()


def prove(ctx, prover, d, bind=BIND, bind2=BIND2, tables=False):
    """one proof on `prover` -> (proof bytes, Claims, alpha [4], then m, h_f, h_t as downloaded if `tables`)"""
    n, k = prover.stmt.n, prover.stmt.k
    prover.multiplicities(d.f, d.t, d.idx, d.m)
    alpha, hf, ht = prover.begin(d.t, d.idx, K.mont(bind) if len(bind) else None)
    got = [ctx.download_fe(d.m, 1 << k), ctx.download_fe(hf, 1 << n), ctx.download_fe(ht, 1 << k)] if tables else []
    proof, claims = prover.finish(K.mont(bind2) if len(bind2) else None)
    return [proof, claims, alpha] + got


def make_prover(ctx, n, k, n_bind=2, n_bind2=1):
    from provekit_amd import lookup

    return lookup.LookupProver(ctx, lookup.Statement(n, k, n_bind, n_bind2))


@pytest.mark.parametrize("n, k", SIZES)
def test_the_provers_bytes_alpha_sum_and_tables_are_the_references(ctx, n, k):
    from provekit_amd import lookup

    f, t, idx, ref = reference(n, k)
    d, prover = Device(ctx, k, f, t, idx), make_prover(ctx, n, k)
    proof, claims, alpha, m, h_f, h_t = prove(ctx, prover, d, tables=True)
    assert K.unmont(alpha) == [ref["alpha"]] and K.unmont(claims.s) == [ref["s"]]
    assert K.unmont(m) == ref["m"] and K.unmont(h_t) == ref["h_t"] and K.unmont(h_f) == ref["h_f"]
    assert proof == ref["proof"]
    assert K.unmont(claims.r_f) == ref["r_f"] and K.unmont(claims.r_t) == ref["r_t"]
    for name in L.CLAIMS:
        assert K.unmont(getattr(claims, name)) == [ref["claims"][name]], name
    res, side, seen = lookup.verify(prover.stmt, proof, K.mont(BIND), K.mont(BIND2))
    assert res.accepted and side == "OUTER" and res.offset == len(proof), res
    for name in ("alpha", "s", "r_f", "r_t") + L.CLAIMS:
        assert np.array_equal(getattr(seen, name), getattr(claims, name)), name
    prover.close()
    d.free()


def uniform_case(n, k, seed):
    """Montgomery images straight from numpy: (f, t, idx) with idx uniform over the table"""
    from provekit_amd.field import random_field

    t = random_field(1 << k, seed).reshape(-1, 4)
    idx = np.random.default_rng(seed).integers(0, 1 << k, size=1 << n, dtype=np.uint32)
    return t[idx], t, idx


def check_helpers(ctx, prover, d, sample=48):
    """begin() on a counted prover: h_f is 1 / (alpha - f) at `sample` seeded places and at every x the gather of h_t's own inverse;
    h_t is m / (alpha - t) at `sample` places, and s is the sum of h_t; then finish() and the host verifier accepts"""
    from provekit_amd import lookup

    n, k = prover.stmt.n, prover.stmt.k
    alpha, hf, ht = prover.begin(d.t, d.idx)
    a = K.unmont(alpha)[0]
    h_f, h_t, m = ctx.download_fe(hf, 1 << n), ctx.download_fe(ht, 1 << k), ctx.download_fe(d.m, 1 << k)
    rng = np.random.default_rng(7)
    for x in sorted(set([0, (1 << n) - 1] + [int(v) for v in rng.integers(0, 1 << n, size=sample)])):
        assert K.unmont(h_f[x])[0] * (a - K.unmont(d.images[0][x])[0]) % P == 1, x
    for y in sorted(set([0, (1 << k) - 1] + [int(v) for v in rng.integers(0, 1 << k, size=sample)])):
        assert K.unmont(h_t[y])[0] * (a - K.unmont(d.images[1][y])[0]) % P == K.unmont(m[y])[0], y
    # every lookup of one entry reads the same element: h_f is constant on each idx class, and equals the sampled class's value
    idx = d.images[2]
    first_of = np.full(1 << k, -1, dtype=np.int64)
    first_of[idx[::-1]] = np.arange((1 << n) - 1, -1, -1)
    assert np.array_equal(h_f, h_f[first_of[idx]])
    proof, claims = prover.finish()
    assert K.unmont(claims.s)[0] == sum(K.unmont(h_t)) % P
    res, _, _ = lookup.verify(prover.stmt, proof)
    assert res.accepted, res


@pytest.mark.parametrize("step", [-1, 0, 1])
@pytest.mark.parametrize("limit", ["gather", "count"])
def test_counts_and_the_gather_are_exact_on_both_sides_of_their_lds_limits(ctx, limit, step):
    """k one below, at and one above the largest table the gather stages in LDS, and the largest table counted in LDS (both read from
    the library), n = 12: 16 lookups per lane of one workgroup, four tiles of either gather kernel"""
    from provekit_amd import lookup

    n, k = 12, (lookup.gather_lds_max_k() if limit == "gather" else lookup.count_lds_max_k()) + step
    f, t, idx = uniform_case(n, k, seed=50 + step)
    d, prover = Device(ctx, k, f, t, idx), make_prover(ctx, n, k, 0, 0)
    prover.multiplicities(d.f, d.t, d.idx, d.m)
    assert K.unmont(ctx.download_fe(d.m, 1 << k)) == np.bincount(idx, minlength=1 << k).tolist()
    check_helpers(ctx, prover, d)
    prover.close()
    d.free()


@pytest.mark.parametrize("k_from_limit", [None, 1])
@pytest.mark.parametrize("skew", ["one bin", "uniform", "duplicates", "unused"])
def test_multiplicities_under_skew_are_numpys_bincount(ctx, skew, k_from_limit):
    """n = 16 on a table of 2^3 (LDS histogram) and on one past the LDS limit (device-memory atomics): every lookup one bin, so one count
    is 2^n; uniform lookups; a table with duplicate values, idx choosing either copy; a table most of whose entries are never used"""
    from provekit_amd import lookup
    from provekit_amd.field import random_field

    n = 16
    k = 3 if k_from_limit is None else lookup.count_lds_max_k() + k_from_limit
    rng = np.random.default_rng(len(skew))
    t = random_field(1 << k, 60).reshape(-1, 4)
    if skew == "one bin":
        idx = np.full(1 << n, (1 << k) - 3, dtype=np.uint32)
    elif skew == "uniform":
        idx = rng.integers(0, 1 << k, size=1 << n, dtype=np.uint32)
    elif skew == "duplicates":
        t[1::2] = t[0::2]
        idx = rng.integers(0, 1 << k, size=1 << n, dtype=np.uint32)
    else:
        idx = rng.integers(0, 3, size=1 << n, dtype=np.uint32) * 2 + 1
    want = np.bincount(idx, minlength=1 << k)
    assert skew != "one bin" or want.max() == 1 << n
    assert skew != "unused" or (want == 0).sum() == (1 << k) - 3
    d, prover = Device(ctx, k, t[idx], t, idx), make_prover(ctx, n, k, 0, 0)
    prover.multiplicities(d.f, d.t, d.idx, d.m)
    assert K.unmont(ctx.download_fe(d.m, 1 << k)) == want.tolist()
    alpha, hf, ht = prover.begin(d.t, d.idx)
    h_t = ctx.download_fe(ht, 1 << k)
    assert not h_t[want == 0].any()  # a count of 0 gives h_t = 0
    proof, claims = prover.finish()
    res, _, _ = lookup.verify(prover.stmt, proof)
    assert res.accepted and K.unmont(claims.s)[0] == sum(K.unmont(h_t)) % P, res
    prover.close()
    d.free()


@pytest.mark.parametrize("n, k", [(12, 11), (9, 13)])
def test_no_bit_depends_on_the_grid(ctx, n, k):
    """grids 1, 2, 7, 300 and the library's own, set through the lab's probe of a prover: m, h_f, h_t, s and the proof.  (12, 11): LDS histogram and LDS-staged gather, two tiles of
    the table kernel, so grids above 2 leave workgroups without a tile; (9, 13): device-memory counts, the gather through L2, eight tiles"""
    from tools.pk_probes import lib as probes

    f, t, idx = uniform_case(n, k, seed=70 + n)
    d, prover = Device(ctx, k, f, t, idx), make_prover(ctx, n, k)
    outs = []
    for grid in (0, 1, 2, 7, 300):
        assert probes.pk_probe_lookup_set_grid(prover.handle, grid) == 0
        outs.append(prove(ctx, prover, d, tables=True))
    for got in outs[1:]:
        assert got[0] == outs[0][0] and np.array_equal(got[1].s, outs[0][1].s)
        for a, b in zip(got[2:], outs[0][2:]):
            assert np.array_equal(a, b)
    assert K.unmont(outs[0][3]) == np.bincount(idx, minlength=1 << k).tolist()
    prover.close()
    d.free()


@pytest.mark.parametrize("n, k", [(8, 8), (10, 13)])
def test_a_failed_validation_names_the_smallest_bad_lookup_and_the_prover_stays_usable(ctx, n, k):
    from provekit_amd._lib import ProveKitHipError

    f, t, idx, ref = reference(n, k)
    last = (1 << n) - 1
    other = K.mont([(f[5] + 1) % P])[0]
    cases = {"idx out of range at 0": ({0: 1 << k}, {}, 0), "idx out of range at the end": ({last: 2**32 - 1}, {}, last),
             "f differs from t[idx]": ({}, {77 % (1 << n): other}, 77 % (1 << n)),
             "several at once": ({last: 1 << k, 9: (1 << k) + 5}, {200 % (1 << n): other, 31: other}, 9)}
    good, prover = Device(ctx, k, f, t, idx), make_prover(ctx, n, k)
    for name, (bad_idx, bad_f, want) in cases.items():
        f_img, idx_arr = K.mont(f), np.asarray(idx, dtype=np.uint32).copy()
        for x, v in bad_idx.items():
            idx_arr[x] = v
        for x, v in bad_f.items():
            f_img[x] = v
        d = Device(ctx, k, f_img, good.images[1], idx_arr)
        with pytest.raises(ProveKitHipError, match=f"lookup {want} fails") as e:
            prover.multiplicities(d.f, d.t, d.idx, d.m)
        assert e.value.code == -6 and prover.first_bad == want, name
        with pytest.raises(ProveKitHipError, match="needs a successful pkl_multiplicities") as e:  # nothing is proved
            prover.begin(d.t, d.idx, K.mont(BIND))
        assert e.value.code == -1
        d.free()
        assert prove(ctx, prover, good)[0] == ref["proof"], name
        assert prover.first_bad is None
    prover.close()
    good.free()


def test_alpha_hitting_the_table_is_refused_with_a_reason_and_another_bind_proves(ctx):
    """alpha depends on the bind elements alone, so the reference names it and the table is built around it: entry 5 IS alpha.  Once with
    the entry looked up and once with it unused (its denominator is zero all the same)"""
    from provekit_amd._lib import ProveKitHipError

    n, k = 6, 4
    alpha = L.alpha_of(n, k, BIND, n_bind2=len(BIND2))
    for used in (True, False):
        f, t, idx = L.random_case(n, k, seed=80)
        t[5] = alpha
        idx = [i if (i != 5 or used) else 6 for i in idx]
        idx[3] = 5 if used else idx[3]
        f = [t[i] for i in idx]
        d, prover = Device(ctx, k, f, t, idx), make_prover(ctx, n, k)
        prover.multiplicities(d.f, d.t, d.idx, d.m)
        with pytest.raises(ProveKitHipError, match="alpha is an entry of t") as e:
            prover.begin(d.t, d.idx, K.mont(BIND))
        assert e.value.code == -6
        with pytest.raises(ProveKitHipError, match="needs a successful pkl_begin"):
            prover.finish(K.mont(BIND2))
        other = [BIND[0], (BIND[1] + 1) % P]
        alpha2, hf, ht = prover.begin(d.t, d.idx, K.mont(other))  # the counts are still good
        proof, _ = prover.finish(K.mont(BIND2))
        assert proof == L.prove(n, k, f, t, idx, other, BIND2)["proof"]
        prover.close()
        d.free()


def test_the_callers_tables_are_unchanged_and_a_prover_proves_again_the_same(ctx):
    n, k = 9, 4
    f, t, idx, ref = reference(n, k)
    d, prover = Device(ctx, k, f, t, idx), make_prover(ctx, n, k)
    first = prove(ctx, prover, d)[0]
    assert np.array_equal(ctx.download_fe(d.f, 1 << n), d.images[0]) and np.array_equal(ctx.download_fe(d.t, 1 << k), d.images[1])
    assert np.array_equal(ctx.download(d.idx, (1 << n,), np.uint32), d.images[2])
    assert first == prove(ctx, prover, d)[0] == ref["proof"]
    prover.close()
    d.free()


def test_the_order_of_the_calls_and_a_short_proof_buffer(ctx):
    from provekit_amd import lookup
    from provekit_amd._lib import ProveKitHipError

    n, k = 8, 8
    f, t, idx, ref = reference(n, k)
    d, prover = Device(ctx, k, f, t, idx), make_prover(ctx, n, k)
    with pytest.raises(ProveKitHipError, match="needs a successful pkl_multiplicities"):
        prover.begin(d.t, d.idx, K.mont(BIND))
    with pytest.raises(ProveKitHipError, match="needs a successful pkl_begin"):
        prover.finish(K.mont(BIND2))
    prover.multiplicities(d.f, d.t, d.idx, d.m)
    with pytest.raises(ProveKitHipError, match="not the ones pkl_multiplicities validated"):
        prover.begin(d.t, d.f, K.mont(BIND))
    prover.begin(d.t, d.idx, K.mont(BIND))
    for cap in (0, len(ref["proof"]) - 1):
        with pytest.raises(ProveKitHipError, match="proof buffer") as e:
            prover.finish(K.mont(BIND2), capacity=cap)
        assert e.value.code == -1 and prover.last_len == len(ref["proof"]) == lookup.proof_bytes(prover.stmt)
    assert prover.finish(K.mont(BIND2), capacity=len(ref["proof"]) + 100)[0] == ref["proof"]
    with pytest.raises(ProveKitHipError, match="needs a successful pkl_begin"):  # a proof ends its begin
        prover.finish(K.mont(BIND2))
    prover.close()
    d.free()


def test_composition_with_the_commitment_scheme_and_the_provided_contract(ctx):
    """n = 12, k = 8: commit f, t, m; begin; commit h_f, h_t; finish.  The seven claims are pkw_evaluate of the actual tables, and every
    opening verifies against pkl_verify's claims (h_f at two points in one opening).  Then the PROVIDED contract: a proof the Python
    reference makes for an f with a non-member, validation skipped, is accepted by pkl_verify -- and its claim about h_f at the
    all-halves point is NOT what the committed h_f evaluates to, which is where the opening would fail"""
    import whir_pcs_cases as W
    from provekit_amd import lookup, whir_pcs

    n, k = 12, 8
    f, t, idx = L.random_case(n, k, seed=90)
    d = Device(ctx, k, f, t, idx)
    cfg_n, cfg_k = W.small_config(n, 1), W.small_config(k, 1)
    scheme_n, scheme_k = whir_pcs.Scheme(ctx, cfg_n), whir_pcs.Scheme(ctx, cfg_k)
    prover = lookup.LookupProver(ctx, lookup.Statement(n, k, 3, 2))
    prover.multiplicities(d.f, d.t, d.idx, d.m)
    com = {"f": scheme_n.commit([d.f]), "t": scheme_k.commit([d.t]), "m": scheme_k.commit([d.m])}
    as_fe = lambda c: int.from_bytes(c.root(), "little")  # noqa: E731
    bind = K.mont([as_fe(com[name]) for name in ("f", "t", "m")])
    alpha, hf, ht = prover.begin(d.t, d.idx, bind)
    com["h_f"], com["h_t"] = scheme_n.commit([hf]), scheme_k.commit([ht])
    bind2 = K.mont([as_fe(com["h_f"]), as_fe(com["h_t"])])
    proof, claims = prover.finish(bind2)
    res, side, seen = lookup.verify(prover.stmt, proof, bind, bind2)
    assert res.accepted and side == "OUTER", res

    half_n, half_k = K.mont([L.INV2] * n), K.mont([L.INV2] * k)
    at_f, at_t = np.stack([seen.r_f, half_n]), np.stack([seen.r_t, half_k])
    ev_n = whir_pcs.evaluate(ctx, [d.f, hf], n, at_f)
    ev_k = whir_pcs.evaluate(ctx, [d.t, d.m, ht], k, at_t)
    actual = {"f_at_rf": ev_n[0, 0], "hf_at_rf": ev_n[1, 0], "hf_at_half": ev_n[1, 1], "t_at_rt": ev_k[0, 0], "m_at_rt": ev_k[1, 0], "ht_at_rt": ev_k[2, 0],
              "ht_at_half": ev_k[2, 1]}
    for name in L.CLAIMS:
        assert np.array_equal(getattr(seen, name), actual[name]) and np.array_equal(getattr(claims, name), actual[name]), name
    openings = [("f", scheme_n, cfg_n, at_f[:1], ["f_at_rf"]), ("h_f", scheme_n, cfg_n, at_f, ["hf_at_rf", "hf_at_half"]), ("t", scheme_k, cfg_k, at_t[:1], ["t_at_rt"]),
                ("m", scheme_k, cfg_k, at_t[:1], ["m_at_rt"]), ("h_t", scheme_k, cfg_k, at_t, ["ht_at_rt", "ht_at_half"])]
    for name, scheme, cfg, points, claimed in openings:
        evals, opening = scheme.open(com[name], points)
        wres, wevals = whir_pcs.verify(cfg, points, opening, expected_root=com[name].root())
        assert wres.accepted, (name, wres)
        for q, claim in enumerate(claimed):
            assert np.array_equal(wevals[0, q], getattr(seen, claim)) and np.array_equal(evals[0, q], getattr(seen, claim)), claim
    # another root: other challenges, rejected
    res, side, _ = lookup.verify(prover.stmt, proof, K.mont([as_fe(com["t"]), as_fe(com["f"]), as_fe(com["m"])]), bind2)
    assert not res.accepted and side in ("F", "T")

    # a non-member at x = 7: the device refuses it ...
    from provekit_amd._lib import ProveKitHipError

    bad_f = list(f)
    bad_f[7] = (max(t) + 1) % P if (max(t) + 1) % P not in t else 12345
    bad = Device(ctx, k, bad_f, t, idx)
    with pytest.raises(ProveKitHipError, match="lookup 7 fails"):
        prover.multiplicities(bad.f, bad.t, bad.idx, bad.m)
    # ... the reference prover does not, and the verifier accepts its proof: accepted PROVIDED the claims hold, and one does not
    ref = L.prove(n, k, bad_f, t, idx, K.unmont(bind), K.unmont(bind2), validate=False)
    res, side, lied = lookup.verify(prover.stmt, ref["proof"], bind, bind2)
    assert res.accepted, res
    d_hf = ctx.upload(K.mont(ref["h_f"]))
    ev = whir_pcs.evaluate(ctx, [bad.f, d_hf], n, np.stack([lied.r_f, half_n]))
    assert np.array_equal(lied.f_at_rf, ev[0, 0]) and np.array_equal(lied.hf_at_rf, ev[1, 0])
    assert not np.array_equal(lied.hf_at_half, ev[1, 1])
    assert K.unmont(lied.ht_at_half) == [L.mle_at(ref["h_t"], [L.INV2] * k)]
    for b in (d_hf,):
        b.free()
    for c in com.values():
        c.close()
    prover.close()
    scheme_n.close()
    scheme_k.close()
    bad.free()
    d.free()


def test_the_cpp_demo_commits_proves_opens_every_claim_and_sees_the_error_paths():
    import subprocess

    demo = os.path.join(ROOT, "examples", "lookup_pcs_demo")
    assert os.path.exists(demo), "examples/lookup_pcs_demo is built by __graft_entry__.build()"
    out = subprocess.run(["timeout", "-k", "10", "120", demo, "12", "8", "7"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("ok n=12 k=8 lookup_bytes=%d " % L.proof_bytes(12, 8))
    assert lines[1].startswith("non-member entry: refused at x=%d " % (4096 // 3)) and "lookup %d fails" % (4096 // 3) in lines[1]
    assert "rejected, side=1 check=ROUND" in lines[2] and "round 0:" in lines[2] and "another root: rejected" in lines[3]
