"""GPU: libprovekit_tuplelookup.so on the device.  The leaf kernel bit-exact against Python ints across one workgroup's sweep, for every
width, group count and several grids; the count kernel's multiplicities and the smallest failing stacked index on both sides of its LDS
limit; the proof bytes and claims against the Python reference (tests/tuplelookup_refs.py); a prover reused, a short buffer, the three
unsatisfied cases with their reasons; one larger size against pkw_evaluate; the composition with libprovekit_whir.so; the C++ example."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import prodcheck_refs as K  # noqa: E402
import tuplelookup_refs as T  # noqa: E402

pytestmark = pytest.mark.gpu
P = K.P
BIND = K.random_elements(3, seed=43)
GRIDS = (1, 3, 0)  # workgroups per group (0: the library's rule)
VALUES = ("random", "all p-1", "all 0", "zero leaf")
BETAS = ("0", "1", "p-1", "random")
SENTINEL = 0xA5


def pointers(bufs):
    return (C.c_void_p * len(bufs))(*[b.ptr for b in bufs])


def sweep(n):
    """an int, or "s-1", "s", "s+1": around 2^s rows, one workgroup's sweep of the leaf kernel at the shipped rows per lane"""
    if isinstance(n, int):
        return n
    from tools.pk_probes import lib as probes

    rows = 256 * probes.pk_probe_tuple_leaf_items()
    assert rows & (rows - 1) == 0
    return rows.bit_length() - 1 + int(n[1:] or 0)


def leaf_case(n, w, c, values, beta_kind, seed):
    """(groups, alpha, beta): c groups of w columns of 2^n canonical ints"""
    import random

    rng = random.Random(seed)
    beta = {"0": 0, "1": 1, "p-1": P - 1, "random": rng.randrange(P)}[beta_kind]
    alpha = rng.randrange(P)
    fill = {"all p-1": P - 1, "all 0": 0}.get(values)
    groups = [[[rng.randrange(P) if fill is None else fill for _ in range(1 << n)] for _ in range(w)] for _ in range(c)]
    if values == "zero leaf":  # alpha is one compressed row: the last row of the last group
        alpha = T.compress(groups[c - 1], (1 << n) - 1, beta)
    return groups, alpha, beta


def check_leaves(ctx, n, w, c, values, beta_kind, seed):
    from tools.pk_probes import lib as probes
    from provekit_amd import tuplelookup as tl

    groups, alpha, beta = leaf_case(n, w, c, values, beta_kind, seed)
    want = K.mont(T.leaves(groups, alpha, beta))
    if values == "zero leaf":
        assert not want[-1].any()
    images = [K.mont(col) for cols in groups for col in cols]
    bufs = [ctx.upload(im) for im in images]
    rows = c << n
    d_leaf = ctx.alloc_fe(rows + 1)
    a, b = K.mont([alpha]), K.mont([beta])
    ctx.zero(d_leaf, 32 * (rows + 1))
    tl.leaves(ctx, n, w, c, [bufs[g * w : (g + 1) * w] for g in range(c)], a, b, d_leaf)  # the C ABI's entry: the library's grid
    got = ctx.download_fe(d_leaf, rows + 1)
    assert np.array_equal(got[:rows], want) and not got[rows].any()  # and nothing past the end
    for grid in GRIDS:
        ctx.zero(d_leaf, 32 * (rows + 1))
        assert probes.pk_probe_tuple_leaves(ctx.handle, n, w, c, pointers(bufs), a.ctypes.data, b.ctypes.data, d_leaf.ptr, grid, None) == 0
        got = ctx.download_fe(d_leaf, rows + 1)
        assert np.array_equal(got[:rows], want) and not got[rows].any(), grid
    for buf, im in zip(bufs, images):  # the caller's columns are unchanged
        assert ctx.download_fe(buf, 1 << n).tobytes() == im.tobytes()
        buf.free()
    d_leaf.free()


SHAPES = list(itertools.product((1, 3, "s-1", "s", "s+1"), (1, 2, 3, 4), (1, 2, 4)))
KINDS = list(itertools.product(VALUES, BETAS))


# Every (n, w, c) with every grid; the 16 (values, beta) kinds go round over the 60 shapes, so each kind meets three or four shapes, and
# the next test crosses all 16 at one shape: the kernel's paths depend on the shape (tile edges, the group's offset, W) and never on
# the values, whose edge cases are the field arithmetic's.
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=lambda i: "n%s-w%d-c%d-%s-beta %s" % (SHAPES[i] + KINDS[i % len(KINDS)]))
def test_the_leaf_kernel_is_bit_exact_for_every_width_group_count_and_grid(ctx, i):
    (n, w, c), (values, beta_kind) = SHAPES[i], KINDS[i % len(KINDS)]
    check_leaves(ctx, sweep(n), w, c, values, beta_kind, seed=i)


@pytest.mark.parametrize("values, beta_kind", KINDS)
def test_the_leaf_kernel_is_bit_exact_for_every_kind_of_values_and_beta(ctx, values, beta_kind):
    check_leaves(ctx, 3, 4, 2, values, beta_kind, seed=77)


def raw_columns(count, rows, seed):
    """stored words below p, and no field arithmetic: the count kernel compares words"""
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, 2**63, size=(count, rows, 4), dtype=np.uint64)
    cols[:, :, 3] >>= np.uint64(8)  # below p
    return cols


class CountCase:
    """c groups of w columns that are rows idx[g][x] of a table of 2^k rows, on the device"""

    def __init__(self, ctx, n, k, w, c, skew, seed=0):
        self.ctx, self.n, self.k, self.w, self.c = ctx, n, k, w, c
        rng = np.random.default_rng(100 * n + k + seed)
        self.t = raw_columns(w, 1 << k, seed=k)
        self.idx = np.full((c, 1 << n), (1 << k) - 1, dtype=np.uint32) if skew else rng.integers(0, 1 << k, size=(c, 1 << n), dtype=np.uint32)
        self.f = np.stack([self.t[:, self.idx[g]] for g in range(c)])  # [c, w, 2^n, 4]
        self.d_t = [ctx.upload(self.t[j]) for j in range(w)]
        self.d_f = [[ctx.upload(self.f[g, j]) for j in range(w)] for g in range(c)]
        self.d_idx = [ctx.upload(self.idx[g]) for g in range(c)]
        self.d_m = ctx.alloc_fe(1 << k)

    def counts(self):
        return np.bincount(self.idx.reshape(-1), minlength=1 << self.k)

    def free(self):
        for buf in self.d_t + [b for cols in self.d_f for b in cols] + self.d_idx + [self.d_m]:
            buf.free()


def lds_k(k):
    from provekit_amd import tuplelookup as tl

    return k if isinstance(k, int) else tl.count_lds_max_k() + int(k[1:] or 0)


@pytest.mark.parametrize("skew", [False, True], ids=["uniform", "full skew"])
@pytest.mark.parametrize("c", [1, 4])
@pytest.mark.parametrize("w", [1, 4])
@pytest.mark.parametrize("n", [1, 5, 7, 12])
@pytest.mark.parametrize("k", [1, "L", "L+1"])
def test_the_count_kernel_gives_the_python_count_for_every_grid(ctx, k, n, w, c, skew):
    from tools.pk_probes import lib as probes
    from provekit_amd import tuplelookup as tl

    k = lds_k(k)
    case = CountCase(ctx, n, k, w, c, skew)
    want = K.mont([int(v) for v in case.counts()])
    prover = tl.Prover(ctx, tl.Statement(n, k, w, c))
    for grid in GRIDS:
        assert probes.pk_probe_tuple_set_grid(prover.handle, grid) == 0
        ctx.zero(case.d_m, 32 << k)
        prover.multiplicities(case.d_f, case.d_t, case.d_idx, case.d_m)
        assert prover.first_bad == tl.NO_BAD_ROW
        assert np.array_equal(ctx.download_fe(case.d_m, 1 << k), want), grid
    prover.close()
    case.free()


FAILURES = ("an index of 2^k", "an index of 2^32-1", "column w-1", "group c-1", "x = 0", "x = 2^n-1", "two rows")


@pytest.mark.parametrize("failure", FAILURES)
@pytest.mark.parametrize("k, n, w, c", [(1, 5, 4, 4), ("L", 7, 4, 4), ("L+1", 12, 4, 4), ("L", 5, 1, 1)])
def test_a_failing_row_is_reported_as_the_smallest_stacked_index(ctx, k, n, w, c, failure):
    from provekit_amd import tuplelookup as tl
    from provekit_amd._lib import ProveKitHipError

    k = lds_k(k)
    case = CountCase(ctx, n, k, w, c, skew=False, seed=5)
    rows, mid = 1 << n, (1 << n) // 2 + 1

    def break_index(g, x, value):
        idx = case.idx[g].copy()
        idx[x] = value
        ctx.upload_into(case.d_idx[g].ptr, idx)

    def break_column(g, j, x):
        col = case.f[g, j].copy()
        col[x, 3] ^= np.uint64(1)  # the last stored word of the row's column differs
        ctx.upload_into(case.d_f[g][j].ptr, col)

    if failure == "an index of 2^k":
        break_index(c - 1, mid, 1 << k)
        want = (c - 1) * rows + mid
    elif failure == "an index of 2^32-1":
        break_index(0, mid, 2**32 - 1)
        want = mid
    elif failure == "column w-1":
        break_column(0, w - 1, mid)
        want = mid
    elif failure == "group c-1":
        break_column(c - 1, 0, mid)
        want = (c - 1) * rows + mid
    elif failure == "x = 0":
        break_column(c - 1, 0, 0)
        want = (c - 1) * rows
    elif failure == "x = 2^n-1":
        break_column(0, w - 1, rows - 1)
        want = rows - 1
    else:  # the smaller of two, across groups and kinds of failure
        break_column(c - 1, w - 1, 3)
        break_index(0, rows - 2, 1 << k)
        want = min((c - 1) * rows + 3, rows - 2)
    prover = tl.Prover(ctx, tl.Statement(n, k, w, c))
    with pytest.raises(ProveKitHipError, match="stacked index %d " % want) as e:
        prover.multiplicities(case.d_f, case.d_t, case.d_idx, case.d_m)
    assert e.value.code == tl.ERR_UNSATISFIED and prover.first_bad == want
    prover.close()
    case.free()


class Proved:
    """one statement's columns on the device, with the reference's proof; computed once per statement and shared, never changed"""

    def __init__(self, ctx, n, k, w, c, n_bind=3):
        self.size, self.bind = (n, k, w, c), BIND[:n_bind]
        self.f, self.t, self.m, self.idx = T.random_case(n, k, w, c, seed=1000 * n + 100 * k + 10 * w + c)
        self.ref = T.prove(n, k, self.f, self.t, self.m, self.bind)
        self.d_f = [[ctx.upload(K.mont(col)) for col in cols] for cols in self.f]
        self.d_t = [ctx.upload(K.mont(col)) for col in self.t]
        self.d_idx = [ctx.upload(np.asarray(i, dtype=np.uint32)) for i in self.idx]
        self.d_m = ctx.alloc_fe(1 << k)

    def free(self):
        for buf in [b for cols in self.d_f for b in cols] + self.d_t + self.d_idx + [self.d_m]:
            buf.free()


def same_claims(claims, ref):
    for name in ("alpha", "beta", "f_value", "t_value", "m_value"):
        assert K.unmont(getattr(claims, name)) == [ref[name]], name
    assert K.unmont(claims.z_lo) == ref["z_lo"] and K.unmont(claims.z_t) == ref["z_t"] and K.unmont(claims.t_coeff) == ref["t_coeff"]
    assert [K.unmont(row) for row in claims.f_coeff] == ref["f_coeff"]


@pytest.mark.parametrize("size", [(1, 1, 1, 1), (3, 2, 2, 1), (4, 3, 3, 4), (6, 4, 4, 2), (2, 6, 2, 4)])
def test_proof_bytes_and_claims_are_the_references_and_a_prover_proves_twice(ctx, size):
    from provekit_amd import tuplelookup as tl

    n, k, w, c = size
    case = Proved(ctx, *size)
    stmt = tl.Statement(n, k, w, c, 3)
    prover = tl.Prover(ctx, stmt)
    prover.multiplicities(case.d_f, case.d_t, case.d_idx, case.d_m)
    assert K.unmont(ctx.download_fe(case.d_m, 1 << k)) == case.m
    bind = K.mont(case.bind)
    proof, claims = prover.prove(case.d_f, case.d_t, case.d_m, bind)
    assert proof == case.ref["proof"] and len(proof) == tl.proof_bytes(stmt)
    same_claims(claims, case.ref)
    res, side, layer, seen = tl.verify(stmt, proof, bind)
    assert res.accepted and res.offset == len(proof), res
    same_claims(seen, case.ref)
    again, _ = prover.prove(case.d_f, case.d_t, case.d_m, bind)  # the same prover, the same bytes
    assert again == proof
    # a short buffer: the length is told, nothing is proved or written, the prover stays usable
    from provekit_amd._lib import ProveKitHipError

    prover.fill = SENTINEL
    with pytest.raises(ProveKitHipError, match="the proof buffer holds") as e:
        prover.prove(case.d_f, case.d_t, case.d_m, bind, capacity=len(proof) - 1)
    assert e.value.code == -1 and prover.last_len == len(proof) and bytes(prover.buffer) == bytes([SENTINEL]) * (len(proof) - 1)
    assert prover.prove(case.d_f, case.d_t, case.d_m, bind)[0] == proof
    for cols, bufs in zip(case.f + [case.t], case.d_f + [case.d_t]):  # the caller's columns are unchanged
        for col, buf in zip(cols, bufs):
            assert ctx.download_fe(buf, len(col)).tobytes() == K.mont(col).tobytes()
    prover.close()
    case.free()


def test_a_row_outside_t_a_wrong_m_and_alpha_on_a_row_are_unsatisfied_and_name_the_case(ctx):
    from provekit_amd import tuplelookup as tl
    from provekit_amd._lib import ProveKitHipError

    size = n, k, w, c = 4, 3, 3, 2
    case = Proved(ctx, *size)
    stmt, bind = tl.Statement(n, k, w, c, 3), K.mont(case.bind)
    prover = tl.Prover(ctx, stmt)
    prover.fill = SENTINEL
    d_m = ctx.upload(K.mont(case.m))
    honest, _ = prover.prove(case.d_f, case.d_t, d_m, bind)
    assert honest == case.ref["proof"]

    def refused(d_f, d_t, d_m_, reason):
        with pytest.raises(ProveKitHipError, match=reason) as e:
            prover.prove(d_f, d_t, d_m_, bind)
        assert e.value.code == tl.ERR_UNSATISFIED
        assert bytes(prover.buffer) == bytes([SENTINEL]) * len(honest)  # nothing is written
        assert prover.prove(case.d_f, case.d_t, d_m, bind)[0] == honest  # and the next honest proof succeeds

    # one row outside t (group 1, row 5), m otherwise honest
    have = set(T.rows(case.t))
    row = next(r for r in (tuple((v + d) % P for v in T.rows(case.t)[0]) for d in range(1, 9)) if r not in have)
    outside = [[list(col) for col in cols] for cols in case.f]
    for j in range(w):
        outside[1][j][5] = row[j]
    d_out = [case.d_f[0], [ctx.upload(K.mont(col)) for col in outside[1]]]
    refused(d_out, case.d_t, d_m, r"a row is not in t: stacked index %d \(group 1, row 5\)" % (16 + 5))
    # m off by one in one bin
    wrong = list(case.m)
    wrong[2] += 1
    d_wrong = ctx.upload(K.mont(wrong))
    refused(case.d_f, case.d_t, d_wrong, "m is wrong")
    # alpha forced onto a row: alpha and beta depend on the statement and the bind elements alone, so the row is chosen after them
    alpha, beta, _ = T.challenges(n, k, w, c, case.bind)
    hit = [list(col) for col in case.t]
    y = case.idx[0][0]  # a row of t that f uses: both sides have the zero denominator
    hit[0][y] = (alpha - sum(pow(beta, j, P) * hit[j][y] for j in range(1, w))) % P
    assert T.compress(hit, y, beta) == alpha
    f_hit = [[[hit[j][i] for i in case.idx[g]] for j in range(w)] for g in range(c)]
    d_t_hit = [ctx.upload(K.mont(col)) for col in hit]
    d_f_hit = [[ctx.upload(K.mont(col)) for col in cols] for cols in f_hit]
    refused(d_f_hit, d_t_hit, d_m, "a denominator is zero: alpha is a compressed row of f")
    refused(case.d_f, d_t_hit, d_m, "a denominator is zero: alpha is a compressed row of t")  # in t alone (f's rows are then outside, seen later)
    for buf in d_out[1] + [d_wrong, d_m] + d_t_hit + [b for cols in d_f_hit for b in cols]:
        buf.free()
    prover.close()
    case.free()


def small_images(ctx, columns):
    """device columns of small canonical integers, converted to Montgomery form on the device"""
    from provekit_amd._lib import lib as product

    out = []
    for col in columns:
        limbs = np.zeros((len(col), 4), dtype=np.uint64)
        limbs[:, 0] = col
        buf = ctx.upload(limbs)
        assert product.pk_fe_to_mont(ctx.handle, buf.ptr, buf.ptr, len(col)) == 0
        out.append(buf)
    return out


def test_one_larger_lookup_is_verified_and_its_claims_hold_of_the_columns_evaluations(ctx):
    """n = 14, k = 10, w = 3, c = 2: nothing is proved in Python at this size"""
    from provekit_amd import tuplelookup as tl, whir_pcs

    n, k, w, c = 14, 10, 3, 2
    rng = np.random.default_rng(14)
    y = np.arange(1 << k, dtype=np.uint64)
    t = [y >> np.uint64(5), y & np.uint64(31), (y >> np.uint64(5)) ^ (y & np.uint64(31))]  # (a, b, a XOR b) over 5-bit operands
    idx = rng.integers(0, 1 << k, size=(c, 1 << n), dtype=np.uint32)
    d_t = small_images(ctx, t)
    d_f = [small_images(ctx, [col[idx[g]] for col in t]) for g in range(c)]
    d_idx, d_m = [ctx.upload(idx[g]) for g in range(c)], ctx.alloc_fe(1 << k)
    stmt = tl.Statement(n, k, w, c)
    prover = tl.Prover(ctx, stmt)
    prover.multiplicities(d_f, d_t, d_idx, d_m)
    assert K.unmont(ctx.download_fe(d_m, 1 << k)) == [int(v) for v in np.bincount(idx.reshape(-1), minlength=1 << k)]
    proof, claims = prover.prove(d_f, d_t, d_m)
    assert len(proof) == tl.proof_bytes(stmt)
    res, side, layer, seen = tl.verify(stmt, proof)
    assert res.accepted and res.offset == len(proof), res
    for name in ("alpha", "beta", "z_lo", "z_t", "f_coeff", "t_coeff", "f_value", "t_value", "m_value"):
        assert np.array_equal(getattr(seen, name), getattr(claims, name)), name
    f_evals = np.stack([whir_pcs.evaluate(ctx, d_f[g], n, seen.z_lo[None])[:, 0] for g in range(c)])  # [c, w, 4]
    tm = whir_pcs.evaluate(ctx, d_t + [d_m], k, seen.z_t[None])[:, 0]
    assert tl.check_claims(stmt, seen, f_evals, tm[:w], tm[w]) == "NONE"
    changed = f_evals.copy()
    changed[1, 2] = K.mont([(K.unmont(changed[1, 2])[0] + 1) % P])[0]
    assert tl.check_claims(stmt, seen, changed, tm[:w], tm[w]) == "F"
    prover.close()
    for buf in d_t + [b for cols in d_f for b in cols] + d_idx + [d_m]:
        buf.free()


def test_composition_with_the_commitment_scheme(ctx):
    """commit each group and {t.., m}, bind the roots, prove, open every group at z_lo and the table's columns at z_T, verify the
    openings, check the claims on the opened values; with one evaluation changed the claims fail"""
    import whir_pcs_cases as W
    from provekit_amd import tuplelookup as tl, whir_pcs

    n, k, w, c = 10, 6, 2, 2
    case = Proved(ctx, n, k, w, c, n_bind=0)
    d_m = ctx.upload(K.mont(case.m))
    cfg_n, cfg_k = W.small_config(n, w), W.small_config(k, w + 1)
    scheme_n, scheme_k = whir_pcs.Scheme(ctx, cfg_n), whir_pcs.Scheme(ctx, cfg_k)
    coms = [scheme_n.commit(case.d_f[g]) for g in range(c)]
    com_t = scheme_k.commit(case.d_t + [d_m])
    bind = K.mont([int.from_bytes(com.root(), "little") for com in coms + [com_t]])
    stmt = tl.Statement(n, k, w, c, c + 1)
    prover = tl.Prover(ctx, stmt)
    proof, _ = prover.prove(case.d_f, case.d_t, d_m, bind)
    res, side, layer, seen = tl.verify(stmt, proof, bind)
    assert res.accepted, res
    f_evals = []
    for com in coms:
        _, opening = scheme_n.open(com, seen.z_lo[None])
        wres, wevals = whir_pcs.verify(cfg_n, seen.z_lo[None], opening, expected_root=com.root())
        assert wres.accepted, wres
        f_evals.append(wevals[:, 0])
    _, opening = scheme_k.open(com_t, seen.z_t[None])
    wres, wevals = whir_pcs.verify(cfg_k, seen.z_t[None], opening, expected_root=com_t.root())
    assert wres.accepted, wres
    f_evals, tm = np.stack(f_evals), wevals[:, 0]
    assert tl.check_claims(stmt, seen, f_evals, tm[:w], tm[w]) == "NONE"
    for which, at in (("F", (0, 1, 1)), ("T", (1, 0)), ("M", (1, w))):
        fe, te = f_evals.copy(), tm.copy()
        target = fe if which == "F" else te
        target[at[1:]] = K.mont([(K.unmont(target[at[1:]])[0] + 1) % P])[0]
        assert tl.check_claims(stmt, seen, fe, te[:w], te[w]) == which
    # other roots: another alpha, beta and other seeds, rejected at the first layer of side F
    res, side, layer, _ = tl.verify(stmt, proof, K.mont([1, 2, 3]))
    assert (res.check, side, layer) == ("SUM", "F", 1)
    for closing in coms + [com_t, prover, scheme_n, scheme_k]:
        closing.close()
    d_m.free()
    case.free()


def test_the_cpp_demo_commits_proves_opens_checks_the_claims_and_sees_a_row_outside_refused():
    demo = os.path.join(ROOT, "examples", "tuplelookup_pcs_demo")
    assert os.path.exists(demo), "examples/tuplelookup_pcs_demo is built by __graft_entry__.build()"
    out = subprocess.run(["timeout", "-k", "10", "120", demo, "10", "7"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("ok n=10 k=8 w=3 c=2 proof_bytes=%d " % T.proof_bytes(10, 8, 3, 2)) and "claims=hold" in lines[0]
    assert lines[1].startswith("one row outside the table: refused rc=-6") and "a row is not in t" in lines[1]
