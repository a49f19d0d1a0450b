"""GPU parity of every pass plan of the NTT and the RS-encode (ntt.hip ntt_plan / ntt_columns_in / rs_encode_x): a Python mirror of
the plan classifies each case, and an import-time check makes sure the grids below reach every plan class the device code can take up
to 2^20 rows.  Operands are uniform random, closed forms (impulses, constants, alternating signs, computed with Python integers) and
the extremes of the limb representation; results are compared with the CPU oracle and, where a closed form exists, with it as well.
Also: the fused loads and the stores touch nothing outside their data, and the device's shared twiddle tables survive the context
that built them and are rebuilt after the device's last context is gone."""
import os
import subprocess
import sys
import tempfile
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BT = 4  # ntt.hip: columns per tile of the single-pass kernel
PRE_MAX_TERMS = 3


# ---- a mirror of ntt.hip's plan -------------------------------------------------------------------------------------------------
def pass_is_fast(log_r, log_v, n):
    return log_r >= 3 and log_v < 62 and log_v >= 11 - log_r and n >= 8


def ntt_plan(log_n, nonzero):
    """ntt_plan for log_n > 9: pass radices (log2), pass 1's row stride, L1 and whether pass 1 is folded into pass 2's load"""
    n = 1 << log_n
    if log_n <= 18:
        l1 = (log_n + 1) // 2
        radices = (l1, log_n - l1)
        fast = (pass_is_fast(radices[0], radices[1], n), pass_is_fast(radices[1], radices[0], n))
    else:
        l1 = (log_n + 2) // 3
        l2 = (log_n - l1 + 1) // 2
        radices = (l1, l2, log_n - l1 - l2)
        fast = (pass_is_fast(l1, l2 + radices[2], n), pass_is_fast(l2, radices[2], n), pass_is_fast(radices[2], l1, n))
    stride1 = n >> radices[0]
    L1 = max(1, (min(nonzero, n) + stride1 - 1) // stride1)
    return dict(radices=radices, fast=fast, stride1=stride1, L1=L1, pre=L1 <= PRE_MAX_TERMS and fast[1])


def scaled_available(log_n):
    if log_n <= 9 or log_n > 27:
        return False
    r = ntt_plan(log_n, 1 << log_n)["radices"]
    return pass_is_fast(r[0], r[1], 1 << log_n) if len(r) == 2 else pass_is_fast(r[1], r[2], 1 << log_n)


def reads_polys(log_n, nonzero):
    if log_n <= 9:
        return False
    q = ntt_plan(log_n, nonzero)
    return q["pre"] or q["fast"][0]


def row_strides(log_n):
    """natural-index distances between the rows of each pass's DFT (1 for the last pass)"""
    if log_n <= 9:
        return [1]
    r = ntt_plan(log_n, 1 << log_n)["radices"]
    return [1 << sum(r[i + 1:]) for i in range(len(r))]


def plan_class(kind, log_n, nonzero, ncols):
    """the code path a transform takes: kind ("ntt": pk_ntt, "enc": pk_rs_encode, whose columns may be read in place), passes,
    which of the launched passes run the register-radix kernel, pass 1 folded away (L1), leftover single-pass columns, fused input
    and whether the size has the hash-ready output"""
    if log_n <= 9:
        return (kind, 1, "l", 0, ncols % BT != 0, False, False)
    q = ntt_plan(log_n, nonzero)
    fast = q["fast"][1:] if q["pre"] else q["fast"]
    pre = q["L1"] if q["pre"] else 0
    fused = kind == "enc" and reads_polys(log_n, nonzero)
    return (kind, len(q["radices"]), "".join("f" if f else "l" for f in fast), pre, False, fused, scaled_available(log_n))


def class_id(c):
    kind, npass, fast, pre, left, fused, hr = c
    s = "%s-%dp-%s" % (kind, npass, fast)
    if pre:
        s += "-pre%d" % pre
    if left:
        s += "-leftover"
    if fused:
        s += "-fused"
    if hr:
        s += "-hr"
    return s


def reachable_classes(max_log=20):
    out = set()
    for log_n in range(max_log + 1):
        for ncols in (1, 4):
            out.add(plan_class("ntt", log_n, 1 << log_n, ncols))
            for a in range(log_n + 1):
                out.add(plan_class("enc", log_n, 1 << a, ncols))
    return out


# ---- the grids --------------------------------------------------------------------------------------------------------------------
# pk_ntt at every size up to 2^20 (2^21..2^23 are in test_gpu_large.py): full tiles and leftover columns of the single pass
NTT_GRID = [(log_n, ncols) for log_n in range(21) for ncols in ((1, 3, 4, 5, 7) if log_n <= 9 else (1, 3))]


def ntt_case_id(log_n, ncols):
    return "%s-n%d-c%d" % (class_id(plan_class("ntt", log_n, 1 << log_n, ncols)), log_n, ncols)


def nonzero_for(lr, l1_tag):
    """L = coefficients per column giving L1 = 1, 2 or 4 nonzero rows of pass 1 (the single pass has no such rows: 1, 2^(lr/2), N/2)"""
    if lr <= 9:
        return {1: 1, 2: 1 << (lr // 2), 4: 1 << (lr - 1)}[l1_tag]
    return ntt_plan(lr, 1 << lr)["stride1"] * l1_tag


MAX_ELEMS = 1 << 21  # batch * 2^fold * rows: keeps the oracle cheap


def encode_grid():
    out = []
    for fold in (0, 1, 2, 3, 4, 5, 8):
        for batch in (1, 2, 3, 16):
            for lr in (6, 8, 9, 10, 11, 14, 18, 19):
                if (batch << (fold + lr)) > MAX_ELEMS:
                    continue
                for tag in (1, 2, 4):
                    L = nonzero_for(lr, tag)
                    n_vars = fold + L.bit_length() - 1
                    rho = lr - (L.bit_length() - 1)
                    assert rho >= 1
                    out.append((fold, batch, n_vars, rho))
    return out


ENCODE_GRID = encode_grid()


def encode_class(fold, batch, n_vars, rho):
    return plan_class("enc", n_vars + rho - fold, 1 << (n_vars - fold), batch << fold)


def encode_case_id(fold, batch, n_vars, rho):
    return "%s-f%d-b%d-n%d-r%d" % (class_id(encode_class(fold, batch, n_vars, rho)), fold, batch, n_vars, rho)


def _check_coverage():
    reach = reachable_classes()
    hit = {plan_class("ntt", log_n, 1 << log_n, ncols) for log_n, ncols in NTT_GRID} | {encode_class(*c) for c in ENCODE_GRID}
    missing = reach - hit
    assert not missing, "plan classes the grids no longer reach: %s" % sorted(class_id(c) for c in missing)
    # and, by name: every radix template of the single pass, the LDS-only two-pass size, both pre forms in both pass counts, fused
    # input at every fold and batch of the grid
    assert {n for n, _ in NTT_GRID} >= set(range(21))
    pres = {(c[1], c[3]) for c in hit if c[3]}
    assert pres >= {(2, 1), (2, 2), (3, 1), (3, 2)}, pres
    assert {f for f, b, n, r in ENCODE_GRID if encode_class(f, b, n, r)[5]} >= {0, 1, 2, 3, 4, 5, 8}
    assert {b for f, b, n, r in ENCODE_GRID if encode_class(f, b, n, r)[5]} >= {1, 2, 3, 16}


_check_coverage()


# ---- helpers --------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=4)
def omega_powers(log_n):
    """w^e for e < N, w = the oracle's root of unity of order N (as a plain integer)"""
    import oracle_lib

    w = oracle_lib.limbs_to_ints(oracle_lib.from_mont(oracle_lib.root_of_unity(log_n)))[0]
    out, x = [], 1
    for _ in range(1 << log_n):
        out.append(x)
        x = x * w % P
    return tuple(out)


def limb_constants(oracle):
    """c as the kernels see it: the raw limbs of p - 1, the Montgomery image of p - 1 and that of 1 (as plain integers)"""
    mont = oracle.limbs_to_ints(oracle.to_mont(oracle.ints_to_limbs([P - 1, 1])))
    return {"raw_pm1": P - 1, "mont_pm1": mont[0], "mont_1": mont[1]}


def fill_ff(ctx, buf, n_bytes):
    ctx.upload_into(buf.ptr, np.full(n_bytes, 0xFF, dtype=np.uint8))


def encode_on_device(ctx, coeffs, n_vars, rho, fold):
    from provekit_amd.rs import rs_encode

    return rs_encode(coeffs, n_vars, rho, fold, ctx=ctx)


def spot_check_by_evaluation(oracle, got, coeffs, n_vars, rho, fold, picks):
    """leaf_i[b 2^fold + j] = f_{b,j}(w^i), f_{b,j}(X) = sum_t coeffs[b][2^fold t + j] X^t (Horner in the oracle, no NTT)"""
    fw = 1 << fold
    wroot = oracle.root_of_unity(n_vars + rho - fold)
    for i, col in picks:
        b, j = divmod(col, fw)
        pw = np.empty(4, dtype=np.uint64)
        oracle.L.pko_fe_pow(oracle._p(wroot), i, oracle._p(pw))
        assert np.array_equal(got[i, col], oracle.eval_univariate(np.ascontiguousarray(coeffs[b][j::fw]), pw)), (i, col)


# ---- 3. closed forms through pk_ntt -------------------------------------------------------------------------------------------
CLOSED_SIZES = [3, 6, 9, 10, 11, 14, 18, 19, 20]


def impulse_positions(log_n):
    n = 1 << log_n
    js = {0, 1, n // 2, n - 1}
    for s in row_strides(log_n):
        if s > 1:
            js |= {s - 1, s, s + 1}
    return sorted(j % n for j in js)


@pytest.mark.parametrize("rep", ["raw_pm1", "mont_pm1", "mont_1"])
@pytest.mark.parametrize("log_n", CLOSED_SIZES, ids=lambda n: ntt_case_id(n, 1))
def test_ntt_closed_forms(ctx, oracle, log_n, rep):
    """impulses d_j -> X[k] = c w^(jk); the constant c -> X = [N c, 0, ...]; c (-1)^n -> N c at N/2 and 0 elsewhere"""
    from provekit_amd.rs import ntt

    n, mask = 1 << log_n, (1 << log_n) - 1
    c = limb_constants(oracle)[rep]
    js = impulse_positions(log_n)
    ncols = len(js) + 2
    cl, ncl = oracle.ints_to_limbs([c, (P - c) % P])
    x = np.zeros((ncols, n, 4), dtype=np.uint64)
    for i, j in enumerate(js):
        x[i, j] = cl
    x[-2] = cl
    x[-1, 0::2] = cl
    x[-1, 1::2] = ncl
    got = ntt(x, ctx=ctx)
    table = oracle.ints_to_limbs([c * w % P for w in omega_powers(log_n)])  # c w^e, e < N
    k = np.arange(n, dtype=np.int64)
    for i, j in enumerate(js):
        assert np.array_equal(got[i], table[(j * k) & mask]), ("impulse", j)
    nc = oracle.ints_to_limbs([n * c % P])[0]
    exp = np.zeros((n, 4), dtype=np.uint64)
    exp[0] = nc
    assert np.array_equal(got[-2], exp), "constant"
    exp = np.zeros((n, 4), dtype=np.uint64)
    exp[n // 2] = nc
    assert np.array_equal(got[-1], exp), "alternating"
    if log_n <= 14:  # the closed forms against the oracle's own transform
        for i in range(ncols):
            assert np.array_equal(got[i], oracle.ntt(x[i], log_n)), i


# ---- 4. RS-encode over fold x batch x size x nonzero rows of pass 1 --------------------------------------------------------------
@pytest.mark.parametrize("fold,batch,n_vars,rho", ENCODE_GRID, ids=[encode_case_id(*c) for c in ENCODE_GRID])
def test_rs_encode_plan_grid(ctx, oracle, fold, batch, n_vars, rho):
    from provekit_amd.field import random_field

    coeffs = random_field(batch << n_vars, 3000 + 97 * fold + 31 * batch + 7 * n_vars + rho).reshape(batch, 1 << n_vars, 4)
    got = encode_on_device(ctx, coeffs, n_vars, rho, fold)
    assert np.array_equal(got, oracle.rs_encode(coeffs.reshape(-1, 4), batch, n_vars, rho, fold))
    lr = n_vars + rho - fold
    if lr >= 18:
        rows, w = 1 << lr, batch << fold
        spot_check_by_evaluation(oracle, got, coeffs, n_vars, rho, fold, [(0, 0), (1, w - 1), (rows // 2 + 3, w // 2), (rows - 1, w - 1)])


# ---- 5. extreme polynomials at the fused / pre and the plain pass-1 sizes ----------------------------------------------------------
# (log_rows, fold, batch): the single pass, the LDS-only two passes, two register-radix passes at two sizes, three passes
EXTREME_SIZES = [(9, 3, 3), (10, 1, 3), (11, 5, 3), (14, 2, 3), (19, 0, 3)]
EXTREME_GRID = [(lr, fold, batch, tag) for lr, fold, batch in EXTREME_SIZES for tag in (1, 2, 4)]


def extreme_case_id(lr, fold, batch, tag):
    L = nonzero_for(lr, tag)
    return "%s-f%d-b%d-lr%d-L%d" % (class_id(plan_class("enc", lr, L, batch << fold)), fold, batch, lr, L)


@pytest.mark.parametrize("pattern", ["raw_pm1", "mont_pm1", "last_only", "alt_0_pm1"])
@pytest.mark.parametrize("lr,fold,batch,tag", EXTREME_GRID, ids=[extreme_case_id(*c) for c in EXTREME_GRID])
def test_rs_encode_extreme_polynomials(ctx, oracle, lr, fold, batch, tag, pattern):
    L = nonzero_for(lr, tag)
    n_vars = fold + L.bit_length() - 1
    rho = lr - (L.bit_length() - 1)
    nc = 1 << n_vars
    consts = limb_constants(oracle)
    pm1 = oracle.ints_to_limbs([P - 1])[0]
    mpm1 = oracle.ints_to_limbs([consts["mont_pm1"]])[0]
    coeffs = np.zeros((batch, nc, 4), dtype=np.uint64)
    if pattern == "raw_pm1":
        coeffs[:] = pm1
    elif pattern == "mont_pm1":
        coeffs[:] = mpm1
    elif pattern == "last_only":
        coeffs[:, nc - 1] = pm1
    else:
        coeffs[:, 1::2] = pm1
    got = encode_on_device(ctx, coeffs, n_vars, rho, fold)
    assert np.array_equal(got, oracle.rs_encode(coeffs.reshape(-1, 4), batch, n_vars, rho, fold))
    if pattern == "last_only":
        # coefficient 2^n_vars - 1 is t = L - 1 of column j = 2^fold - 1: leaf_i = (p - 1) w^(i (L - 1)) there, 0 in every other column
        rows, fw = 1 << lr, 1 << fold
        pw = omega_powers(lr)
        col = oracle.ints_to_limbs([(P - 1) * pw[(i * (L - 1)) % rows] % P for i in range(rows)])
        exp = np.zeros_like(got)
        for b in range(batch):
            exp[:, b * fw + fw - 1] = col
        assert np.array_equal(got, exp)


# ---- 7. memory hygiene: nothing past the data is loaded, nothing outside the leaves is written --------------------------------------
GUARD_FES = 128  # 4 KiB
# the single pass (leftover columns, fold 8, batch 16), the LDS-only two passes, two register-radix passes with pass 1 folded away
# (L1 = 1, 2) and kept, three passes with pass 1 folded away and kept
HYGIENE_GRID = [(0, 3, 8, 1), (8, 1, 11, 1), (5, 16, 10, 2), (2, 3, 11, 1), (1, 3, 8, 7), (3, 2, 10, 5), (3, 2, 14, 2), (0, 1, 13, 6), (0, 1, 16, 4)]


@pytest.mark.parametrize("fold,batch,n_vars,rho", HYGIENE_GRID, ids=[encode_case_id(*c) for c in HYGIENE_GRID])
def test_rs_encode_reads_and_writes_only_its_data(ctx, oracle, fold, batch, n_vars, rho):
    """polynomials at the head of 0xFF-tailed buffers (0xFF bytes are no field element), leaves and scratch pre-filled with 0xFF and
    a 0xFF guard after the leaves (PassParams: inputs past `nonzero` are neither loaded nor multiplied, a pass writes its columns)"""
    from provekit_amd.field import random_field
    from provekit_amd.rs import rs_encode_device

    lr = n_vars + rho - fold
    rows, w, nc = 1 << lr, batch << fold, 1 << n_vars
    coeffs = random_field(batch << n_vars, 4000 + fold * 17 + n_vars).reshape(batch, nc, 4)
    polys = []
    for b in range(batch):
        buf = ctx.alloc_fe(2 * nc)
        fill_ff(ctx, buf, 64 * nc)
        ctx.upload_into(buf.ptr, coeffs[b])
        polys.append(buf)
    leaves = ctx.alloc_fe(rows * w + GUARD_FES)
    scratch = ctx.alloc_fe(2 * rows * w)
    fill_ff(ctx, leaves, 32 * (rows * w + GUARD_FES))
    fill_ff(ctx, scratch, 64 * rows * w)
    rs_encode_device(ctx, [p.ptr for p in polys], n_vars, rho, fold, leaves.ptr, scratch.ptr)
    out = ctx.download(leaves, (rows * w + GUARD_FES, 4))
    got = np.ascontiguousarray(out[: rows * w].reshape(w, rows, 4).transpose(1, 0, 2))
    assert np.array_equal(got, oracle.rs_encode(coeffs.reshape(-1, 4), batch, n_vars, rho, fold))
    assert (out[rows * w:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "guard after the leaves overwritten"
    for b in range(batch):
        tail = ctx.download(polys[b].view_fe(nc), (nc, 4))
        assert (tail == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "input buffer written"


@pytest.mark.parametrize("log_n,ncols", [(3, 5), (8, 7), (9, 4), (10, 3), (11, 1), (14, 3), (19, 1)], ids=lambda v: str(v))
def test_ntt_writes_only_its_output(ctx, oracle, log_n, ncols):
    from provekit_amd._lib import lib
    from provekit_amd.field import random_field

    n = 1 << log_n
    x = random_field(ncols << log_n, 5000 + log_n * 8 + ncols).reshape(ncols, n, 4)
    d_in = ctx.upload(x)
    d_out = ctx.alloc_fe(ncols * n + GUARD_FES)
    fill_ff(ctx, d_out, 32 * (ncols * n + GUARD_FES))
    ctx._check(lib.pk_ntt(ctx.handle, d_in.ptr, d_out.ptr, log_n, ncols))
    out = ctx.download(d_out, (ncols * n + GUARD_FES, 4))
    for c in range(ncols):
        assert np.array_equal(out[c * n: (c + 1) * n], oracle.ntt(x[c], log_n)), c
    assert (out[ncols * n:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "guard after the output overwritten"
    assert np.array_equal(ctx.download(d_in, (ncols, n, 4)), x), "input written"


# ---- 8. the shared twiddle tables outlive the context that built them and are rebuilt after the last one ------------------------
# (n_vars, rho, fold, batch): 2^19 rows, three passes with pass-ordered tables; 2^14 rows, pass 1 folded away (L1 = 2)
LIFETIME_CASES = [(18, 3, 2, 1), (10, 6, 2, 2)]

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
torch.cuda.is_available()
import provekit_amd
from provekit_amd.rs import rs_encode
from provekit_amd.whir import commit_batch

d = np.load(sys.argv[2])
cases = [tuple(int(v) for v in c) for c in d["cases"]]

def run(ctx, name):
    for i, (n_vars, rho, fold, batch) in enumerate(cases):
        coeffs = d["coeffs%d" % i]
        got = rs_encode(coeffs, n_vars, rho, fold, ctx=ctx)
        if not np.array_equal(got, d["leaves%d" % i]):
            sys.exit("%s: Montgomery encode %d differs" % (name, i))
        com = commit_batch(ctx, [ctx.upload(coeffs[b]) for b in range(batch)], n_vars, rho, fold)
        try:
            if np.frombuffer(com.root, dtype=np.uint64).tobytes() != d["root%d" % i].tobytes():
                sys.exit("%s: hash-ready commit root %d differs" % (name, i))
            idx = d["idx%d" % i]
            lv, _, _ = com.open(idx, canonical_leaves=False)
            if not np.array_equal(lv, d["leaves%d" % i][idx]):
                sys.exit("%s: opened leaves %d differ" % (name, i))
        finally:
            com.close()

a = provekit_amd.Context(0)
run(a, "A")
b = provekit_amd.Context(0)
a.close()
run(b, "B")
b.close()  # the device's last context: its tables are freed
c = provekit_amd.Context(0)
run(c, "C")
c.close()
print("OK")
"""


def test_twiddle_tables_outlive_their_context_and_are_rebuilt(oracle):
    """context A builds the tables (2^19 rows: pass-ordered and hash-ready ones too), B takes them over and A is destroyed, B is
    destroyed (the tables go with it), C builds them anew: every encode and commit root equals the oracle's, in a fresh process"""
    from provekit_amd.field import random_field

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert ntt_plan(19, 1 << 16)["L1"] >= 4 and ntt_plan(14, 1 << 8)["pre"] and ntt_plan(14, 1 << 8)["L1"] == 2
    arrays = {"cases": np.array(LIFETIME_CASES, dtype=np.int64)}
    for i, (n_vars, rho, fold, batch) in enumerate(LIFETIME_CASES):
        coeffs = random_field(batch << n_vars, 6000 + i).reshape(batch, 1 << n_vars, 4)
        leaves = oracle.rs_encode(coeffs.reshape(-1, 4), batch, n_vars, rho, fold)
        rows = leaves.shape[0]
        arrays["coeffs%d" % i] = coeffs
        arrays["leaves%d" % i] = leaves
        arrays["root%d" % i] = oracle.merkle_commit(leaves)[1]
        arrays["idx%d" % i] = np.array([0, 1, rows // 2, rows - 1], dtype=np.uint64)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "expected.npz")
        np.savez(path, **arrays)
        out = subprocess.run([sys.executable, "-c", _CHILD, root, path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1:] == ["OK"], (out.returncode, out.stdout[-1000:], out.stderr[-3000:])
