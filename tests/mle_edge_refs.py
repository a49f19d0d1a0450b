"""Shared by test_gpu_mle_edges.py and test_mle_edge_refs_host.py: the Python-int definitions and closed forms the MLE / sumcheck
edge tests use as references, and the grid rule of reduce.hpp's reduction_blocks.  Everything here works on STORED values: a field
element is the integer its 32 bytes hold (the Montgomery image), a product of two stored values is x y R^-1 mod p, sums and
differences are plain ones mod p.  No kernel and no C oracle in this file: the CPU suite checks it against both."""
import numpy as np

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R = (1 << 256) % P  # the stored value of the field's one
R_INV = pow(R, -1, P)
ONE, MINUS_ONE, TOP = R, P - R, P - 1  # stored: the field's 1 and -1, and the largest stored value there is
CHALLENGES = {"zero": 0, "one": ONE, "minus_one": MINUS_ONE, "top": TOP}

RED_THREADS, RED_MAX_BLOCKS = 256, 1024


def mul(x, y):
    return x * y * R_INV % P


def limbs(xs):
    xs = list(xs)
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u8").reshape(len(xs), 4).copy()


def ints(a):
    b = np.ascontiguousarray(a, dtype="<u8").reshape(-1, 4).tobytes()
    return [int.from_bytes(b[i: i + 32], "little") for i in range(0, len(b), 32)]


def const(n, v):
    return np.tile(limbs([v]), (n, 1))


def periodic(n, pool):
    """element i holds pool[i % len(pool)]"""
    reps = -(-n // len(pool))
    return np.tile(limbs(pool), (reps, 1))[:n].copy()


def stored_sum(a):
    """sum of the stored values of an (n, 4) array mod p, through 32-bit column sums (n < 2^32)"""
    w = np.ascontiguousarray(a, dtype="<u8").reshape(-1, 4).view("<u4").reshape(-1, 8)
    cols = w.sum(axis=0, dtype=np.uint64)
    return sum(int(c) << (32 * i) for i, c in enumerate(cols)) % P


# ---- the grid of a reduction launch (reduce.hpp reduction_blocks) ----------------------------------------------------------------
def reduction_blocks(items, latency, num_cus):
    per_thread = 1 if latency else 4
    need = max(1, -(-items // (RED_THREADS * per_thread)))
    return min(need, num_cus * 4, RED_MAX_BLOCKS)


def geometry_items(latency):
    """item counts on both sides of each boundary of the grid rule, with the workgroups a 1024-workgroup cap gives them:
    one workgroup | two; 256 | 257 (the final pass's second stride); the cap reached and, in latency mode, exceeded"""
    if latency:
        return {256: 1, 257: 2, 1 << 16: 256, (1 << 16) + 1: 257, 1 << 18: 1024, (1 << 19) + 3: 1024}
    return {1024: 1, 1025: 2, 1 << 18: 256, (1 << 18) + 1: 257, 1 << 20: 1024}


# ---- closed forms -----------------------------------------------------------------------------------------------------------------
def dot_of_constants(n, w, f):
    """<w, f> of two constant arrays of n elements"""
    return n * mul(w, f) % P


def horner_closed_forms(c):
    """sum_i c[i] z^i at z = 0, 1, -1: c[0], the plain sum and the alternating sum"""
    c = np.ascontiguousarray(c).reshape(-1, 4)
    return {"zero": ints(c[:1])[0], "one": stored_sum(c), "minus_one": (stored_sum(c[0::2]) - stored_sum(c[1::2])) % P}


def horner(c_ints, z):
    acc = 0
    for v in reversed(c_ints):
        acc = (mul(acc, z) + v) % P
    return acc


def product_table_coeffs_ints(xs):
    """to_coeffs of f[i] = prod_j (bit_j(i) ? x_j : 1): prod_j (x_j - 1)^bit_j(i)  (each variable's v[i | h] -= v[i] acts on its own factor)"""
    out = [ONE]
    for x in xs:
        out = out + [mul(v, (x - ONE) % P) for v in out]
    return out


def product_table_ints(xs):
    out = [ONE]
    for x in xs:
        out = out + [mul(v, x) for v in out]
    return out


def to_coeffs_ints(v):
    v = list(v)
    h = 1
    while h < len(v):
        for i in range(len(v)):
            if i & h:
                v[i] = (v[i] - v[i ^ h]) % P
        h <<= 1
    return v


# ---- definitions, evaluated once per DISTINCT tuple of operands -------------------------------------------------------------------
def grouped(cols, fn):
    """cols: arrays (n, 4) -- row i of each is one operand of work item i.  fn(tuple of ints) -> (sums, outs): the item's addends
    and its output values.  Returns (the sums over all items mod p, one (n, 4) array per output).  The definition runs once per
    distinct operand tuple, so structured inputs of any length cost a handful of evaluations and random ones n."""
    m = np.concatenate([np.ascontiguousarray(c).reshape(-1, 4) for c in cols], axis=1)
    packed = np.ascontiguousarray(m).view(np.dtype((np.void, m.shape[1] * 8))).ravel()
    u, inv, cnt = np.unique(packed, return_inverse=True, return_counts=True)
    rows = np.frombuffer(u.tobytes(), dtype="<u8").reshape(len(u), -1)
    vals = ints(rows.reshape(-1, 4))
    k = len(cols)
    sums, outs = None, None
    for j in range(len(u)):
        s, o = fn(tuple(vals[j * k: (j + 1) * k]))
        if sums is None:
            sums, outs = [0] * len(s), [[] for _ in o]
        for t, v in enumerate(s):
            sums[t] = (sums[t] + int(cnt[j]) * v) % P
        for t, v in enumerate(o):
            outs[t].append(v)
    return sums, [limbs(o)[inv.ravel()] for o in outs]


def fold(x0, x1, r):
    return (x0 + mul(r, (x1 - x0) % P)) % P


def cubic_map(a0, a1, b0, b1, c0, c1, e0, e1):
    """f0 = eq0 (a0 b0 - c0); f(-1) = (2 eq0 - eq1) ((2 a0 - a1)(2 b0 - b1) - (2 c0 - c1)); f_inf = (eq1 - eq0)(a1 - a0)(b1 - b0)"""
    f0 = mul(e0, (mul(a0, b0) - c0) % P)
    fm = mul((2 * e0 - e1) % P, (mul((2 * a0 - a1) % P, (2 * b0 - b1) % P) - (2 * c0 - c1)) % P)
    fi = mul(mul((e1 - e0) % P, (a1 - a0) % P), (b1 - b0) % P)
    return [f0, fm, fi]


def cubic_round(a, b, c, eq, fold_r=None):
    """sumcheck_fold_map_reduce::<4,3>: the partner of i is i + len/2; folding first p0 += r (p2 - p0), p1 += r (p3 - p1) with
    p = (i, i + len/4, i + len/2, i + 3 len/4).  -> ([f0, f(-1), f_inf], the four folded arrays of len/2 elements (or None))"""
    arrs = [np.ascontiguousarray(x).reshape(-1, 4) for x in (a, b, c, eq)]
    n = arrs[0].shape[0]
    if fold_r is None:
        h = n // 2
        cols = [x[o: o + h] for x in arrs for o in (0, h)]
        sums, _ = grouped(cols, lambda t: (cubic_map(*t), []))
        return sums, None
    q = n // 4
    cols = [x[o: o + q] for x in arrs for o in (0, q, 2 * q, 3 * q)]

    def fn(t):
        v = []
        for k in range(4):
            x0, x1, x2, x3 = t[4 * k: 4 * k + 4]
            v += [fold(x0, x2, fold_r), fold(x1, x3, fold_r)]
        return cubic_map(*v), v

    sums, outs = grouped(cols, fn)
    return sums, [np.concatenate([outs[2 * k], outs[2 * k + 1]]) for k in range(4)]


def quadratic_map(f0, f1, w0, w1):
    """h(0) = f0 w0, h(1) = f1 w1, h(2) = (2 f1 - f0)(2 w1 - w0) over the adjacent pairs (2i, 2i + 1)"""
    return [mul(f0, w0), mul(f1, w1), mul((2 * f1 - f0) % P, (2 * w1 - w0) % P)]


def quadratic_round(f, w, fold_r=None):
    """folding first v'[i] = v[2i] + r (v[2i+1] - v[2i]).  -> ([h(0), h(1), h(2)], (f', w') or None)"""
    f, w = (np.ascontiguousarray(x).reshape(-1, 4) for x in (f, w))
    if fold_r is None:
        sums, _ = grouped([f[0::2], f[1::2], w[0::2], w[1::2]], lambda t: (quadratic_map(*t), []))
        return sums, None

    def fn(t):
        v = [fold(t[0], t[1], fold_r), fold(t[2], t[3], fold_r), fold(t[4], t[5], fold_r), fold(t[6], t[7], fold_r)]
        return quadratic_map(*v), v

    sums, outs = grouped([f[0::4], f[1::4], f[2::4], f[3::4], w[0::4], w[1::4], w[2::4], w[3::4]], fn)
    n = f.shape[0] // 2
    fo, wo = np.empty((n, 4), np.uint64), np.empty((n, 4), np.uint64)
    fo[0::2], fo[1::2], wo[0::2], wo[1::2] = outs
    return sums, (fo, wo)


def fold_pairs(v, r):
    v = np.ascontiguousarray(v).reshape(-1, 4)
    return grouped([v[0::2], v[1::2]], lambda t: ([], [fold(t[0], t[1], r)]))[1][0]


def fold_coeffs(c, k, rs):
    """out[t] = sum_j c[2^k t + j] prod_b r_b^bit_b(j)"""
    wts = [ONE]
    for r in rs:
        wts = wts + [mul(v, r) for v in wts]
    c = np.ascontiguousarray(c).reshape(-1, 4)
    cols = [c[j:: 1 << k] for j in range(1 << k)]
    return grouped(cols, lambda t: ([], [(t[0] + sum(mul(t[j], wts[j]) for j in range(1, 1 << k))) % P]))[1][0]


def axpy(y, beta, x):
    """y + beta x, element by element"""
    return grouped([y, x], lambda t: ([], [(t[0] + mul(beta, t[1])) % P]))[1][0]


def eq_table_ints(point):
    """eq(x, i) = prod_j (bit_j(i) ? x_j : 1 - x_j), variable 0 <-> the most significant index bit"""
    out = [ONE]
    for x in point:
        out = [v for t in out for v in (mul(t, (ONE - x) % P), mul(t, x))]
    return out


def eq_accumulate(w, points, scales, overwrite=False):
    """out[i] (+)= sum over the points of scale * eq(point, i)"""
    acc = [0] * len(w) if overwrite else list(w)
    for pt, s in zip(points, scales):
        acc = [(a + mul(s, e)) % P for a, e in zip(acc, eq_table_ints(pt))]
    return acc
