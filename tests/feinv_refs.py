"""The safegcd inverse (csrc/feinv.hpp) piecewise: what each of its functions must return, stated on Python ints, and operands that put
each function into the states a whole inversion of a random operand reaches with probability about 2^-30 per batch -- matrices with
|u| + |v| = 2^30, d and e at both ends of (-2p, p), md at both ends of its range, zero runs of a whole batch, swaps at the first and
the last steps, eta in the hundreds.

Plain Python ints, seeded, no GPU and no import of the library: tests/test_feinv_host.py (CPU, also the sanitizer program) and
tests/test_gpu_feinv.py (device) take the same records and the same expected values from here.  Every set is built once.

THE REFERENCE is the definition, not a transliteration of the 32-bit code:
  * a batch (parts 0, 1) is 30 single division steps of Bernstein-Yang (eprint 2019/266) on unbounded integers,
        delta > 0 and g odd:  (delta, f, g) <- (1 - delta, g, (g - f) / 2)        otherwise:  (1 + delta, f, (g + (g mod 2) f) / 2)
    carried as 2 delta: even for the classic form (part 1, delta = -eta), odd for the half-delta form (part 0, 2 delta = -2 zeta - 1).
    The matrix is the integer one with (f30, g30) 2^30 = (u f0 + v g0, q f0 + r g0), its entries read as signed 32-bit values;
  * update_de (part 2): md starts as u [d < 0] + v [e < 0] and is lowered by (p^-1 (u d + v e) + md) mod 2^30; then
    d' = (u d + v e + p md) / 2^30, an exact division; the same for e' with (q, r) and me;
  * update_fg (part 3): (u f + v g) / 2^30 and (q f + r g) / 2^30, exact;
  * normalize (part 4): sign(sign) r mod p in [0, p) on canonical limbs;
  * to_s30 / from_s30 (parts 5, 6): the nine 30-bit limbs of a 256-bit value and back;
  * the whole inverse: pow(x, -1, P), 0 -> 0.
var_trace below IS a transliteration of divsteps30_var, kept for one purpose: to say which `limit`, zero runs and swap positions a
record reaches (the batched form's own bookkeeping, which the definition does not have).  Its matrix is checked against the
definition's on every record, and nothing is compared with it.

PRECONDITIONS of the functions, which every record here meets:
  * divsteps30, divsteps30_var: f0 odd; g0 any 32-bit word (only the low 30 bits of either decide the steps); zeta / eta any value
    whose walk over 30 steps stays inside 32 bits (here |eta| <= 750);
  * update_de: d, e in (-2p, p) as nine limbs, limbs 0..7 in [0, 2^30), limb 8 signed; a matrix a batch can emit (|u| + |v| <= 2^30,
    |q| + |r| <= 2^30).  It returns d', e' in (-2p, p) in the same form;
  * update_fg: |f|, |g| < 2^255 in the same form with (f, g) = (f0, g0) mod 2^30 for the (f0, g0) the matrix came from;
  * normalize: r in (-2p, p) in the same form; only the sign bit of `sign` is read;
  * to_s30: any 256-bit value;  from_s30: limbs in [0, 2^30) of a value below 2^256.

A RECORD is 32 signed 32-bit words in and 32 out, packed as csrc/selftest_inv30.hpp states (an s30 as its nine limbs, a matrix as
u, v, q, r, a word of f or g as its 32 bits); words a part does not name are zero."""
import functools
import random

import numpy as np

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R = 1 << 256
B30 = 1 << 30
M30 = B30 - 1
M32 = (1 << 32) - 1
PINV30 = pow(P, -1, B30)
PARTS = {0: "divsteps30", 1: "divsteps30_var", 2: "update_de", 3: "update_fg", 4: "normalize", 5: "to_s30", 6: "from_s30"}


def s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def limbs9(v):
    """a signed value as update_de leaves it: limbs 0..7 in [0, 2^30), limb 8 signed"""
    return [(v >> (30 * i)) & M30 for i in range(8)] + [v >> 240]


def value9(ls):
    return sum(int(x) << (30 * i) for i, x in enumerate(ls))


def pack(rows):
    """rows of at most 32 integers (any of them as a signed or an unsigned 32-bit word) -> (n, 32) int32"""
    a = np.zeros((len(rows), 32), dtype=np.int64)
    for i, row in enumerate(rows):
        a[i, : len(row)] = [s32(x) for x in row]
    return a.astype(np.int32)


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def batch(delta2, f0, g0, steps=30):
    """`steps` division steps from (2 delta, f0, g0): (u, v, q, r), 2 delta'"""
    assert f0 & 1
    f, g, u, v, q, r = f0, g0, 1, 0, 0, 1
    for _ in range(steps):
        if delta2 > 0 and g & 1:
            delta2, f, g = 2 - delta2, g, (g - f) >> 1
            u, v, q, r = 2 * q, 2 * r, q - u, r - v
        else:
            if g & 1:
                g, q, r = g + f, q + u, r + v
            delta2, g, u, v = delta2 + 2, g >> 1, 2 * u, 2 * v
    assert (u * f0 + v * g0, q * f0 + r * g0) == (f << steps, g << steps)
    return (u, v, q, r), delta2


def divsteps30(zeta, f0, g0):
    t, d2 = batch(-2 * zeta - 1, f0, g0)
    return t, -(d2 + 1) // 2


def divsteps30_var(eta, f0, g0):
    t, d2 = batch(-2 * eta, f0, g0)
    return t, -d2 // 2


def update_de(d, e, t):
    """-> d', e', md, me"""
    out = []
    for a, b in ((t[0], t[1]), (t[2], t[3])):
        c = a * d + b * e
        m = a * (d < 0) + b * (e < 0)
        m -= (PINV30 * c + m) % B30
        c += P * m
        assert c % B30 == 0
        out.append((c >> 30, m))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def update_fg(f, g, t):
    cf, cg = t[0] * f + t[1] * g, t[2] * f + t[3] * g
    assert cf % B30 == 0 and cg % B30 == 0
    return cf >> 30, cg >> 30


def normalize(r, sign):
    return (-r if s32(sign) < 0 else r) % P


def inverse(x):
    return pow(x, -1, P) if x % P else 0


# ---- the batched form's bookkeeping (coverage only) ----------------------------------------------------------------------------------
def var_trace(eta, f0, g0):
    """divsteps30_var step by step: (u, v, q, r) as 32-bit words, eta', the `limit` of every multiple of f it added, the zero runs it
    shifted and the step index (0..29) of every swap"""
    u, v, q, r, f, g = 1, 0, 0, 1, f0 & M32, g0 & M32
    finv = f * (2 - f * f) & M32
    i, limits, runs, swaps = 30, [], [], []
    while True:
        x = g | (M32 << i & M32)
        zeros = (x & -x).bit_length() - 1
        g, u, v, eta, i = g >> zeros, u << zeros & M32, v << zeros & M32, eta - zeros, i - zeros
        runs.append(zeros)
        if i == 0:
            break
        if eta < 0:
            swaps.append(30 - i)
            eta, f, g, u, q, v, r = -eta, g, -f & M32, q, -u & M32, r, -v & M32
            finv = f * (2 - f * f) & M32
        limit = min(eta + 1, i, 6)
        limits.append(limit)
        w = -g * finv & ((1 << limit) - 1)
        g, q, r = (g + f * w) & M32, (q + u * w) & M32, (r + v * w) & M32
    return tuple(s32(x) for x in (u, v, q, r)), eta, limits, runs, swaps


# ---- operands: parts 0 and 1 -----------------------------------------------------------------------------------------------------------
G_WORDS = (0, 1, 2, 3, 1 << 28, (1 << 28) + (1 << 29), 1 << 29, M30, B30, B30 + 1, 1 << 31, M32, 0x55555555, 0xAAAAAAAA, 0xC0000000,
           0x80000000 | (1 << 29), (1 << 31) - 1, 0x3FFFFFFE, 0x7FFFFFFC, 5 << 27)
F_WORDS = (1, 3, M30, M32, 0x55555555, 0x80000001, 0x40000001, P & M32, P & M30, 0xAAAAAAAB, (1 << 31) - 1, 7 << 28 | 1)
ETAS = tuple(range(-40, 41)) + (-300, 300, -750, 750)


@functools.lru_cache(maxsize=None)
def step_operands():
    """(eta or zeta, f0, g0): every eta with every structured g0, the structured f0 in rotation, and random words"""
    rnd = random.Random(30)
    ops = []
    for n, eta in enumerate(ETAS):
        for k, g0 in enumerate(G_WORDS):
            ops.append((eta, F_WORDS[(n + k) % len(F_WORDS)], g0))
            ops.append((eta, rnd.getrandbits(32) | 1, g0))
        for f0 in F_WORDS[n % 3::3]:
            ops.append((eta, f0, rnd.getrandbits(32)))
        for sh in (0, 7, 19, 27):  # random words with a run of low zeros
            ops.append((eta, rnd.getrandbits(32) | 1, rnd.getrandbits(32) << sh & M32))
        ops += [(eta, rnd.getrandbits(32) | 1, rnd.getrandbits(32)) for _ in range(6)]
    return tuple(ops)


@functools.lru_cache(maxsize=None)
def step_results(part):
    """the definition on step_operands(): ((u, v, q, r), eta') per record"""
    fn = divsteps30 if part == 0 else divsteps30_var
    return tuple(fn(*op) for op in step_operands())


@functools.lru_cache(maxsize=None)
def matrices():
    """every distinct matrix parts 0 and 1 produce on step_operands(), with the (f0, g0) of its first appearance"""
    seen = {}
    for part in (0, 1):
        for (_, f0, g0), (t, _) in zip(step_operands(), step_results(part)):
            seen.setdefault(t, (f0, g0))
    return tuple(sorted(seen.items()))


# ---- operands: part 2 ------------------------------------------------------------------------------------------------------------------
DE_EDGES = (-2 * P + 1, -2 * P + 2, -P - 1, -P, -P + 1, -1, 0, 1, P - 2, P - 1, -(1 << 254), 1 << 253)


def _tz(c):
    return (c & -c).bit_length() - 1


def _steer_k(a, b, d, e, largest, outward):
    """d, e with one of them moved by less than 2^30 (away from zero or towards it: its sign stays) so that the multiple of p that
    update_de takes off for the row (a, b) is the largest, or the smallest, that the row's common power of two allows: the low bits of
    the operand under the entry with the fewest trailing zeros steer it"""
    if a == 0 and b == 0:
        return d, e
    on_e = a == 0 or (b != 0 and _tz(b) <= _tz(a))
    c, x = (b, e) if on_e else (a, d)
    z = _tz(c)
    k0 = (PINV30 * (a * d + b * e) + a * (d < 0) + b * (e < 0)) % B30
    target = (B30 - (1 << z) if largest else 0) + k0 % (1 << z)
    dx = ((target - k0) % B30 >> z) * pow(PINV30 * (c >> z), -1, B30) % (B30 >> z)  # PINV30 c dx = target - k0 mod 2^30
    x += dx if (x > 0) == outward else dx - (B30 >> z)
    return (d, x) if on_e else (x, e)


def _steer(a, b, largest, high):
    """d, e in (-2p, p) that bring the row (a, b) to an end of its output range: a d + b e + p md0 = +-(|a| + |b|) (p - 1) (`high`: +),
    then the largest or the smallest multiple of p taken off"""
    def end(c):  # c (x + p [x < 0]) = +-|c| (p - 1)
        return 0 if c == 0 else P - 1 if (c > 0) == high else -2 * P + 1
    return _steer_k(a, b, end(a), end(b), largest, False)


@functools.lru_cache(maxsize=None)
def de_operands():
    """(d, e, t): every matrix with edge pairs in rotation, the matrices at the ends of what a batch emits with every edge pair and with
    operands steered to both ends of the outputs and of md, and random d, e in (-2p, p)"""
    rnd = random.Random(31)
    ms = [t for t, _ in matrices()]
    pairs = [(d, e) for d in DE_EDGES for e in DE_EDGES]
    ops = []
    for n, t in enumerate(ms):
        ops += [(pairs[(5 * n + 37 * k) % len(pairs)] + (t,)) for k in range(3)]
    neg = lambda a, b: min(a, 0) + min(b, 0)
    full = [t for t in ms if abs(t[0]) + abs(t[1]) == B30 or abs(t[2]) + abs(t[3]) == B30]
    by_neg = sorted(ms, key=lambda t: min(neg(t[0], t[1]), neg(t[2], t[3])))
    ends = []
    for t in full[:: max(1, len(full) // 24)][:24] + by_neg[:8] + [(B30, 0, 0, 1)]:
        if t not in ends:
            ends.append(t)
    for t in ends:
        ops += [(d, e, t) for d, e in pairs]
    for t in full + by_neg[:64]:
        for a, b in ((t[0], t[1]), (t[2], t[3])):
            for largest, high in ((True, False), (False, True), (False, False), (True, True)):
                ops.append(_steer(a, b, largest, high) + (t,))
            # both operands negative under negative entries: md starts at its lowest
            d, e = (-1 if a < 0 else 1), (-1 if b < 0 else 1)
            ops.append((d, e, t))
            ops.append(_steer_k(a, b, d, e, True, True) + (t,))
    for _ in range(2000):
        ops.append((rnd.randrange(-2 * P + 1, P), rnd.randrange(-2 * P + 1, P), rnd.choice(ms)))
    assert all(-2 * P < d < P and -2 * P < e < P for d, e, _ in ops)
    return tuple(ops)


@functools.lru_cache(maxsize=None)
def de_results():
    return tuple(update_de(*op) for op in de_operands())


# ---- operands: parts 3 and 4 -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fg_operands():
    """(f, g, t): signed f, g below 2^255 in magnitude that end in the (f0, g0) the matrix came from (so both divisions are exact):
    nothing above the low limb, minus one above it, both ends of the range, random"""
    rnd = random.Random(32)
    top = 1 << 225  # multiples of 2^30 up to 2^255
    highs = (0, -1, top - 1, -top, 1, -2, top >> 1, -(top >> 1))
    ops = []
    for n, (t, (f0, g0)) in enumerate(matrices()):
        for k in range(2):
            hf, hg = (highs[(n + 3 * k) % 8], highs[(3 * n + k + 1) % 8]) if k == 0 else (rnd.randrange(-top, top), rnd.randrange(-top, top))
            ops.append(((f0 & M30) + (hf << 30), (g0 & M30) + (hg << 30), t))
    assert all(abs(f) < 1 << 255 and abs(g) < 1 << 255 for f, g, _ in ops)
    return tuple(ops)


@functools.lru_cache(maxsize=None)
def normalize_operands():
    """(r, sign): the ends of (-2p, p), what update_de returned at its ends, the values around 0 and -p, limbs of all ones and all zeros
    on either side of zero, random values; sign = 0 and -1 as the inverse passes them, and other words of either sign"""
    rnd = random.Random(33)
    outs = [x for d, e, _, _ in de_results() for x in (d, e)]
    vals = set(DE_EDGES) | {min(outs), max(outs), P - (1 << 240), -(1 << 240), -P - (1 << 240), (1 << 240) - 1, -2 * P + (1 << 30)}
    for k in range(1, 9):
        for c in ((1 << 30 * k), (1 << 30 * k) - 1, (1 << 30 * k) + 1):
            vals.update(x for x in (c, -c, P - c, c - P, -P - c, c - 2 * P) if -2 * P < x < P)
    vals.update(rnd.randrange(-2 * P + 1, P) for _ in range(300))
    vals.update(sorted(outs)[:40] + sorted(outs)[-40:])
    signs = (0, -1, 1, -(1 << 31), (1 << 31) - 1, -12345)
    return tuple((r, s) for r in sorted(vals) for s in signs)


@functools.lru_cache(maxsize=None)
def conversion_values():
    """256-bit values for to_s30 (and, as limbs, for from_s30): ones and zeros on either side of every limb and word boundary"""
    rnd = random.Random(34)
    vals = {0, 1, R - 1, P, P - 1, 2 * P, 5 * P}
    for b in sorted(set(range(0, 256, 30)) | set(range(0, 256, 32))):
        vals.update(x % R for x in ((1 << b), (1 << b) - 1, (1 << b) + 1, R - (1 << b), (M30 << b), (M32 << b), R - 1 - (M30 << b) % R))
    vals.update(rnd.getrandbits(256) for _ in range(400))
    return tuple(sorted(vals))


# ---- the records of a part -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def records(part):
    """(in, want): two (n, 32) int32 arrays"""
    if part in (0, 1):
        rin = [list(op) for op in step_operands()]
        want = [list(t) + [x] for t, x in step_results(part)]
    elif part == 2:
        rin = [limbs9(d) + limbs9(e) + list(t) for d, e, t in de_operands()]
        want = [limbs9(d) + limbs9(e) for d, e, _, _ in de_results()]
    elif part == 3:
        rin = [limbs9(f) + limbs9(g) + list(t) for f, g, t in fg_operands()]
        want = [limbs9(a) + limbs9(b) for a, b in (update_fg(*op) for op in fg_operands())]
    elif part == 4:
        rin = [limbs9(r) + [s] for r, s in normalize_operands()]
        want = [limbs9(normalize(r, s)) for r, s in normalize_operands()]
    elif part == 5:
        rin = [[(v >> 32 * i) & M32 for i in range(8)] for v in conversion_values()]
        want = [limbs9(v) for v in conversion_values()]
    elif part == 6:
        rin = [limbs9(v) for v in conversion_values()]
        want = [[(v >> 32 * i) & M32 for i in range(8)] for v in conversion_values()]
    else:
        raise ValueError(part)
    a, b = pack(rin), pack(want)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def differing(got, want, rin, limit=4):
    """the first records whose 32 words differ: (index, words in, words got, words wanted)"""
    bad = np.flatnonzero((np.asarray(got) != want).any(axis=1))[:limit]
    return [(int(i), rin[i][:22].tolist(), np.asarray(got)[i][:18].tolist(), want[i][:18].tolist()) for i in bad]


# ---- whole inversions ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inversion_values():
    """operands of the whole inverse whose walks leave the middle of the road: powers of two and their neighbours (zero runs, eta in the
    hundreds), p minus them, odd multiples of 2^30, 2^60 and 2^90 (whole batches of zeros after the first), inverses of small numbers and
    their negatives (the OUTPUT at either end), (p +- 1) / 2, and the values tests/test_fe29_host.py has"""
    rnd = random.Random(35)
    vals = {0, 1, 2, 3, P - 1, P - 2, (P + 1) // 2, (P - 1) // 2, 1 << 253, 1 << 128, M30, B30}
    for k in range(254):
        vals.update(x for x in ((1 << k) - 1, 1 << k, (1 << k) + 1, P - (1 << k)) if 0 <= x < P)
    for sh in (30, 60, 90):
        for m in (1, 3, 5, M30, B30 + 1, rnd.getrandbits(100) | 1, rnd.getrandbits(160) | 1, (P >> sh) - 1 | 1, ((P >> sh) - 2) | 1):
            if m << sh < P:
                vals.add(m << sh)
    for s in range(1, 41):
        vals.update((pow(s, -1, P), P - pow(s, -1, P)))
    return tuple(sorted(vals))


def walk(x, var=True):
    """the inversion of x batch by batch on the definition (variable-time form: batches until g = 0; else 20 batches of the half-delta
    form): what it passes through.  The batched form's own figures (limits, zero runs) come from var_trace."""
    d, e, f, g, eta = 0, 1, P, x, -1
    info = {"batches": 0, "eta": [eta], "d": [], "md": [], "limits": [], "runs": [], "zero_batches": []}
    for it in range(30 if var else 20):
        if var and g == 0:
            break
        if var:
            t, eta2 = divsteps30_var(eta, f & M30, g & M30)
            tt, te, limits, runs, _ = var_trace(eta, f & M30, g & M30)
            assert (tt, te) == (t, eta2)
            info["limits"] += limits
            info["runs"] += runs
            if runs[0] == 30:  # g = 0 mod 2^30 on entry (a run of 30 after g + w f = 0 is the end of a walk, not this)
                info["zero_batches"].append(it)
        else:
            t, eta2 = divsteps30(eta, f & M30, g & M30)
        d, e, md, me = update_de(d, e, t)
        f, g = update_fg(f, g, t)
        eta = eta2
        info["batches"] += 1
        info["eta"].append(eta)
        info["d"] += [d, e]
        info["md"] += [md, me]
    assert g == 0 and f in (1, -1) or x == 0
    info["result"] = normalize(d, f)
    return info


@functools.lru_cache(maxsize=None)
def inversion_walks():
    """the variable-time walk of every value of inversion_values(), in that order"""
    ws = tuple(walk(x) for x in inversion_values())
    assert all(w["result"] == inverse(x) for w, x in zip(ws, inversion_values()))
    return ws


def sorted_order():
    """the values by the batches their walks take (ties by value)"""
    vals, ws = inversion_values(), inversion_walks()
    return [vals[i] for i in sorted(range(len(vals)), key=lambda i: (ws[i]["batches"], vals[i]))]


def interleaved_order(wave=64):
    """a lane order in which every wavefront opens with the lane that leaves the batch loop at once (x = 0), one that takes the most
    batches the list holds, x = 1 and another of the longest (0, 1 and the few longest values are repeated in every wavefront), and then
    alternates the most and the fewest batches of what is left: the sorted values dealt round the wavefronts, each wavefront's share laid
    out from both ends inwards.  A short share is filled with values a second time, so that every wavefront is whole."""
    srt = sorted_order()
    most = max(w["batches"] for w in inversion_walks())
    longest = [x for x, w in zip(inversion_values(), inversion_walks()) if w["batches"] == most]
    rest = [x for x in srt if x > 1]
    per = wave - 4
    n_waves = -(-len(rest) // per)
    order = []
    for w in range(n_waves):
        share = rest[w::n_waves]
        share = sorted(share + [rest[(7 * w + 11 * k) % len(rest)] for k in range(per - len(share))], key=srt.index)  # whole wavefronts
        lanes, lo, hi = [0, longest[2 * w % len(longest)], 1, longest[(2 * w + 1) % len(longest)]], 0, len(share) - 1
        for k in range(len(share)):
            if k % 2 == 0:
                lanes.append(share[hi])
                hi -= 1
            else:
                lanes.append(share[lo])
                lo += 1
        order += lanes
    return order


def summarize(ws):
    """the figures of a set of walks: batch counts, the eta range, the ends of d / p and of md, the histogram of `limit`"""
    ds = [x for w in ws for x in w["d"]]
    mds = [x for w in ws for x in w["md"]]
    etas = [x for w in ws for x in w["eta"]]
    lim = [x for w in ws for x in w["limits"]]
    return {"batches": sorted({w["batches"] for w in ws}), "eta": (min(etas), max(etas)), "d_over_p": (min(ds) / P, max(ds) / P),
            "md": (min(mds), max(mds)), "limits": {k: lim.count(k) for k in range(1, 7)},
            "zero_batches_after_first": sum(1 for w in ws if any(b > 0 for b in w["zero_batches"]))}


def to_limbs(xs):
    xs = list(xs)
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u8").reshape(len(xs), 4).copy()


def from_limbs(a):
    b = np.ascontiguousarray(a, dtype="<u8").reshape(-1, 4).tobytes()
    return [int.from_bytes(b[32 * i: 32 * i + 32], "little") for i in range(len(b) // 32)]
