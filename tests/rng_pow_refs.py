"""References and fixed cases of tests/test_gpu_rng_pow_edges.py: the proof RNG's draw and the witness fill restated over the
host block function (pk_selftest_chacha, which test_host_only.test_chacha_block_vectors pins to the RFC), and the proof-of-work
challenges, found on the CPU with the oracle from fixed seeds.  tests/test_rng_pow_refs_host.py checks all of it without a GPU."""
import ctypes as C
import functools

import numpy as np

import oracle_lib as oracle

P = oracle.P
MASK254 = (1 << 254) - 1
RNG_STREAMS = (1, 2, 3, 4, 5, 6)  # RNG_MASK, RNG_G, RNG_BLIND, RNG_MASK_B, RNG_G_B, RNG_FILL (csrc/internal.hpp)
RNG_FILL = 6

# the draw: one key, every size a prefix of the longest (the rule does not know n)
DRAW_SEED = bytes((11 * i + 5) & 0xFF for i in range(32))
DRAW_SIZES = (1, 2, 3, 511, 512, 513, 4095, 4096, 4097, 5001, 100001)
FILL_SEED = bytes((29 * i + 1) & 0xFF for i in range(32))


def chacha12(seed32: bytes, counter: int, n0: int, n1: int) -> bytes:
    from provekit_amd._lib import lib

    out = (C.c_uint8 * 64)()
    assert lib.pk_selftest_chacha(seed32, counter, n0, n1, 12, out) == 0
    return bytes(out)


def draw_ref(seed32: bytes, stream: int, n: int):
    """-> (values, attempts): the whole draw `stream` of n elements under seed32 as Python ints, and how many blocks each element
    looked at.  Pair j = elements 2j, 2j + 1 reads the blocks (counter j, nonce {stream, attempt}), attempt = 0, 1, ...: half h of a
    block, masked to 254 bits, is element 2j + h's candidate of that attempt, accepted iff < p; an accepted half keeps its value
    while the other half goes on."""
    vals, attempts = [0] * n, [0] * n
    for j in range((n + 1) // 2):
        need = [True, 2 * j + 1 < n]
        attempt = 0
        while need[0] or need[1]:
            blk = chacha12(seed32, j, stream, attempt)
            for half in (0, 1):
                if need[half]:
                    v = int.from_bytes(blk[32 * half: 32 * half + 32], "little") & MASK254
                    if v < P:
                        vals[2 * j + half], attempts[2 * j + half], need[half] = v, attempt + 1, False
            attempt += 1
    return vals, attempts


@functools.lru_cache(maxsize=None)
def draw_cached(stream: int, n: int = max(DRAW_SIZES)):
    """draw_ref under DRAW_SEED, computed once per (stream, n); callers must not change the lists"""
    return draw_ref(DRAW_SEED, stream, n)


def fill_ref(seed32: bytes, is_set, vals):
    """fill_witness as values (not Montgomery images): entry i keeps vals[i] where is_set[i], otherwise it is the 128-bit word
    i & 3 of the block (counter i >> 2, nonce {RNG_FILL, 0}).  -> (values, how many were filled)"""
    out, blocks = [int(v) for v in vals], {}
    for i in np.flatnonzero(np.asarray(is_set) == 0):
        i = int(i)
        if i >> 2 not in blocks:
            blocks[i >> 2] = chacha12(seed32, i >> 2, RNG_FILL, 0)
        out[i] = int.from_bytes(blocks[i >> 2][16 * (i & 3): 16 * (i & 3) + 16], "little")
    return out, int((np.asarray(is_set) == 0).sum())


# ---- proof of work -------------------------------------------------------------------------------------------------------
CHECK_BITS = (1.0, 2.5, 8.0)
CHECK_NONCES = tuple(list(range(64)) + [(1 << 32) + d for d in (-2, -1, 0, 1, 2)] + [1 << 40, (1 << 63) - 1, 1 << 63, (1 << 64) - 2, (1 << 64) - 1])
TOP_NONCE = (1 << 64) - 1
POW_SEED = 2024
BIAS_BITS = 5.0


def challenge_words(v: int) -> np.ndarray:
    return oracle.ints_to_limbs([v])[0]


def _challenges(rng, count):
    """`count` 256-bit challenges: the even ones anywhere in [0, 2^256) (four in five are >= p: generic.rs reduces them), the odd
    ones below 2^252 < p"""
    out = []
    for k in range(count):
        w = rng.integers(0, 1 << 64, size=4, dtype=np.uint64)
        if k & 1:
            w[3] &= np.uint64((1 << 60) - 1)
        out.append(w)
    return out


@functools.lru_cache(maxsize=None)
def pow_cases():
    """The fixed proof-of-work cases, every expected answer from the oracle alone:
      check:  three challenges (one random below p, one random with the top bit set, i.e. >= p, and p - 1) for CHECK_BITS x CHECK_NONCES
      bias:   (challenge, BIAS_BITS, nonce): the smallest nonce valid at BIAS_BITS, and NOT valid under the prover's threshold
              (BIAS_BITS + 0.01), so pk_pow_solve has to pass it by; `bias_solve` is what it finds instead
      solve:  [(challenge, bits, smallest nonce under the biased threshold)]: 64 challenges at 12 bits, 16 at 14, one at 1 bit
              whose answer is 0, and one each at 0.25 and 0.99 bits
    Callers must not change the arrays."""
    rng = np.random.default_rng(POW_SEED)
    lo, hi = _challenges(rng, 2)[1], _challenges(rng, 1)[0]
    hi[3] |= np.uint64(1 << 63)
    check = [lo, hi, challenge_words(P - 1)]
    bias = None
    for ch in _challenges(rng, 4000):
        first = next(k for k in range(1 << 12) if oracle.pow_verify(ch, BIAS_BITS, k))
        if not oracle.pow_verify(ch, BIAS_BITS + 0.01, first):
            bias = (ch, BIAS_BITS, first)
            break
    assert bias is not None
    solve = [(ch, 12.0, oracle.pow_solve(ch, 12.0)) for ch in _challenges(rng, 64)]
    solve += [(ch, 14.0, oracle.pow_solve(ch, 14.0)) for ch in _challenges(rng, 16)]
    zero = next(ch for ch in _challenges(rng, 64) if oracle.pow_solve(ch, 1.0) == 0)
    solve.append((zero, 1.0, 0))
    solve += [(ch, b, oracle.pow_solve(ch, b)) for ch, b in zip(_challenges(rng, 2), (0.25, 0.99))]
    return {"check": check, "bias": bias, "bias_solve": oracle.pow_solve(bias[0], BIAS_BITS), "solve": solve}
