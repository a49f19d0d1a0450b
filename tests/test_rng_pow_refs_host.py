"""CPU: the references and fixed cases of tests/test_gpu_rng_pow_edges.py (tests/rng_pow_refs.py) against the independent Python
restatement of the draw, and the proof-of-work challenges against the oracle -- a reference that is wrong, or a case that lacks
the property it was chosen for, would otherwise show as a GPU test failing (or passing) for no reason in the kernel."""
import numpy as np

import rng_pow_refs as R

P = R.P


def test_draw_ref_equals_the_restatement_on_two_streams():
    from test_host_only import random_fe_py

    for stream in (1, 6):
        vals, attempts = R.draw_ref(R.DRAW_SEED, stream, 500)
        assert len(vals) == len(attempts) == 500 and all(v < P for v in vals) and min(attempts) >= 1
        for i in range(500):
            assert vals[i] == random_fe_py(R.DRAW_SEED, stream, i), (stream, i)
    # the rule does not know n: a shorter draw is a prefix, an odd length ends on a first half
    vals, attempts = R.draw_ref(R.DRAW_SEED, 1, 500)
    assert R.draw_ref(R.DRAW_SEED, 1, 7) == (vals[:7], attempts[:7])
    assert R.draw_cached(1)[0][:500] == vals and R.draw_ref(R.DRAW_SEED, 1, 0) == ([], [])


def test_draws_the_gpu_tests_use_hold_long_retry_chains():
    """what the state machine of random_fe_kernel can get wrong needs retries: an element with 4 or more attempts in every array
    from 511 elements on, in both orders of the pair (the first half accepted long before the second, and the reverse)"""
    for stream in (1, 6):
        vals, attempts = R.draw_cached(stream)
        assert len(vals) == max(R.DRAW_SIZES) and all(v < P for v in vals)
        assert max(attempts[:511]) >= 4
        pairs = list(zip(attempts[0:510:2], attempts[1:511:2]))
        assert any(a == 1 and b >= 3 for a, b in pairs) and any(a >= 3 and b == 1 for a, b in pairs)
    _, attempts = R.draw_cached(1)
    assert max(attempts) >= 8  # 0.244^7 per element: a few among 10^5
    assert len({R.draw_cached(s)[0][0] for s in R.RNG_STREAMS}) == len(R.RNG_STREAMS)


def test_fill_ref_is_the_rule_of_the_existing_fill_test():
    import ctypes as C

    from provekit_amd._lib import lib

    n = 23
    is_set = np.array([i % 3 == 0 for i in range(n)], dtype=np.uint8)
    vals = list(range(100, 100 + n))
    got, count = R.fill_ref(R.FILL_SEED, is_set, vals)
    assert count == int((is_set == 0).sum())
    blk = (C.c_uint8 * 64)()
    for i in range(n):
        if is_set[i]:
            assert got[i] == vals[i]
        else:
            assert lib.pk_selftest_chacha(R.FILL_SEED, i >> 2, 6, 0, 12, blk) == 0
            assert got[i] == int.from_bytes(bytes(blk)[16 * (i & 3): 16 * (i & 3) + 16], "little") < 1 << 128
    assert R.fill_ref(R.FILL_SEED, np.ones(n, np.uint8), vals) == (vals, 0)


def test_pow_cases_have_the_properties_they_were_chosen_for(oracle):
    cases = R.pow_cases()
    ints = [oracle.limbs_to_ints(ch)[0] for ch in cases["check"]]
    assert len(ints) == 3 and ints[0] < P <= ints[1] and ints[2] == P - 1
    assert set(range(64)) <= set(R.CHECK_NONCES) and {(1 << 32) - 2, (1 << 32) + 2, 1 << 40, (1 << 63) - 1, 1 << 63, R.TOP_NONCE - 1, R.TOP_NONCE} <= set(R.CHECK_NONCES)
    # the high word of the nonce is hashed in both directions: for some (challenge, bits) the nonces at or above 2^32 hold an
    # accepted and a rejected one -- and 2^64 - 1 itself is rejected somewhere (where the parent answered 1) and accepted somewhere
    high = [k for k in R.CHECK_NONCES if k >= 1 << 32]
    assert len(high) == 8
    assert any(len({oracle.pow_verify(ch, b, k) for k in high}) == 2 for ch in cases["check"] for b in R.CHECK_BITS)
    top = {oracle.pow_verify(ch, b, R.TOP_NONCE) for ch in cases["check"] for b in R.CHECK_BITS}
    assert top == {False, True}
    # dropping the high word changes an answer: some high nonce and its low word differ under the oracle
    assert any(oracle.pow_verify(ch, b, k) != oracle.pow_verify(ch, b, k & 0xFFFFFFFF) for ch in cases["check"] for b in R.CHECK_BITS for k in high)

    ch, bits, nonce = cases["bias"]
    assert oracle.pow_verify(ch, bits, nonce) and not oracle.pow_verify(ch, bits + 0.01, nonce)
    assert all(not oracle.pow_verify(ch, bits, k) for k in range(nonce))
    assert cases["bias_solve"] == oracle.pow_solve(ch, bits) > nonce and oracle.pow_verify(ch, bits + 0.01, cases["bias_solve"])

    solve = cases["solve"]
    assert [b for _, b, _ in solve] == [12.0] * 64 + [14.0] * 16 + [1.0, 0.25, 0.99]
    want = [w for _, _, w in solve]
    assert want[80] == 0 and any(0 < w < 256 for w in want)
    assert any(4096 <= w < 8192 for w in want[:64])  # a lane's second stride at 12 bits (16 x 256 lanes)
    assert any(w >= 1 << 14 for w in want)
    for ch, b, w in solve[::9] + solve[80:]:  # the answers are the oracle's smallest nonces under the biased threshold
        assert oracle.pow_verify(ch, b + 0.01, w) and oracle.pow_verify(ch, b, w)
        assert w > 4096 or all(not oracle.pow_verify(ch, b + 0.01, k) for k in range(w))
    assert any(oracle.limbs_to_ints(ch)[0] >= P for ch, _, _ in solve) and any(oracle.limbs_to_ints(ch)[0] < P for ch, _, _ in solve)
