"""GPU: the kernels with no algebraic reference at their edges -- random_fe_kernel and fill_witness_kernel (csrc/rng.hip) over whole
arrays with guard elements behind them, pow_search_kernel / pk_pow_check (csrc/pow.hip) against the oracle for acceptances AND
rejections, and the hash kernels (csrc/hash.hip) at Skyscraper v1, wide leaves and every node of the heap.  Everything is
bit-exact.  The references and the fixed cases are tests/rng_pow_refs.py, checked on the CPU by tests/test_rng_pow_refs_host.py.

Not reachable through the C ABI at a difficulty a test can afford, and so not tested here: the search striped over a device set
(world > 1) and the loop that moves the window after a miss (base += window)."""
import ctypes as C
import functools

import numpy as np
import pytest

import rng_pow_refs as R

pytestmark = pytest.mark.gpu

P = R.P


def sentinel(m, tag=0):
    """m elements no kernel here can produce: the top limb is all ones (>= p, not a 254-bit candidate, not a Montgomery image)"""
    s = np.empty((m, 4), dtype=np.uint64)
    s[:, 0] = np.arange(m, dtype=np.uint64) + np.uint64(0xDEAD00000000 + (tag << 24))
    s[:, 1], s[:, 2], s[:, 3] = np.uint64(0x5A5A5A5A5A5A5A5A), np.uint64(0xA5A5A5A5A5A5A5A5), np.uint64(0xFFFFFFFFFFFFFFFF)
    return s


# ---- random_fe_kernel ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def draw_limbs(stream, n=max(R.DRAW_SIZES)):
    import oracle_lib

    return oracle_lib.ints_to_limbs(R.draw_cached(stream, n)[0])


def device_draw(ctx, stream, n, seed=R.DRAW_SEED):
    """draw n elements into a buffer of n + 2 sentinels -> all n + 2"""
    from provekit_amd._lib import lib

    d = ctx.upload(sentinel(n + 2, stream))
    ctx._check(lib.pk_selftest_random_fe(ctx.handle, seed, stream, d.ptr, n))
    return ctx.download_fe(d, n + 2)


@pytest.mark.parametrize("n", R.DRAW_SIZES)
def test_draw_equals_the_reference_everywhere_and_stops_at_n(ctx, n):
    """every element of the draw, and the two elements behind it: at an odd n the second half of the last pair is not stored --
    at 5001 and 100001 that pair is a lane's later pair (done1 recomputed after j += stride), at n = 1 the lane starts with it"""
    got = device_draw(ctx, 1, n)
    assert np.array_equal(got[n:], sentinel(n + 2, 1)[n:])
    assert np.array_equal(got[:n], draw_limbs(1)[:n])


def test_draw_of_nothing_touches_nothing(ctx):
    from provekit_amd._lib import lib

    got = device_draw(ctx, 1, 0)
    assert np.array_equal(got, sentinel(2, 1))
    ctx._check(lib.pk_selftest_random_fe(ctx.handle, R.DRAW_SEED, 1, None, 0))


@pytest.mark.parametrize("stream", [1, 6])
def test_a_shorter_draw_is_a_prefix_of_a_longer_one(ctx, stream):
    """one and two workgroups, another stride: draw(4097)[:513] == draw(513), both the reference's"""
    long, short = device_draw(ctx, stream, 4097), device_draw(ctx, stream, 513)
    assert np.array_equal(long[:513], short[:513])
    assert np.array_equal(long[:4097], draw_limbs(stream, 4097)) and np.array_equal(short[513:], sentinel(515, stream)[513:])


def test_the_streams_of_one_key_differ(ctx, oracle):
    firsts = []
    for stream in R.RNG_STREAMS:
        got = device_draw(ctx, stream, 8)
        assert oracle.limbs_to_ints(got[:8]) == R.draw_ref(R.DRAW_SEED, stream, 8)[0], stream
        firsts.append(got[0].tobytes())
    assert len(set(firsts)) == len(R.RNG_STREAMS)


# ---- fill_witness_kernel -------------------------------------------------------------------------------------------------
def device_fill(ctx, oracle, is_set, seed=R.FILL_SEED, want_count=True, field_seed=1):
    """pk_witness_fill over n random stored elements with one sentinel behind them -> (got (n + 1, 4), expected (n + 1, 4), count or
    None, expected count): set entries keep their bits, unset ones are the Montgomery images of fill_ref's words"""
    from provekit_amd._lib import lib
    from provekit_amd.field import random_field

    is_set = np.ascontiguousarray(is_set, dtype=np.uint8)
    n = len(is_set)
    exp = np.concatenate([random_field(max(n, 1), field_seed)[:n], sentinel(1)])
    d_w = ctx.upload(exp)
    d_set = ctx.upload(is_set if n else np.zeros(8, np.uint8))
    words, exp_count = R.fill_ref(seed, is_set, [0] * n)
    unset = np.flatnonzero(is_set == 0)
    if len(unset):
        exp[unset] = oracle.to_mont(oracle.ints_to_limbs([words[i] for i in unset]))
    cnt = C.c_size_t(12345)
    ctx._check(lib.pk_witness_fill(ctx.handle, d_w.ptr, d_set.ptr, n, seed, C.byref(cnt) if want_count else None))
    return ctx.download_fe(d_w, n + 1), exp, cnt.value if want_count else None, exp_count


@pytest.mark.parametrize("n", [1, 4, 5, 1023])
def test_fill_with_every_entry_set_changes_nothing(ctx, oracle, n):
    got, exp, count, _ = device_fill(ctx, oracle, np.ones(n, np.uint8))
    assert count == 0 and np.array_equal(got, exp)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023])
def test_fill_with_no_entry_set(ctx, oracle, n):
    got, exp, count, _ = device_fill(ctx, oracle, np.zeros(n, np.uint8))
    assert count == n and np.array_equal(got, exp)


@pytest.mark.parametrize("n", [5, 1021])
def test_fill_alternating_and_last_entry_masks(ctx, oracle, n):
    """n % 4 == 1: the last entry is word 0 of a block of its own"""
    assert n % 4 == 1
    for first in (0, 1):
        mask = (np.arange(n) + first) & 1
        got, exp, count, exp_count = device_fill(ctx, oracle, mask)
        assert count == exp_count == int((mask == 0).sum()) and np.array_equal(got, exp)
    mask = np.ones(n, np.uint8)
    mask[n - 1] = 0
    got, exp, count, _ = device_fill(ctx, oracle, mask)
    assert count == 1 and np.array_equal(got, exp)


def test_fill_past_one_grid_stride(ctx, oracle):
    """2^19 + 5 entries: more than the lanes of the capped grid (CUs x 8 workgroups x 256), so lanes take a second stride"""
    import torch

    n = (1 << 19) + 5
    assert n > torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    mask = np.random.default_rng(19).integers(0, 2, size=n).astype(np.uint8)
    mask[n - 5:] = (1, 0, 0, 1, 0)
    got, exp, count, exp_count = device_fill(ctx, oracle, mask)
    assert count == exp_count == int((mask == 0).sum())
    assert np.array_equal(got, exp)


def test_fill_without_a_count_pointer_and_of_nothing(ctx, oracle):
    from provekit_amd._lib import lib

    mask = np.random.default_rng(3).integers(0, 2, size=777).astype(np.uint8)
    got, exp, count, _ = device_fill(ctx, oracle, mask, want_count=False)
    assert count is None and np.array_equal(got, exp)
    got, exp, count, _ = device_fill(ctx, oracle, np.zeros(0, np.uint8))
    assert count == 0 and np.array_equal(got, exp)
    ctx._check(lib.pk_witness_fill(ctx.handle, None, None, 0, R.FILL_SEED, None))


def test_fill_twice_counts_each_call(ctx, oracle):
    """the device counter is zeroed by every call"""
    rng = np.random.default_rng(4)
    for n, density in ((1000, 0.5), (333, 0.1), (1000, 0.9)):
        mask = (rng.random(n) < density).astype(np.uint8)
        got, exp, count, exp_count = device_fill(ctx, oracle, mask)
        assert count == exp_count == int((mask == 0).sum()) and np.array_equal(got, exp)


# ---- pow_search_kernel, pk_pow_check -------------------------------------------------------------------------------------
def pow_check(ctx, ch, bits, nonce):
    from provekit_amd._lib import lib

    ok = C.c_int(-1)
    ctx._check(lib.pk_pow_check(ctx.handle, ch.ctypes.data, bits, nonce, C.byref(ok)))
    assert ok.value in (0, 1)
    return bool(ok.value)


def pow_solve(ctx, ch, bits):
    from provekit_amd._lib import lib

    nonce = C.c_uint64(0xFFFF)
    ctx._check(lib.pk_pow_solve(ctx.handle, ch.ctypes.data, bits, C.byref(nonce)))
    return nonce.value


@pytest.mark.parametrize("bits", R.CHECK_BITS)
def test_pow_check_accepts_and_rejects_like_the_oracle(ctx, oracle, bits):
    """nonces 0..63, around 2^32, 2^40, around 2^63 and the two largest: the high word of the nonce is hashed, and a rejection
    is a rejection"""
    for c, ch in enumerate(R.pow_cases()["check"]):
        for nonce in R.CHECK_NONCES:
            assert pow_check(ctx, ch, bits, nonce) == oracle.pow_verify(ch, bits, nonce), (c, bits, nonce)


def test_pow_check_of_the_largest_nonce_is_its_hash_and_leaves_the_search_armed(ctx, oracle):
    """nonce 2^64 - 1 is the value the search's device word uses for `nothing found`: pk_pow_check must answer it by its hash
    (it answered 1 for every challenge and difficulty), and a search right after must still be right"""
    cases = R.pow_cases()
    ch_s, bits_s, want = cases["solve"][0]
    for ch in cases["check"]:
        for bits in R.CHECK_BITS + (20.0,):
            assert pow_check(ctx, ch, bits, R.TOP_NONCE) == oracle.pow_verify(ch, bits, R.TOP_NONCE), bits
            assert pow_solve(ctx, ch_s, bits_s) == want
            assert pow_check(ctx, ch, 0.0, R.TOP_NONCE)  # pow.rs:24-26: no work asked, nothing hashed


def test_pow_prover_bias_boundary(ctx, oracle):
    """a nonce valid at `bits` but not under the prover's threshold (bits + 0.01): the check accepts it, the search passes it by"""
    cases = R.pow_cases()
    ch, bits, nonce = cases["bias"]
    assert pow_check(ctx, ch, bits, nonce) and not pow_check(ctx, ch, bits + 0.01, nonce)
    got = pow_solve(ctx, ch, bits)
    assert got != nonce and got == cases["bias_solve"] == oracle.pow_solve(ch, bits)
    assert pow_check(ctx, ch, bits, got) and pow_check(ctx, ch, bits + 0.01, got)


def test_pow_solve_returns_the_oracles_smallest_nonce(ctx, oracle):
    """64 challenges at 12 bits, 16 at 14 (answers below 256, in a lane's second stride, beyond 2^14), one whose answer is 0, and
    difficulties below one bit: a wrong early exit or a lost atomicMin would return a larger nonce"""
    for k, (ch, bits, want) in enumerate(R.pow_cases()["solve"]):
        assert pow_solve(ctx, ch, bits) == want, (k, bits)
    for ch, bits, want in R.pow_cases()["solve"][-3:]:
        assert pow_check(ctx, ch, bits, want) == oracle.pow_verify(ch, bits, want) == True  # noqa: E712


def test_pow_solve_after_an_argument_error(ctx):
    from provekit_amd import ProveKitHipError

    ch, bits, want = R.pow_cases()["solve"][1]
    with pytest.raises(ProveKitHipError):
        pow_solve(ctx, ch, 60.0)
    with pytest.raises(ProveKitHipError):
        pow_check(ctx, ch, 60.0, 1)
    assert pow_solve(ctx, ch, bits) == want


# ---- hash kernels: Skyscraper v1 and v2, wide leaves, every node ------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 33, 64, 256])
@pytest.mark.parametrize("version", [2, 1])
def test_leaf_hash_widths_sizes_versions_layouts(ctx, oracle, version, width):
    """1, 255, 256, 257 leaves (the last lane of a workgroup, one lane of a second) of up to 256 elements (a commit folding 8
    variables hashes leaves this wide and wider), both layouts, both versions: every digest"""
    from provekit_amd._lib import PK_COL_MAJOR, PK_LEAF_MAJOR, lib
    from provekit_amd.field import random_field

    leaves = random_field(257 * width, 500 + width).reshape(257, width, 4)
    leaves[0, 0], leaves[256, width - 1] = 0, oracle.ints_to_limbs([P - 1])[0]
    exp = oracle.leaf_hash(leaves, version)
    ctx.set_hash_version(version)
    try:
        for n in (1, 255, 256, 257):
            for layout, arr in ((PK_LEAF_MAJOR, leaves[:n]), (PK_COL_MAJOR, leaves[:n].transpose(1, 0, 2))):
                d_l, d_out = ctx.upload(arr), ctx.upload(sentinel(n + 1))
                ctx._check(lib.pk_leaf_hash(ctx.handle, d_l.ptr, n, width, layout, d_out.ptr))
                got = ctx.download_fe(d_out, n + 1)
                assert np.array_equal(got[:n], exp[:n]) and np.array_equal(got[n], sentinel(n + 1)[n]), (n, layout)
    finally:
        ctx.set_hash_version(2)


@pytest.mark.parametrize("log_n", [10, 11, 12, 16])
def test_merkle_commit_v1_every_node(ctx, oracle, log_n):
    """Skyscraper v1 through the top kernel alone (2^10 leaves), one and two fused levels below it (2^11, 2^12), five fused levels
    then one (2^16): every node of the heap, slot 0 cleared, nothing behind the heap"""
    from provekit_amd._lib import PK_LEAF_MAJOR, lib
    from provekit_amd.field import random_field

    n, width = 1 << log_n, 2
    leaves = random_field(n * width, 300 + log_n).reshape(n, width, 4)
    exp = oracle.merkle_commit(leaves, version=1)
    assert not exp[0].any()
    d_l, d_nodes = ctx.upload(leaves), ctx.upload(sentinel(2 * n + 1))
    ctx.set_hash_version(1)
    try:
        ctx._check(lib.pk_merkle_commit(ctx.handle, d_l.ptr, n, width, PK_LEAF_MAJOR, d_nodes.ptr))
        got = ctx.download_fe(d_nodes, 2 * n + 1)
    finally:
        ctx.set_hash_version(2)
    assert np.array_equal(got[: 2 * n], exp) and np.array_equal(got[2 * n], sentinel(2 * n + 1)[2 * n])
    assert not np.array_equal(exp, oracle.merkle_commit(leaves, version=2))


@pytest.mark.parametrize("version", [2, 1])
def test_merkle_inner_on_caller_digests_canonical_or_not(ctx, oracle, version):
    """pk_merkle_inner takes the caller's digests as they are: p, p + 1 and 2^256 - 1 among them hash as the oracle hashes them
    (generic.rs reduces any 256-bit input); 2^11 leaves = one fused level, then the top kernel"""
    from provekit_amd._lib import lib
    from provekit_amd.field import random_field

    n = 1 << 11
    digests = random_field(n, 40 + version)
    odd = [P, P + 1, (1 << 256) - 1, 0, P - 1]
    at = [0, 1, 2, 3, 1000, 1001, n - 2, n - 1]
    digests[at] = oracle.ints_to_limbs([odd[k % len(odd)] for k in range(len(at))])
    digests[1001], digests[n - 1] = oracle.ints_to_limbs([(1 << 256) - 1, P])
    exp = oracle.merkle_inner(digests, version)
    heap = sentinel(2 * n + 1)
    heap[n: 2 * n] = digests
    d_nodes = ctx.upload(heap)
    ctx.set_hash_version(version)
    try:
        ctx._check(lib.pk_merkle_inner(ctx.handle, d_nodes.ptr, n))
        got = ctx.download_fe(d_nodes, 2 * n + 1)
    finally:
        ctx.set_hash_version(2)
    assert np.array_equal(got[: 2 * n], exp) and np.array_equal(got[2 * n], heap[2 * n])
    assert max(oracle.limbs_to_ints(got[1:n])) < P
