"""CPU: host-only entry points of the C ABI (no device needed): PoW threshold conversion and the ark MultiPath
wire format, checked against the oracle, the golden vectors and the bytes of the reference's proof fixture."""
import json
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_pow_threshold_matches_oracle_and_golden(oracle):
    from provekit_amd.pow import threshold

    vec = json.load(open(os.path.join(G, "vectors.json")))["pow_threshold"]
    for d, h in vec:
        assert oracle.limbs_to_ints(threshold(float(d)))[0] == int(h, 16)
    for d in (0.01, 3.141592653589793, 17.5, 59.99):
        assert np.array_equal(threshold(d), oracle.pow_threshold(d))
    with pytest.raises(ValueError):
        threshold(80.0)



def test_multipath_serialization_matches_fixture_bytes():
    """ark MultiPath wire format: re-serialise the fully-opened blinding tree of the reference's proof fixture
    and compare with the bytes the reference prover wrote (host-only entry point)."""
    from provekit_amd.whir import multipath_serialize

    fix = json.load(open(os.path.join(G, "fixture_merkle.json")))
    raw = fix["blinding_T0_multipath_raw"]
    t = fix["trees"][0]
    mp = t["multipath"]

    def limbs(hs):
        return np.frombuffer(b"".join(int(h, 16).to_bytes(32, "little") for h in hs), dtype="<u8").reshape(-1, 4)

    idx = mp["leaf_indexes"]
    sib = limbs(mp["leaf_sibling_hashes"])
    paths = np.stack([limbs(p) for p in mp["auth_paths_root_to_leaf"]])
    assert multipath_serialize(idx, sib, paths).hex() == raw["serialized_hex"]




def test_whir_config_derivation_matches_the_fixture_shape():
    """pk_whir_config_derive restates WhirConfig::new for provekit's parameters (provekit/r1cs-compiler/src/whir_r1cs.rs:38-53).
    The whir crate is not in the reference tree; what pins the derivation is the reference's proof fixture:
    for n = 21 the prover opened 109 / 28 / 16 / 11 leaves in the four rounds and 9 in the final one, sent one OOD answer per
    round and a PoW nonce in every round; the blinding WHIR (n = 8) has one round + final with nonces in both."""
    from provekit_amd.scheme import WhirConfig, blinding_config_for

    c = WhirConfig.derive(21)
    assert c.num_queries == [109, 28, 16, 11] and c.final_queries == 9
    assert c.ood_samples == [1, 1, 1, 1] and c.commitment_ood_samples == 1
    # pow_bits = 128 - queries * log_inv_rate (rates 1, 4, 7, 10, 13): every round grinds, as the fixture's nonces show
    assert c.pow_bits == [19.0, 16.0, 16.0, 18.0] and c.final_pow_bits == 11.0
    assert c.final_folding_pow_bits == 0.0  # 128 < field_bits - 1: whir.go:196-201 does not run
    b = blinding_config_for(20)
    assert b.n_vars == 8 and b.n_rounds == 1  # next_power_of_two(4 * 20) + 1 variables
    # default_max_pow(8, 1) = 6 -> 122 queries into the 32-leaf tree (all 32 opened in the fixture), ceil(122/4) = 31 into
    # the 16-leaf round tree (13 distinct in the fixture)
    assert b.num_queries == [122] and b.final_queries == 31 and b.pow_bits == [6.0] and b.final_pow_bits == 4.0
    # round count / final polynomial size as recursive-verifier/app/circuit/whir.go:24-29 reads them
    for n in (4, 8, 12, 17, 23, 25, 26):
        c = WhirConfig.derive(n)
        assert c.n_rounds == n // 4 - 1 and n - 4 * (c.n_rounds + 1) == n % 4
        assert all(q * r + p >= 128 - 1e-9 for q, r, p in zip(c.num_queries, range(1, 40, 3), c.pow_bits))


def _chacha_block_py(key: bytes, counter: int, n0: int, n1: int, rounds: int) -> bytes:
    """RFC 8439 section 2.3, restated independently (state words 12, 13 = 64-bit counter, 14, 15 = nonce)"""
    import struct

    M = 0xFFFFFFFF
    rotl = lambda v, n: ((v << n) | (v >> (32 - n))) & M
    s = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + list(struct.unpack("<8I", key)) + [counter & M, counter >> 32, n0, n1]
    x = list(s)

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & M; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & M; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & M; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & M; x[b] = rotl(x[b] ^ x[c], 7)

    for _ in range(rounds // 2):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return struct.pack("<16I", *[(a + b) & M for a, b in zip(x, s)])


def random_fe_py(seed32: bytes, stream: int, i: int) -> int:
    """element i of the proof RNG's draw `stream`: candidate (i mod 2) of the blocks (counter i // 2, nonce {stream, attempt}),
    attempt = 0, 1, ... until it is < p; 12 rounds"""
    P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    attempt, half = 0, i & 1
    while True:
        blk = _chacha_block_py(seed32, i >> 1, stream, attempt, 12)
        v = int.from_bytes(blk[32 * half : 32 * half + 32], "little") & ((1 << 254) - 1)
        if v < P:
            return v
        attempt += 1


def test_chacha_block_vectors():
    """the proof RNG's block function: RFC 8439 section 2.3.2 (20 rounds; key 00..1f, nonce 00:00:00:09:00:00:00:4a:00:00:00:00,
    block counter 1), the all-zero ChaCha12 and ChaCha20 keystream blocks (draft-strombergson-chacha-test-vectors TC1), and
    the independent Python restatement on random inputs at 12 rounds (what the device runs)"""
    import ctypes as C

    from provekit_amd._lib import lib

    key = bytes(range(32))
    out = (C.c_uint8 * 64)()
    assert lib.pk_selftest_chacha(key, 1 | (0x09000000 << 32), 0x4A000000, 0, 20, out) == 0
    want = bytes.fromhex("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
                         "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
    assert bytes(out) == want
    assert lib.pk_selftest_chacha(bytes(32), 0, 0, 0, 12, out) == 0
    assert bytes(out).hex() == ("9bf49a6a0755f953811fce125f2683d50429c3bb49e074147e0089a52eae155f"
                                "0564f879d27ae3c02ce82834acfa8c793a629f2ca0de6919610be82f411326be")
    assert lib.pk_selftest_chacha(bytes(32), 0, 0, 0, 20, out) == 0
    assert bytes(out).hex().startswith("76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7")
    rng = np.random.default_rng(3)
    for _ in range(20):
        k = rng.bytes(32)
        ctr, n0, n1 = int(rng.integers(0, 2**63)), int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32))
        assert lib.pk_selftest_chacha(k, ctr, n0, n1, 12, out) == 0
        assert bytes(out) == _chacha_block_py(k, ctr, n0, n1, 12)


def test_sparse_matrix_rejects_malformed_arrays():
    """R1CS upload reads new_row_indices[0..rows) and values[0..nnz) on the C side: lengths and ranges are checked first"""
    from provekit_amd.sparse_matrix import SparseMatrix

    ok = SparseMatrix(3, 4, np.array([0, 1, 2], np.uint32), np.array([0, 1, 3], np.uint32), np.array([0, 0, 1], np.uint32))
    assert ok.nnz == 3
    with pytest.raises(ValueError):
        SparseMatrix(3, 4, np.array([0, 1], np.uint32), np.array([0, 1, 3], np.uint32), np.array([0, 0, 1], np.uint32))
    with pytest.raises(ValueError):
        SparseMatrix(3, 4, np.array([0, 1, 2], np.uint32), np.array([0, 1, 3], np.uint32), np.array([0, 0], np.uint32))
    with pytest.raises(ValueError):
        SparseMatrix(3, 4, np.array([0, 1, 2], np.uint32), np.array([0, 1, 4], np.uint32), np.array([0, 0, 1], np.uint32))  # column out of range
    with pytest.raises(ValueError):
        SparseMatrix(3, 4, np.array([0, 2, 1], np.uint32), np.array([0, 1, 3], np.uint32), np.array([0, 0, 1], np.uint32))  # offsets not sorted
    with pytest.raises(ValueError):
        SparseMatrix(3, 4, np.array([0, 1, 5], np.uint32), np.array([0, 1, 3], np.uint32), np.array([0, 0, 1], np.uint32))  # offset beyond nnz


def test_derived_pow_bits_are_consistent_with_the_reference_proofs_nonces():
    """the grinding difficulties pk_whir_config_derive computes (blinding 6 / 4, witness 19 / 16 / 16 / 18 / 11 bits) cannot be
    read off a proof -- but the reference's proof carries the seven nonces its grinder found, and a valid nonce of a d-bit grind is (close to)
    geometric with mean 2^d.  The fixture's nonces are 67, 2 | 332221, 106952, 37657, 156995, 1587: log2 = 6.1, 1.6 | 18.3, 16.7, 15.2, 17.3,
    10.6.  A statistical pin, not an exact one: (i) every nonce lies in the window a d-bit search produces with probability 0.97, (ii) the
    derived vector is more likely than the same vector shifted by two bits or more either way, than a flat 16-bit schedule (round 1 of this
    repository) and than no grinding at all, (iii) the mean of log2(nonce) - d sits where an exponential puts it (-0.83 +- 0.7)."""
    import json
    import math
    import os

    from provekit_amd.scheme import WhirConfig, blinding_config_for

    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fixture_whir.json")))
    cb, cw = blinding_config_for(20), WhirConfig.derive(21)
    bits = list(cb.pow_bits) + [cb.final_pow_bits] + list(cw.pow_bits) + [cw.final_pow_bits]
    nonces = fx["pow_nonces"]["blinding"] + fx["pow_nonces"]["witness"]
    assert bits == [6.0, 4.0, 19.0, 16.0, 16.0, 18.0, 11.0] and len(nonces) == 7

    def loglik(ds):  # the smallest valid nonce of a d-bit grind: P(n) = p (1 - p)^n, p = 2^-d (the verifier's threshold, pow.rs:24-26)
        return sum(math.log(2.0 ** -d) + n * math.log1p(-(2.0 ** -d)) if d > 0 else (0.0 if n == 0 else -math.inf) for d, n in zip(ds, nonces))

    for d, n in zip(bits, nonces):
        assert 2.0 ** (d - 5) <= n + 1 <= 2.0 ** (d + 4), (d, n)
    ours = loglik(bits)
    for shift in (-6, -4, -3, -2, 2, 3, 4, 6):
        assert ours > loglik([d + shift for d in bits]), shift
    assert ours > loglik([16.0] * 7) and ours > loglik([10.0] * 7) and loglik([0.0] * 7) == -math.inf
    dev = [math.log2(n + 1) - d for d, n in zip(bits, nonces)]
    assert -1.6 < sum(dev) / len(dev) < -0.1, dev


def test_scheme_arena_bytes_is_the_sum_of_a_proofs_buffers():
    """pk_scheme_arena_bytes (host only): what pk_scheme_create will allocate for a prover of a given shape -- ~20.6 x 32 B x 2^m at
    rate 1/2, fold 16, batch 2; bench.py sizes its prover counts from it.  Monotone in every argument, refuses nonsense."""
    import ctypes as C

    from provekit_amd._lib import lib
    from provekit_amd.scheme import WhirConfig, _cfg_struct, arena_bytes

    sizes = {m: arena_bytes(m, m - 1, (1 << (m - 1)) - 5, WhirConfig.derive(m)) for m in (13, 17, 21, 23, 25)}
    for m, b in sizes.items():
        assert 19.0 < (b - (64 << 20)) / (32.0 * (1 << m)) < 22.0, (m, b)  # the arena itself, without the 64 MiB constant
    assert sizes[21] < 1.6e9 and 22e9 < sizes[25] < 24e9
    assert arena_bytes(21, 20, 1 << 20, WhirConfig.derive(21)) > arena_bytes(21, 20, 1 << 19, WhirConfig.derive(21))
    n = C.c_size_t()
    cw = _cfg_struct(WhirConfig.derive(21))
    assert lib.pk_scheme_arena_bytes(21, 22, 1 << 20, C.byref(cw), C.byref(n)) == -1  # m_0 > m
    assert lib.pk_scheme_arena_bytes(21, 20, 1 << 20, None, C.byref(n)) == -1
    assert lib.pk_scheme_arena_bytes(21, 20, 1 << 20, C.byref(cw), None) == -1
    # the configs pk_scheme_create refuses are refused by the host-only entry points too
    from provekit_amd.scheme import WhirConfigStruct, blinding_config_for

    assert lib.pk_scheme_arena_bytes(21, 20, 1 << 20, C.byref(WhirConfigStruct()), C.byref(n)) == -1  # all zero
    cb = _cfg_struct(blinding_config_for(20))
    cw.starting_log_inv_rate = 0
    assert lib.pk_whir_r1cs_io_pattern(20, C.byref(cw), C.byref(cb), None, 0, C.byref(n)) == -1
    why = C.create_string_buffer(256)
    assert lib.pk_io_pattern_check(b"x", 1, 20, C.byref(cw), C.byref(cb), why, len(why)) == -1


def test_test_hooks_are_an_entry_point_not_the_environment():
    """the GPU suite's hooks (a gated kernel's spin bound, a stalled host, the RCCL branch for a repeated device) are set through
    pk_selftest_set_hook; the library reads no test switch from the environment"""
    import os

    from provekit_amd._lib import lib

    assert lib.pk_selftest_set_hook(0, 0) == 0 and lib.pk_selftest_set_hook(2, 0) == 0
    assert lib.pk_selftest_set_hook(3, 1) == -1 and lib.pk_selftest_set_hook(-1, 1) == -1 and lib.pk_selftest_set_hook(0, -5) == -1
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "provekit_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".hpp")):
            txt = open(os.path.join(csrc, f)).read()
            assert "PK_TEST_" not in txt and "PK_RCCL_SAME_DEVICE" not in txt, f
