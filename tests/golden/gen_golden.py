#!/usr/bin/env python3
"""Mint the golden fixtures under tests/golden/.

Reads the proof fixture kept next to this script (poseidon-1000.np, a copy of
the reference's tooling/provekit-bench/benches/poseidon-1000.np); the outputs
are committed and are what the tests read.

Sources of truth:
  * skyscraper_kats.json  -- the known-answer values typed in the reference's own
    tests: skyscraper/core/src/reference.rs:104-188 (sbox table, ss(2), bb(6),
    permute(0,0), permute(random)); skyscraper/core/src/pow.rs:88-103
    (f64_to_u256); skyscraper/block-multiplier/proptest-regressions/scalar.txt
    (two shrunk multiplier inputs).  Data only.
  * fixture_merkle.json   -- Merkle openings decoded from the reference's proof
    fixture tooling/provekit-bench/benches/poseidon-1000.np (a data file held by
    the reference's benches).  The fixture predates the Skyscraper v2 switch, so
    the openings verify under v1; they pin leaf layout, tree
    orientation and MultiPath encoding.
  * vectors.json          -- outputs of the pure-Python restatement oracle/pyref.py
    on seeded inputs (compress v1/v2 incl. edge inputs >= p, Montgomery products,
    RS-encode by naive evaluation, to_coeffs, eq table, cubic/quadratic sumcheck
    rounds, coefficient fold, PoW thresholds).  The reference has no vectors for
    these rows ("parity unpinned" at value level); pyref is an
    independent restatement of the definitions, and these vectors pin the C
    oracle and the HIP path to it.
"""
import ctypes
import json
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref as pr  # noqa: E402

FIXTURE = os.path.join(HERE, "poseidon-1000.np")


def hx(x):
    return "%064x" % x


# --------------------------------------------------------------------------- KATs
def kats():
    return {
        "source": "skyscraper/core/src/reference.rs:104-188; pow.rs:88-103; block-multiplier/proptest-regressions/scalar.txt",
        "sbox": [[0xCD, 0xD3], [0x17, 0x0E], [0x83, 0x17], [0x14, 0x28], [0x2B, 0x46], [0x1E, 0xBC]],
        "ss2": {
            "l": "11818428481613126259506041491792444971306025298632020312923851211664140080269",
            "r": "16089984100220651117533376273482359701319211672522891227502963383930673183481",
            "el": "2897520731550929941842826131888578795995028656093850302425034320680216166225",
            "er": "10274752619072178425540318899508997829349102488123199431506343228471746115261",
        },
        "bb6": {
            "l": "13251711941470795978907268022756015766767985221093713388330058285942871890923",
            "r": "1017722258958995329580328739423576514309327442471989504101393158056883989572",
            "el": "3193610555912363022088172260048956988022957239290210718020144819371540058981",
            "er": "17363210535454321713488811303876243393424286347736908007836172565366081010820",
        },
        "permute": [
            {
                "l": "0",
                "r": "0",
                "el": "5793276905781313965269111743763131906666794041798623267477617572701829069290",
                "er": "12296274483727574983376829575121280934973829438414198530604912453551798647077",
            },
            {
                "l": "50417215636675310123686652273432694184389644587803328798109154235492038730484",
                "r": "14620920779025509970947930308416120371903474543120179490887326852503500806990",
                "el": "8412949970293910117511617126618515787729842528183672400383899220234743146062",
                "er": "11868175801025513844525564200589229804433722826344843184417708742749423276015",
            },
        ],
        "sigma_inv": "9915499612839321149637521777990102151350674507940716049588462388200839649614",
        # (f64 bit pattern, expected [u64;4])
        "f64_to_u256": [
            [struct.unpack("<Q", struct.pack("<d", 0.0))[0], [0, 0, 0, 0]],
            [struct.unpack("<Q", struct.pack("<d", -1.7976931348623157e308))[0], [0, 0, 0, 0]],
            [struct.unpack("<Q", struct.pack("<d", 0.49))[0], [0, 0, 0, 0]],
            [struct.unpack("<Q", struct.pack("<d", 0.50))[0], [1, 0, 0, 0]],
            [struct.unpack("<Q", struct.pack("<d", 1.0))[0], [1, 0, 0, 0]],
            [struct.unpack("<Q", struct.pack("<d", 2.0**128))[0], [0, 0, 1, 0]],
            [0x7FF0000000000000, [2**64 - 1] * 4],
            [struct.unpack("<Q", struct.pack("<d", -42.0))[0], [0, 0, 0, 0]],
            [0x7FF0000000000001, [2**64 - 1] * 4],
        ],
        "scalar_mul_regressions": [
            {"l": [0, 0, 0, 1], "r": [0, 0, 0, 1]},
            {
                "l": [0, 887, 0, 15778841185528309819],
                "r": [458854615557053794, 8784556235901218364, 1751211468174275388, 16873806747226852460],
            },
        ],
    }


# --------------------------------------------------------------------------- fixture
def zstd_decompress(buf):
    z = ctypes.CDLL("libzstd.so.1")
    z.ZSTD_createDStream.restype = ctypes.c_void_p
    z.ZSTD_decompressStream.restype = ctypes.c_size_t
    z.ZSTD_decompressStream.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    z.ZSTD_initDStream.argtypes = [ctypes.c_void_p]
    z.ZSTD_freeDStream.argtypes = [ctypes.c_void_p]

    class Buf(ctypes.Structure):
        _fields_ = [("p", ctypes.c_void_p), ("size", ctypes.c_size_t), ("pos", ctypes.c_size_t)]

    ds = z.ZSTD_createDStream()
    z.ZSTD_initDStream(ds)
    src = ctypes.create_string_buffer(buf, len(buf))
    inb = Buf(ctypes.cast(src, ctypes.c_void_p), len(buf), 0)
    out = bytearray()
    chunk = ctypes.create_string_buffer(1 << 20)
    while True:
        outb = Buf(ctypes.cast(chunk, ctypes.c_void_p), len(chunk), 0)
        rc = z.ZSTD_decompressStream(ds, ctypes.byref(outb), ctypes.byref(inb))
        out += chunk.raw[: outb.pos]
        if rc == 0 or (inb.pos == inb.size and outb.pos == 0):
            break
    z.ZSTD_freeDStream(ds)
    return bytes(out)


def read_transcript():
    raw = open(FIXTURE, "rb").read()
    assert raw[:8] == bytes([0xDC, 0xDF, 0x4F, 0x5A, 0x6B, 0x70, 0x01, 0x00]) and raw[8:16] == b"NPSProof"
    body = zstd_decompress(raw[20:])
    n, shift, i = 0, 0, 0
    while True:  # postcard varint
        b = body[i]
        n |= (b & 0x7F) << shift
        i += 1
        shift += 7
        if not b & 0x80:
            break
    t = body[i : i + n]
    assert len(t) == n
    return t


class Rd:
    def __init__(self, b):
        self.b, self.i = b, 0

    def u64(self):
        v = struct.unpack_from("<Q", self.b, self.i)[0]
        self.i += 8
        return v

    def fe(self):
        v = int.from_bytes(self.b[self.i : self.i + 32], "little")
        self.i += 32
        return v


def parse_hint(t, off):
    ln = struct.unpack_from("<I", t, off)[0]
    return t[off + 4 : off + 4 + ln], off + 4 + ln


def parse_stir_answers(payload):
    rd = Rd(payload)
    n = rd.u64()
    out = []
    for _ in range(n):
        w = rd.u64()
        out.append([rd.fe() for _ in range(w)])
    assert rd.i == len(payload)
    return out


def parse_multipath(payload):
    rd = Rd(payload)
    sib = [rd.fe() for _ in range(rd.u64())]
    pre = [rd.u64() for _ in range(rd.u64())]
    suf = []
    for _ in range(rd.u64()):
        suf.append([rd.fe() for _ in range(rd.u64())])
    idx = [rd.u64() for _ in range(rd.u64())]
    assert rd.i == len(payload)
    return sib, pre, suf, idx


def decode_paths(pre, suf):
    """ark MultiPath -> per-leaf auth paths, root->leaf order (utilities.go:71-82)."""
    paths, prev = [], []
    for p, s in zip(pre, suf):
        cur = prev[:p] + s
        paths.append(cur)
        prev = cur
    return paths


def verify_opening(leaf, idx, sibling, path_root_to_leaf, root, version):
    c = pr.compress if version == 2 else pr.compress_v1
    h = pr.leaf_hash(leaf, version)
    h = c(sibling, h) if idx & 1 else c(h, sibling)
    idx >>= 1
    for s in reversed(path_root_to_leaf):
        h = c(s, h) if idx & 1 else c(h, s)
        idx >>= 1
    return h == root


# (hint offset of stir_answers, root offset) per SURVEY.md Appendix A
HINT_SETS = [
    ("blinding_T0", 3304, 96),
    ("blinding_T1", 39552, 3232),
    ("witness_T0", 47896, 0),
    ("witness_T1", 205744, 47824),
    ("witness_T2", 233384, 205672),
    ("witness_T3", 249248, 233312),
    ("witness_T4", 260056, 249176),
]
KEEP = {"blinding_T0": 32, "blinding_T1": 13, "witness_T0": 8, "witness_T1": 6, "witness_T2": 6, "witness_T3": 6, "witness_T4": 9}


def fixture_merkle():
    t = read_transcript()
    out = {"source": "tooling/provekit-bench/benches/poseidon-1000.np (Skyscraper v1)", "hash_version": 1, "trees": []}
    total = 0
    for name, off, root_off in HINT_SETS:
        root = int.from_bytes(t[root_off : root_off + 32], "little")
        pay, nxt = parse_hint(t, off)
        leaves = parse_stir_answers(pay)
        pay2, _ = parse_hint(t, nxt)
        sib, pre, suf, idx = parse_multipath(pay2)
        paths = decode_paths(pre, suf)
        assert len(leaves) == len(idx) == len(sib) == len(paths)
        ok = 0
        for lf, i, s, pth in zip(leaves, idx, sib, paths):
            assert verify_opening(lf, i, s, pth, root, 1), (name, i)
            assert not verify_opening(lf, i, s, pth, root, 2)
            ok += 1
        total += ok
        k = KEEP[name]
        out["trees"].append(
            {
                "name": name,
                "root": hx(root),
                "height": len(paths[0]) + 1,
                "leaf_width": len(leaves[0]),
                "n_openings_in_fixture": len(idx),
                "multipath": {  # raw ark MultiPath for the kept prefix is NOT prefix-closed, so keep decoded paths
                    "leaf_indexes": idx[:k],
                    "leaf_sibling_hashes": [hx(x) for x in sib[:k]],
                    "auth_paths_root_to_leaf": [[hx(x) for x in p] for p in paths[:k]],
                },
                "leaves": [[hx(x) for x in lf] for lf in leaves[:k]],
            }
        )
        print(f"{name}: {ok}/{len(idx)} openings verify under v1 (kept {k})")
    # the blinding tree is fully opened (32/32): keep its full MultiPath encoding as a Q1 vector
    pay, nxt = parse_hint(t, 3304)
    pay2, _ = parse_hint(t, nxt)
    sib, pre, suf, idx = parse_multipath(pay2)
    out["blinding_T0_multipath_raw"] = {
        "leaf_sibling_hashes": [hx(x) for x in sib],
        "auth_paths_prefix_lengths": pre,
        "auth_paths_suffixes": [[hx(x) for x in s] for s in suf],
        "leaf_indexes": idx,
        "serialized_hex": pay2.hex(),
    }
    assert total == 218
    return out


# --------------------------------------------------------------------------- pyref vectors
def vectors():
    rng = random.Random(0x5EED)
    fe = lambda: rng.randrange(pr.P)
    v = {}
    edge = [0, 1, pr.P - 1, pr.P, pr.P + 1, 2 * pr.P, 2**256 - 1, 2**255]
    pairs = [(a, b) for a in edge for b in edge] + [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(64)]
    v["compress_v2"] = [[hx(a), hx(b), hx(pr.compress(a, b))] for a, b in pairs]
    v["compress_v1"] = [[hx(a), hx(b), hx(pr.compress_v1(a, b))] for a, b in pairs]
    mm = [(fe(), fe()) for _ in range(32)] + [(0, 0), (1, 1), (pr.P - 1, pr.P - 1), (pr.R, pr.R)]
    v["mont_mul"] = [[hx(a), hx(b), hx(pr.mont_mul(a, b))] for a, b in mm]
    # leaf hash + tree (v2): 8 leaves x 32 wide, canonical values
    leaves = [[fe() for _ in range(32)] for _ in range(8)]
    dig = [pr.leaf_hash(l) for l in leaves]
    nodes = pr.merkle_nodes(dig)
    v["merkle_v2"] = {"leaves": [[hx(x) for x in l] for l in leaves], "nodes": [hx(x) for x in nodes]}
    # RS encode by the definition: batch 2, n=6, rate 1/2, fold 4 (SURVEY 8c vi) + a fold-2 case
    for name, batch, n, rho, fold in [("rs_b2_n6_r1_f4", 2, 6, 1, 4), ("rs_b1_n5_r2_f2", 1, 5, 2, 2), ("rs_b1_n4_r3_f4", 1, 4, 3, 4)]:
        polys = [[fe() for _ in range(1 << n)] for _ in range(batch)]
        lv = pr.rs_encode_naive(polys, n, rho, fold)
        v[name] = {
            "batch": batch, "n_vars": n, "log_inv_rate": rho, "fold": fold,
            "coeffs": [[hx(x) for x in p] for p in polys],
            "leaves": [[hx(x) for x in l] for l in lv],
        }
    ev = [fe() for _ in range(8)]
    v["to_coeffs_n3"] = {"evals": [hx(x) for x in ev], "coeffs": [hx(x) for x in pr.to_coeffs(ev)]}
    r3 = [fe() for _ in range(3)]
    v["eq_table_m3"] = {"r": [hx(x) for x in r3], "table": [hx(x) for x in pr.eq_table(r3)]}
    # cubic sumcheck: two rounds on 2^4 arrays (first without fold, second with)
    A, B, C, E = ([fe() for _ in range(16)] for _ in range(4))
    s0, *_ = pr.sumcheck_cubic_round(A, B, C, E)
    alpha = fe()
    s1, A2, B2, C2, E2 = pr.sumcheck_cubic_round(A, B, C, E, alpha)
    v["sumcheck_cubic"] = {
        "a": [hx(x) for x in A], "b": [hx(x) for x in B], "c": [hx(x) for x in C], "eq": [hx(x) for x in E],
        "round0": [hx(x) for x in s0], "alpha": hx(alpha), "round1": [hx(x) for x in s1],
        "a_folded": [hx(x) for x in A2],
    }
    F, W = [fe() for _ in range(16)], [fe() for _ in range(16)]
    q0, *_ = pr.sumcheck_quadratic_round(F, W)
    rr = fe()
    q1, F2, W2 = pr.sumcheck_quadratic_round(F, W, rr)
    v["sumcheck_quadratic"] = {
        "f": [hx(x) for x in F], "w": [hx(x) for x in W], "round0": [hx(x) for x in q0], "r": hx(rr),
        "round1": [hx(x) for x in q1], "f_folded": [hx(x) for x in F2],
    }
    cf = [fe() for _ in range(64)]
    r4 = [fe() for _ in range(4)]
    v["fold_coeffs"] = {"coeffs": [hx(x) for x in cf], "r": [hx(x) for x in r4], "out": [hx(x) for x in pr.fold_coeffs(cf, r4)]}
    z = fe()
    v["eval_univariate"] = {"z": hx(z), "out": hx(pr.eval_univariate(cf, z))}
    v["eq_univariate_n4"] = {"z": hx(z), "table": [hx(x) for x in pr.eq_table(pr.expand_from_univariate(z, 4))]}
    v["pow_threshold"] = [[d, hx(pr.pow_threshold(float(d)))] for d in range(0, 30)]
    v["root_of_unity"] = {str(k): hx(pr.root_of_unity(k)) for k in (1, 2, 4, 18, 23, 28)}
    return v


if __name__ == "__main__":
    json.dump(kats(), open(os.path.join(HERE, "skyscraper_kats.json"), "w"), indent=1)
    json.dump(fixture_merkle(), open(os.path.join(HERE, "fixture_merkle.json"), "w"))
    json.dump(vectors(), open(os.path.join(HERE, "vectors.json"), "w"))
    for f in ("skyscraper_kats.json", "fixture_merkle.json", "vectors.json"):
        print(f, os.path.getsize(os.path.join(HERE, f)))
