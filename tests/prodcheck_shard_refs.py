"""The ownership rule of a sharded product sumcheck (include/provekit_sumcheck_sharded.h) and what a sharded prover's arena holds,
restated on Python ints from the header's text.  TEST INFRASTRUCTURE ONLY.

G = 2^g ranks, chunks of 2^c = 256 elements: rank r owns the indices whose bits [c, c + g) spell r, and its compacted index drops
those bits.  Round i of n is sharded iff n - 1 - i >= c + g."""
C = 8
MAX_GRID, MAX_TERM_TABLES = 1024, 3


def log2(G):
    g = G.bit_length() - 1
    assert G == 1 << g
    return g


def owner(x, g):
    return (x >> C) & ((1 << g) - 1)


def compact(x, g):
    return (x >> (C + g)) << C | (x & ((1 << C) - 1))


def expand(y, g, r):
    return (y >> C) << (C + g) | r << C | (y & ((1 << C) - 1))


def sharded_rounds(n, g):
    return max(0, n - C - g)


def owned(n, g, r):
    """rank r's indices of a table of 2^n, ascending"""
    return [x for x in range(1 << n) if owner(x, g) == r]


def compacted(table, g, r):
    """rank r's compacted table of a full table (whole chunks per rank: len(table) >= 2^(c+g))"""
    return [table[expand(y, g, r)] for y in range(len(table) >> g)]


def eq_split_elements(R):
    """the two split eq tables' suffix levels for R coordinates: H = R - R // 2 leading, L = R // 2 trailing"""
    L = R // 2
    H = R - L
    return (2 << H) + (2 << L) - 2


def arena_elements(n, m, G):
    """A rank's arena, from the header's list, in field elements:
      the compacted tables: m x 2^(n-1) / G from S = 2 on (round 1 is the first to store; with S < 2 no sharded round stores)
    + the replicated tables the hand-over fills and the replicated rounds fold in place: m x 2^(c+g+1)
    + the hand-over's gather: the rank's block of m x 2^(c+1) and the G gathered blocks
    + a round's exchange: (D_max + 1 sums + 1 status element) = 5 elements sent, G x 5 received
    + the round scratch: 4 x MAX_GRID partial sums and 8 results
    + the split eq tables of the n - 1 coordinates after tau_0
    Only the first line depends on the tables' share"""
    g = log2(G)
    S = sharded_rounds(n, g)
    compact_part = m * ((1 << (n - 1)) >> g) if S >= 2 else 0
    return (compact_part + m * (1 << (C + g + 1)) + (1 + G) * m * (1 << (C + 1)) + (1 + G) * (MAX_TERM_TABLES + 2) + 4 * MAX_GRID + 8
            + eq_split_elements(n - 1))


def plan(n, m, G):
    """-> (g, c, S, local_len, handover_len, arena_bytes)"""
    g = log2(G)
    S = sharded_rounds(n, g)
    return g, C, S, ((1 << n) >> g) if S else 0, 1 << (C + g + 1), 32 * arena_elements(n, m, G)
