// asan_main.cpp -- driver of the sanitizer build of this library's host code (make asan; CPU code only):
//   pks_verify_asan verify <case file>
//       u32 n, m, T, has_tau, n_bind, masks[4] | u64 coeffs[4][4] | u32 with_expected | u32 pattern length | pattern |
//       tau (n elements, if has_tau) | bind (n_bind elements) | expected sum (if with_expected) | u32 count | count x (u64 length | bytes)
//     verifies every proof with pks_verify and prints "rc accepted check offset" per proof.  A statement the library refuses prints one
//     REFUSED line and nothing of the rest is read: its counts size nothing.  Proofs, tau and bind live in exact-size heap blocks, so
//     that a read past an end is a report, not a read of the next item.
//   pks_verify_asan lane <D> <lo> <hi> <coeff> <weight> <repeats>        (64 hex digits each, the raw 256-bit value, big-endian)
//     runs lane.hpp's lane_accumulate<D, D> -- the kernel's arithmetic, compiled for the host -- `repeats` times on D tables that all hold
//     (lo, hi), one term over all of them, and prints the D + 1 sums the same way.
//   pks_verify_asan lanes <D> <m> <T> <weighted 0|1> <weight> <repeats> T x (<mask> <coeff>) m x (<lo> <hi>)
//     runs lane_accumulate<D, m> for any (D, m) round.hip dispatches on the caller's terms (mask in decimal; the coefficient's kind is
//     lane.hpp's coeff_kind of it, as the kernel's caller takes it) and per-table (lo, hi), weighted or not, and prints the same.
//   pks_verify_asan shard <n> <world> [lone]
//     drives shard.hpp's ownership rule and pkss_plan for tables of 2^n (n <= 20) and `world` ranks.  It marks, in exact-size heap
//     blocks, the slot expand(y, g, r) of every rank r and compacted index y < 2^n / world -- an index outside the table is a report --
//     and checks that every slot is marked once, that owner and compact invert expand, and the pair property at every sharded round
//     length.  Then pkss_plan for m = 1 .. 4 at this (n, world): prints "n m g c S local_len handover_len arena_bytes" per line, or the
//     refusal.  With `lone`, one more column: the bytes of the lone prover's arena at this (n, m), the layout of a device set of one.
//     exit 1: the rule is not a bijection.
//   pks_verify_asan wide verify <case file>
//       u32 n, m, T, has_tau, n_bind, lens[16], factors[16][5] | u64 coeffs[16][4] | then as `verify`
//     the same for a wide statement (provekit_sumcheck_wide.h) and pksw_verify.
//   pks_verify_asan wide lane <D> <m> <T> <weighted 0|1> <weight> <repeats> T x (<indices joined by '.'> <coeff>) m x (<lo> <hi>)
//     runs wide_lane.hpp's wide_lane_accumulate<D> -- the wide kernel's arithmetic, compiled for the host -- on the caller's terms (the
//     kinds and the packed lists taken by wide_terms, as wide.hip's launch takes them) and per-table (lo, hi), and prints the D + 1 sums.
#include <string>

#include "../../../include/provekit_sumcheck.h"
#include "../asan_case.hpp"
#include "lane.hpp"
#include "layout.hpp"
#include "wide_lane.hpp"

namespace {

using asan_case::take;
using asan_case::take_block;

int run_verify(const char* path) {
    if (!asan_case::read_file(path)) return 2;
    pks_statement st;
    memset(&st, 0, sizeof st);
    uint32_t head[9];
    take(head, sizeof head);
    st.n = head[0], st.m = head[1], st.T = head[2], st.has_tau = head[3], st.n_bind = head[4];
    for (int t = 0; t < 4; t++) st.masks[t] = head[5 + t];
    take(st.coeffs, sizeof st.coeffs);
    size_t proof_len = 0;
    if (int rc = pks_proof_bytes(&st, &proof_len)) {
        printf("%d 0 REFUSED 0 %s\n", rc, pks_create_error());
        return 0;
    }
    uint32_t with_expected, pattern_len;
    take(&with_expected, 4);
    take(&pattern_len, 4);
    uint8_t* pattern = (uint8_t*)take_block(pattern_len);
    uint64_t* tau = st.has_tau ? (uint64_t*)take_block(32 * (size_t)st.n) : nullptr;
    uint64_t* bind = st.n_bind ? (uint64_t*)take_block(32 * (size_t)st.n_bind) : nullptr;
    uint64_t* expected = with_expected ? (uint64_t*)take_block(32) : nullptr;
    uint32_t count;
    take(&count, 4);
    uint64_t* point = (uint64_t*)malloc(32 * (size_t)st.n);
    uint64_t* finals = (uint64_t*)malloc(32 * (size_t)st.m);
    for (uint32_t c = 0; c < count; c++) {
        uint64_t len;
        take(&len, 8);
        uint8_t* proof = (uint8_t*)take_block(len);
        pkv_result r;
        const int rc = pks_verify(&st, pattern_len ? pattern : nullptr, pattern_len, tau, bind, expected, proof, len, point, finals, &r);
        if (rc)
            printf("%d 0 REFUSED 0 %s\n", rc, pks_create_error());
        else
            printf("0 %d %s %llu\n", r.accepted, pks_check_name(r.check), (unsigned long long)r.offset);
        free(proof);
    }
    free(point), free(finals), free(expected), free(bind), free(tau), free(pattern);
    return 0;
}

bool parse_hex(const char* s, pk::fe& out) {
    if (strlen(s) != 64) return false;
    for (int i = 0; i < 8; i++) {
        char word[9] = {0};
        memcpy(word, s + 8 * (7 - i), 8);
        char* end;
        out.v[i] = (uint32_t)strtoul(word, &end, 16);
        if (*end) return false;
    }
    return true;
}
void print_hex(const pk::fe& x) {
    for (int i = 7; i >= 0; i--) printf("%08x", x.v[i]);
    printf("\n");
}

template <int D>
void lane(const pk::fe& lo_v, const pk::fe& hi_v, const pk::fe& coeff, const pk::fe& w, unsigned repeats) {
    pk::fe lo[D], hi[D], acc[D + 1];
    for (int j = 0; j < D; j++) lo[j] = lo_v, hi[j] = hi_v;
    for (int k = 0; k <= D; k++) acc[k] = pk::fe_zero();
    pks::Terms tm;
    memset(&tm, 0, sizeof tm);
    tm.T = 1, tm.masks[0] = (1u << D) - 1, tm.kind[0] = pks::COEFF_ANY, tm.coeff[0] = coeff;
    for (unsigned r = 0; r < repeats; r++) pks::lane_accumulate<D, D>(lo, hi, tm, true, w, acc);
    for (int k = 0; k <= D; k++) print_hex(acc[k]);
}

int run_lane(int argc, char** argv) {
    pk::fe v[4];
    if (argc != 8) return 2;
    for (int i = 0; i < 4; i++)
        if (!parse_hex(argv[3 + i], v[i])) return 2;
    const int D = atoi(argv[2]);
    const unsigned repeats = (unsigned)atoi(argv[7]);
    if (D == 1)
        lane<1>(v[0], v[1], v[2], v[3], repeats);
    else if (D == 2)
        lane<2>(v[0], v[1], v[2], v[3], repeats);
    else if (D == 3)
        lane<3>(v[0], v[1], v[2], v[3], repeats);
    else
        return 2;
    return 0;
}

template <int D, int M>
void lanes(const pk::fe* lo_v, const pk::fe* hi_v, const pks::Terms& tm, bool weighted, const pk::fe& w, unsigned repeats) {
    pk::fe lo[M], hi[M], acc[D + 1];
    for (int j = 0; j < M; j++) lo[j] = lo_v[j], hi[j] = hi_v[j];
    for (int k = 0; k <= D; k++) acc[k] = pk::fe_zero();
    for (unsigned r = 0; r < repeats; r++) pks::lane_accumulate<D, M>(lo, hi, tm, weighted, w, acc);
    for (int k = 0; k <= D; k++) print_hex(acc[k]);
}

int run_lanes(int argc, char** argv) {
    if (argc < 8) return 2;
    const unsigned D = (unsigned)atoi(argv[2]), m = (unsigned)atoi(argv[3]), T = (unsigned)atoi(argv[4]);
    const bool weighted = atoi(argv[5]) != 0;
    const unsigned repeats = (unsigned)atoi(argv[7]);
    pk::fe w, lo[PKS_MAX_TABLES], hi[PKS_MAX_TABLES];
    if (m < 1 || m > PKS_MAX_TABLES || T < 1 || T > PKS_MAX_TERMS || (unsigned)argc != 8 + 2 * T + 2 * m || !parse_hex(argv[6], w)) return 2;
    pks::Terms tm;
    memset(&tm, 0, sizeof tm);
    tm.T = T;
    unsigned degree = 0;
    for (unsigned t = 0; t < T; t++) {
        tm.masks[t] = (unsigned)atoi(argv[8 + 2 * t]);
        if (!tm.masks[t] || tm.masks[t] >> m || !parse_hex(argv[9 + 2 * t], tm.coeff[t])) return 2;
        tm.kind[t] = pks::coeff_kind(tm.coeff[t]);
        const unsigned bits = (unsigned)__builtin_popcount(tm.masks[t]);
        degree = bits > degree ? bits : degree;
    }
    if (degree != D) return 2;  // the kernel's caller takes D from the masks
    for (unsigned j = 0; j < m; j++)
        if (!parse_hex(argv[8 + 2 * T + 2 * j], lo[j]) || !parse_hex(argv[9 + 2 * T + 2 * j], hi[j])) return 2;
#define PKS_CASE(DEG, TABLES) \
    if (D == DEG && m == TABLES) return lanes<DEG, TABLES>(lo, hi, tm, weighted, w, repeats), 0;
    PKS_CASE(1, 1) PKS_CASE(1, 2) PKS_CASE(1, 3) PKS_CASE(1, 4) PKS_CASE(2, 2) PKS_CASE(2, 3) PKS_CASE(2, 4) PKS_CASE(3, 3) PKS_CASE(3, 4)
#undef PKS_CASE
    return 2;
}

int run_shard(unsigned n, unsigned world, bool lone) {
    pks_statement st;
    memset(&st, 0, sizeof st);
    st.n = n, st.T = 1;
    const pk::fe one = pk::fe_one();
    memcpy(st.coeffs[0], one.v, 32);
    for (unsigned m = 1; m <= 4; m++) {
        st.m = m, st.masks[0] = (1u << m) - 1;
        if (m == 4) st.T = 2, st.masks[0] = 7, st.masks[1] = 8, memcpy(st.coeffs[1], one.v, 32);  // a term has at most 3 tables
        struct pkss_plan plan;
        if (int rc = pkss_plan(&st, world, &plan)) {
            printf("%d REFUSED %s\n", rc, pks_create_error());
            return 0;  // n and world are refused whatever m is
        }
        printf("%u %u %u %u %u %zu %zu %zu", n, m, plan.g, plan.c, plan.S, plan.local_len, plan.handover_len, plan.arena_bytes);
        if (lone) printf(" %zu", 32 * pkss::layout(n, m, 0).total);
        printf("\n");
        if (m > 1 || n > 20 || n < PKSS_CHUNK_LOG2 + plan.g) continue;  // the rule itself once, where every rank owns whole chunks
        const unsigned g = plan.g;
        const size_t N = (size_t)1 << n, local = N >> g;
        uint8_t* seen = (uint8_t*)calloc(N, 1);
        for (unsigned r = 0; r < world; r++)
            for (size_t y = 0; y < local; y++) {
                const size_t x = pkss::expand(y, g, r);
                if (y && x <= pkss::expand(y - 1, g, r)) return free(seen), 1;  // in order
                if (pkss::owner(x, g) != r || pkss::compact(x, g) != y) return free(seen), 1;
                seen[x]++;
            }
        for (size_t x = 0; x < N; x++)
            if (seen[x] != 1) return free(seen), 1;
        free(seen);
        for (unsigned i = 0; pkss::round_is_sharded(n, i, g); i++) {  // the pair (x, x + len/2) compacts to (y, y + len_local/2)
            const size_t len = N >> i;
            for (size_t x = 0; x < len / 2; x++)
                if (pkss::owner(x + len / 2, g) != pkss::owner(x, g) || pkss::compact(x + len / 2, g) != pkss::compact(x, g) + (len >> g) / 2) return 1;
        }
        if (pkss::sharded_rounds(n, g) != plan.S) return 1;
    }
    return 0;
}

int run_wide_verify(const char* path) {
    if (!asan_case::read_file(path)) return 2;
    pksw_statement st;
    memset(&st, 0, sizeof st);
    uint32_t head[5];
    take(head, sizeof head);
    st.n = head[0], st.m = head[1], st.T = head[2], st.has_tau = head[3], st.n_bind = head[4];
    take(st.lens, sizeof st.lens);
    take(st.factors, sizeof st.factors);
    take(st.coeffs, sizeof st.coeffs);
    size_t proof_len = 0;
    if (int rc = pksw_proof_bytes(&st, &proof_len)) {
        printf("%d 0 REFUSED 0 %s\n", rc, pksw_create_error());
        return 0;
    }
    uint32_t with_expected, pattern_len;
    take(&with_expected, 4);
    take(&pattern_len, 4);
    uint8_t* pattern = (uint8_t*)take_block(pattern_len);
    uint64_t* tau = st.has_tau ? (uint64_t*)take_block(32 * (size_t)st.n) : nullptr;
    uint64_t* bind = st.n_bind ? (uint64_t*)take_block(32 * (size_t)st.n_bind) : nullptr;
    uint64_t* expected = with_expected ? (uint64_t*)take_block(32) : nullptr;
    uint32_t count;
    take(&count, 4);
    uint64_t* point = (uint64_t*)malloc(32 * (size_t)st.n);
    uint64_t* finals = (uint64_t*)malloc(32 * (size_t)st.m);
    for (uint32_t c = 0; c < count; c++) {
        uint64_t len;
        take(&len, 8);
        uint8_t* proof = (uint8_t*)take_block(len);
        pkv_result r;
        const int rc = pksw_verify(&st, pattern_len ? pattern : nullptr, pattern_len, tau, bind, expected, proof, len, point, finals, &r);
        if (rc)
            printf("%d 0 REFUSED 0 %s\n", rc, pksw_create_error());
        else
            printf("0 %d %s %llu\n", r.accepted, pks_check_name(r.check), (unsigned long long)r.offset);
        free(proof);
    }
    free(point), free(finals), free(expected), free(bind), free(tau), free(pattern);
    return 0;
}

template <int D>
void wide_lane(const pk::fe* lo, const pk::fe* hi, const pks::WideTerms& tm, bool weighted, const pk::fe& w, unsigned repeats) {
    pk::fe acc[D + 1];
    for (int k = 0; k <= D; k++) acc[k] = pk::fe_zero();
    auto load = [&](unsigned j, pk::fe& l, pk::fe& h) { l = lo[j], h = hi[j]; };
    for (unsigned r = 0; r < repeats; r++) pks::wide_lane_accumulate<D>(tm, load, weighted, w, acc);
    for (int k = 0; k <= D; k++) print_hex(acc[k]);
}

int run_wide_lane(int argc, char** argv) {  // argv[3 ..]: D m T weighted weight repeats, the terms, the pairs
    if (argc < 9) return 2;
    pksw_statement st;
    memset(&st, 0, sizeof st);
    const unsigned D = (unsigned)atoi(argv[3]);
    st.n = 1, st.m = (unsigned)atoi(argv[4]), st.T = (unsigned)atoi(argv[5]);
    const bool weighted = atoi(argv[6]) != 0;
    const unsigned repeats = (unsigned)atoi(argv[8]);
    pk::fe w, lo[PKSW_MAX_TABLES], hi[PKSW_MAX_TABLES];
    if (st.m < 1 || st.m > PKSW_MAX_TABLES || st.T < 1 || st.T > PKSW_MAX_TERMS || (unsigned)argc != 9 + 2 * st.T + 2 * st.m || !parse_hex(argv[7], w)) return 2;
    for (unsigned t = 0; t < st.T; t++) {
        for (const char* c = argv[9 + 2 * t]; *c; c++) {
            if (st.lens[t] >= PKSW_MAX_DEGREE) return 2;
            char* end;
            st.factors[t][st.lens[t]++] = (unsigned)strtoul(c, &end, 10);
            if (end == c || (*end && *end != '.')) return 2;
            c = *end ? end : end - 1;
        }
        pk::fe coeff;
        if (!parse_hex(argv[10 + 2 * t], coeff)) return 2;
        memcpy(st.coeffs[t], coeff.v, 32);
    }
    std::string why;
    if (!pks::statement_ok(&st, why) || pks::degree(st) != D) return fprintf(stderr, "%s\n", why.c_str()), 2;  // the kernel's caller takes D from the lists
    for (unsigned j = 0; j < st.m; j++)
        if (!parse_hex(argv[9 + 2 * st.T + 2 * j], lo[j]) || !parse_hex(argv[10 + 2 * st.T + 2 * j], hi[j])) return 2;
    const pks::WideTerms tm = pks::wide_terms(st);
#define PKSW_DEGREE(DEG) \
    if (D == DEG) return wide_lane<DEG>(lo, hi, tm, weighted, w, repeats), 0;
    PKSW_DEGREE(1) PKSW_DEGREE(2) PKSW_DEGREE(3) PKSW_DEGREE(4) PKSW_DEGREE(5)
#undef PKSW_DEGREE
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "wide") && !strcmp(argv[2], "verify")) return run_wide_verify(argv[3]);
    if (argc >= 3 && !strcmp(argv[1], "wide") && !strcmp(argv[2], "lane")) return run_wide_lane(argc, argv);
    if (argc == 3 && !strcmp(argv[1], "verify")) return run_verify(argv[2]);
    if (argc >= 2 && !strcmp(argv[1], "lane")) return run_lane(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "lanes")) return run_lanes(argc, argv);
    const bool lone = argc == 5 && !strcmp(argv[4], "lone");
    if ((argc == 4 || lone) && !strcmp(argv[1], "shard")) return run_shard((unsigned)atoi(argv[2]), (unsigned)atoi(argv[3]), lone);
    fprintf(stderr, "usage: pks_verify_asan verify <case file> | lane <D> <lo> <hi> <coeff> <weight> <repeats> | "
                    "lanes <D> <m> <T> <weighted> <weight> <repeats> T x (<mask> <coeff>) m x (<lo> <hi>) | shard <n> <world> [lone] | "
                    "wide verify <case file> | wide lane <D> <m> <T> <weighted> <weight> <repeats> T x (<i.j.k> <coeff>) m x (<lo> <hi>)\n");
    return 2;
}
