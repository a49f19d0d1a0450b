// feinv_asan_main.cpp -- driver of the sanitizer build of the safegcd inverse's parts (make asan; CPU code only):
//   pk_feinv_asan IN OUT
//     IN:  groups of { int32 part, int32 n, n records of 32 int32 } back to back (the records of selftest_inv30.hpp)
//     OUT: the n records of 32 int32 each group returns, back to back in the same order
//     runs selftest_inv30 -- the functions of feinv.hpp themselves -- on every record under AddressSanitizer + UBSan: the signed sums
//     of update_de (md, me, the 64-bit columns, the top limbs) and of normalize at the ends of their stated ranges are what it is for.
//     Every group lives in heap blocks of exactly its size.  tests/test_feinv_host.py writes IN from tests/feinv_refs.py and compares
//     OUT with the definition.  Prints "feinv parts ok: <groups> groups, <records> records"; exit 1 on a malformed file or an unknown part.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "selftest_inv30.hpp"

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 1;
    }
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fi ? fopen(argv[2], "wb") : nullptr;
    if (!fi || !fo) {
        fprintf(stderr, "cannot open %s\n", fi ? argv[2] : argv[1]);
        return 1;
    }
    size_t groups = 0, records = 0;
    int32_t head[2];
    while (fread(head, sizeof(int32_t), 2, fi) == 2) {
        if (head[1] < 0 || head[1] > (1 << 24)) {
            fprintf(stderr, "group %zu: bad record count %d\n", groups, head[1]);
            return 1;
        }
        const size_t n = (size_t)head[1];
        std::vector<int32_t> in(32 * n), out(32 * n);
        if (fread(in.data(), sizeof(int32_t), 32 * n, fi) != 32 * n) {
            fprintf(stderr, "group %zu: truncated\n", groups);
            return 1;
        }
        for (size_t i = 0; i < n; i++)
            if (!pk::selftest_inv30(head[0], in.data() + 32 * i, out.data() + 32 * i)) {
                fprintf(stderr, "group %zu: no part %d\n", groups, head[0]);
                return 1;
            }
        if (fwrite(out.data(), sizeof(int32_t), 32 * n, fo) != 32 * n) {
            fprintf(stderr, "group %zu: short write\n", groups);
            return 1;
        }
        groups++;
        records += n;
    }
    if (fclose(fo) != 0) return 1;
    fclose(fi);
    printf("feinv parts ok: %zu groups, %zu records\n", groups, records);
    return 0;
}
