// CPU test binary for the marker range plan of the admixture step (csrc/eagle_host.h: admix_range_plan, admix_part_cap), built by
// tests/test_admixture_plan_host.py with -fsanitize=address,undefined.  For every (n, L) of the sweep the ranges cover [0, L) exactly
// once and in order, every boundary but L itself is a multiple of 16, no range is empty, and the partials buffer S * n16 * 16 * 8 bytes
// stays within the stated cap.  Exit code 0 = every check passed.
#include <stdio.h>
#include <stdlib.h>

#include "../../eagleeverything_amd/csrc/eagle_host.h"

static int g_fail = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } \
    } while (0)

static void check(long n, long L) {
    const AdmixPlan p = admix_range_plan(n, L);
    const AdmixPlan again = admix_range_plan(n, L);
    CHECK(p.S == again.S && p.len == again.len);
    CHECK(p.S >= 1 && p.S <= 65535);
    CHECK(p.len >= 16 && p.len % 16 == 0);
    long next = 0;
    for (long s = 0; s < p.S; s++) {
        const long lo = s * p.len, hi = std::min(L, (s + 1) * p.len);
        CHECK(lo == next);          // no gap, no overlap
        CHECK(lo % 16 == 0);
        CHECK(hi > lo);             // no empty range
        CHECK(hi == L || hi % 16 == 0);
        next = hi;
    }
    CHECK(next == L);
    const long n16 = (n + 15) / 16 * 16;
    CHECK(p.S * n16 * 16 * 8 <= admix_part_cap(n));
    CHECK(admix_part_cap(n) >= ADMIX_PART_BYTES);
    if (g_fail) fprintf(stderr, "  at n = %ld, L = %ld: S = %ld, len = %ld\n", n, L, p.S, p.len);
}

int main() {
    const long ns[] = {1, 16, 10000, 15, 17, 1003, 600000, (1L << 30) - 1};
    const long Ls[] = {1, 15, 16, 17, 4097, 1000000, 31, 32, 33, 255, 256, 257};
    for (long n : ns)
        for (long L : Ls) check(n, L);
    // hand-written: one tile of individuals and 4097 markers -> 257 marker tiles, one range each
    AdmixPlan p = admix_range_plan(16, 4097);
    CHECK(p.S == 257 && p.len == 16);
    // 10000 individuals = 625 tiles -> ceil(2048 / 625) = 4 ranges of ceil(62500 / 4) = 15625 marker tiles
    p = admix_range_plan(10000, 1000000);
    CHECK(p.S == 4 && p.len == 15625 * 16);
    // a short panel is never cut below one marker tile
    p = admix_range_plan(1, 1);
    CHECK(p.S == 1 && p.len == 16);
    if (g_fail) {
        fprintf(stderr, "%d admixture plan check(s) failed\n", g_fail);
        return 1;
    }
    printf("admixture plan host checks passed\n");
    return 0;
}
