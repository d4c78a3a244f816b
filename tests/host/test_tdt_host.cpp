// CPU test binary for the HIP-free pieces of eagle_tdt / eagle_bed_tdt (csrc/eagle_host.h: tdt_words, tdt_d_bit, tdt_sign, tdt_families,
// tdt_arg_error), built by tests/test_tdt_abi.py with -fsanitize=address,undefined.  Exit code 0 = every check passed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../eagleeverything_amd/csrc/eagle_host.h"

static int g_fail = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } \
    } while (0)

static bool says(const char* got, const char* part) { return got && strstr(got, part); }

// Rule 2 by allele choices.  Codes: 0 hom A1, 1 het, 2 hom A2, 3 not called.  out = (PT, PU, MT, MU, W, complete).
static void by_alleles(int c, int f, int m, int out[6]) {
    for (int k = 0; k < 6; k++) out[k] = 0;
    if (c == 3 || f == 3 || m == 3) return;
    int fseen[2] = {0, 0}, mseen[2] = {0, 0}, any = 0;
    for (int a = 0; a <= 1; a++)                         // the allele the father passes, then the mother
        for (int b = 0; b <= 1; b++) {
            const bool fa = f == 1 || (f == 0 && a == 0) || (f == 2 && a == 1);
            const bool mb = m == 1 || (m == 0 && b == 0) || (m == 2 && b == 1);
            if (fa && mb && a + b == c) { fseen[a] = mseen[b] = 1; any = 1; }
        }
    if (!any) return;                                    // a Mendel error
    out[5] = 1;
    if (f == 1 && fseen[1] && !fseen[0]) out[0] = 1;
    if (f == 1 && fseen[0] && !fseen[1]) out[1] = 1;
    if (m == 1 && mseen[1] && !mseen[0]) out[2] = 1;
    if (m == 1 && mseen[0] && !mseen[1]) out[3] = 1;
    if (f == 1 && m == 1 && fseen[0] && fseen[1]) out[4] = 1;
}

// the lists live in heap blocks of their exact size, so that a read or write past one is an ASan report
static std::vector<int32_t> families_of(const std::vector<int32_t>& flat) {
    const long T = (long)flat.size() / 3;
    int32_t* p = (int32_t*)malloc(sizeof(int32_t) * (flat.size() ? flat.size() : 1));
    int32_t* o = (int32_t*)malloc(sizeof(int32_t) * (T ? T : 1));
    for (size_t i = 0; i < flat.size(); i++) p[i] = flat[i];
    tdt_families(p, T, o);
    std::vector<int32_t> out(o, o + T);
    free(p);
    free(o);
    return out;
}

static const char* arg_error(long markers, const std::vector<int32_t>& family, bool with_family, long first, long R) {
    const long T = (long)family.size();
    int32_t* p = (int32_t*)malloc(sizeof(int32_t) * (T ? T : 1));
    for (long i = 0; i < T; i++) p[i] = family[i];
    const char* r = tdt_arg_error(markers, T, with_family ? p : nullptr, first, R);
    free(p);
    return r;
}

int main() {
    // the plane formulas equal the enumeration on all 64 code triples, one triple a bit; 11 are informative
    {
        uint64_t A[3] = {0, 0, 0}, B[3] = {0, 0, 0}, C[3] = {0, 0, 0}, want[6] = {0, 0, 0, 0, 0, 0};
        int bit = 0, informative = 0;
        for (int c = 0; c < 4; c++)
            for (int f = 0; f < 4; f++)
                for (int m = 0; m < 4; m++, bit++) {
                    const int code[3] = {c, f, m};
                    for (int k = 0; k < 3; k++) {
                        if (code[k] == 0) A[k] |= 1ull << bit;
                        if (code[k] == 2) B[k] |= 1ull << bit;
                        if (code[k] != 3) C[k] |= 1ull << bit;
                    }
                    int o[6];
                    by_alleles(c, f, m, o);
                    for (int k = 0; k < 6; k++)
                        if (o[k]) want[k] |= 1ull << bit;
                    informative += o[5] && (f == 1 || m == 1);
                }
        CHECK(bit == 64 && informative == 11);
        const TdtWords t = tdt_words(A[0], B[0], C[0], A[1], B[1], C[1], A[2], B[2], C[2]);
        CHECK(t.pt == want[0] && t.pu == want[1] && t.mt == want[2] && t.mu == want[3] && t.w == want[4] && t.k == want[5]);
        CHECK(__builtin_popcountll(t.k) == 27 - 12);     // the 27 called triples less the 12 errors among them
        CHECK(__builtin_popcountll(t.hf) + __builtin_popcountll(t.hm) ==
              __builtin_popcountll(t.pt) + __builtin_popcountll(t.pu) + __builtin_popcountll(t.mt) + __builtin_popcountll(t.mu) + 2 * __builtin_popcountll(t.w));
        CHECK((t.pt & t.pu) == 0 && (t.mt & t.mu) == 0 && (t.w & (t.pt | t.pu | t.mt | t.mu)) == 0);
        for (int b = 0; b < 64; b++) {
            const int d = tdt_d_bit(t, b);
            CHECK(d >= -2 && d <= 2 && d == (int)((want[0] >> b) & 1) + (int)((want[2] >> b) & 1) - (int)((want[1] >> b) & 1) - (int)((want[3] >> b) & 1));
        }
        // an unknown parent (zero words) or a child that is called nowhere: nothing
        const TdtWords u = tdt_words(A[0], B[0], C[0], 0, 0, 0, A[2], B[2], C[2]), v = tdt_words(0, 0, 0, A[1], B[1], C[1], A[2], B[2], C[2]);
        CHECK((u.k | u.hf | u.hm | u.pt | u.pu | u.mt | u.mu | u.w) == 0 && (v.k | v.hf | v.hm | v.pt | v.pu | v.mt | v.mu | v.w) == 0);
        // the image route: three hets inside the word mask are W and nothing else; bits past the last marker are nothing
        const uint64_t mask = mendel_word_mask(1, 70);
        const TdtWords h = tdt_words(0, 0, mask, 0, 0, mask, 0, 0, mask);
        CHECK(h.w == 0x3full && h.k == 0x3full && h.hf == 0x3full && (h.pt | h.pu | h.mt | h.mu) == 0);
        // swapping the alleles swaps transmitted and untransmitted
        const TdtWords s = tdt_words(B[0], A[0], C[0], B[1], A[1], C[1], B[2], A[2], C[2]);
        CHECK(s.pt == t.pu && s.pu == t.pt && s.mt == t.mu && s.mu == t.mt && s.w == t.w && s.k == t.k);
    }

    // the sign rule: bit 31 of maxt_mix; both signs occur; the counter is r 2^16 + phi + 1
    {
        int minus = 0;
        for (uint32_t phi = 0; phi < 1000; phi++) {
            const int sg = tdt_sign(7, 3, phi);
            CHECK(sg == ((maxt_mix(7, 3, phi) >> 31) ? -1 : 1));
            minus += sg < 0;
        }
        CHECK(minus > 400 && minus < 600);
        CHECK(tdt_sign(7, 3, 65535) == tdt_sign(7, 3, 65535) && maxt_mix(7, 2, 65536) == maxt_mix(7, 3, 0));
    }

    // the family rule: the smallest list position with the same couple
    CHECK((families_of({4, 0, 1, 5, 2, 3, 6, 0, 1, 7, 2, 3, 8, 0, 3, 9, 0, -1, 10, 0, -1}) == std::vector<int32_t>{0, 1, 0, 1, 4, 5, 5}));
    CHECK((families_of({4, 1, 0, 5, 0, 1, 6, -1, -1, 7, -1, -1, 8, 1, 0}) == std::vector<int32_t>{0, 1, 2, 2, 0}));
    CHECK((families_of({2, 0, 1}) == std::vector<int32_t>{0}) && families_of({}).empty());

    // the argument rule
    CHECK(arg_error(1000, {0}, false, 1, 0) == nullptr && arg_error(0x7fffffffL, {0}, false, 0, 0) == nullptr);
    CHECK(tdt_arg_error(10, MENDEL_MAX_TRIOS, nullptr, 1, 0) == nullptr && says(tdt_arg_error(10, MENDEL_MAX_TRIOS + 1, nullptr, 1, 0), "number of trios"));
    CHECK(says(tdt_arg_error(10, 0, nullptr, 1, 0), "number of trios") && says(tdt_arg_error(1L << 31, 1, nullptr, 1, 0), "2^31 markers"));
    CHECK(says(tdt_arg_error(10, 1, nullptr, 1, -1), "negative"));
    CHECK(tdt_arg_error(10, TDT_MAX_FLIP_TRIOS, nullptr, 1, 1) == nullptr && says(tdt_arg_error(10, TDT_MAX_FLIP_TRIOS + 1, nullptr, 1, 1), "65535 trios"));
    CHECK(tdt_arg_error(10, 1, nullptr, 1, MAXT_RMAX) == nullptr && says(tdt_arg_error(10, 1, nullptr, 1, MAXT_RMAX + 1), "1024"));
    CHECK(says(tdt_arg_error(10, 1, nullptr, 0, 1), "first must be at least 1"));
    CHECK(tdt_arg_error(10, 1, nullptr, 2147483647L, 1) == nullptr && says(tdt_arg_error(10, 1, nullptr, 2147483647L, 2), "above 2^31"));
    CHECK(arg_error(10, {0, 65535, 7}, true, 1, 1) == nullptr);
    CHECK(says(arg_error(10, {0, 65536, 7}, true, 1, 1), "family") && says(arg_error(10, {0, 1, -1}, true, 1, 1), "family"));
    CHECK(arg_error(10, {0, 65536, -1}, true, 1, 0) == nullptr);     // R = 0: the families are not read

    if (g_fail) {
        fprintf(stderr, "%d tdt host checks FAILED\n", g_fail);
        return 1;
    }
    printf("tdt host checks passed\n");
    return 0;
}
