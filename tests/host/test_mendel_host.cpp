// CPU test binary for the HIP-free pieces of eagle_mendel / eagle_parentage (csrc/eagle_host.h: mendel_xuv, mendel_error_word,
// mendel_word_mask, mendel_arg_error, mendel_trios_check, parentage_arg_error, parentage_list_check, parentage_ordinal), built by
// tests/test_mendel_abi.py with -fsanitize=address,undefined.  Exit code 0 = every check passed.
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

// Rule 3 by allele sets.  Codes: 0 hom A1, 1 het, 2 hom A2, 3 not called.
static bool error_by_alleles(int c, int f, int m) {
    if (c == 3) return false;
    const int want = c;                                  // the number of A2 alleles of the child
    for (int a = 0; a <= 1; a++)
        for (int b = 0; b <= 1; b++) {
            const bool fa = f == 3 || f == 1 || (f == 0 && a == 0) || (f == 2 && a == 1);
            const bool mb = m == 3 || m == 1 || (m == 0 && b == 0) || (m == 2 && b == 1);
            if (fa && mb && a + b == want) return false;
        }
    return true;
}

// the lists live in heap blocks of their exact size, so that a read past one is an ASan report
static long trios_check(const std::vector<int32_t>& flat, long n) {
    int32_t* p = (int32_t*)malloc(sizeof(int32_t) * (flat.size() ? flat.size() : 1));
    for (size_t i = 0; i < flat.size(); i++) p[i] = flat[i];
    const long r = mendel_trios_check(p, (long)flat.size() / 3, n);
    free(p);
    return r;
}

static long list_check(const std::vector<int32_t>& v, long n, bool* dup) {
    int32_t* p = v.empty() ? nullptr : (int32_t*)malloc(sizeof(int32_t) * v.size());
    for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
    const long r = parentage_list_check(p, (long)v.size(), n, dup);
    free(p);
    return r;
}

int main() {
    // the plane formula equals the definition on all 64 code triples, one triple a bit; exactly 16 are errors
    {
        uint64_t A[3] = {0, 0, 0}, B[3] = {0, 0, 0}, C[3] = {0, 0, 0}, want = 0;
        int bit = 0, errors = 0;
        for (int c = 0; c < 4; c++)
            for (int f = 0; f < 4; f++)
                for (int m = 0; m < 4; m++, bit++) {
                    const int code[3] = {c, f, m};
                    for (int k = 0; k < 3; k++) {
                        if (code[k] == 0) A[k] |= 1ull << bit;
                        if (code[k] == 2) B[k] |= 1ull << bit;
                        if (code[k] != 3) C[k] |= 1ull << bit;
                    }
                    if (error_by_alleles(c, f, m)) { want |= 1ull << bit; errors++; }
                }
        CHECK(bit == 64 && errors == 16);
        CHECK(mendel_error_word(A[0], B[0], C[0], A[1], B[1], A[2], B[2]) == want);
        const MendelXUV t = mendel_xuv(A[0], B[0], C[0], A[1], B[1]);
        CHECK((t.x | (t.u & B[2]) | (t.v & A[2])) == want);
        CHECK(t.x == ((A[0] & B[1]) | (B[0] & A[1])));
        // an unknown mother (zero words) leaves the child-father opposite homozygotes; both unknown: nothing
        CHECK(mendel_error_word(A[0], B[0], C[0], A[1], B[1], 0, 0) == t.x);
        CHECK(mendel_error_word(A[0], B[0], C[0], 0, 0, 0, 0) == 0);
        // a child that is called nowhere has no error
        CHECK(mendel_error_word(0, 0, 0, A[1], B[1], A[2], B[2]) == 0);
        // the image route: C is the word mask, and a zero (A, B) bit inside it is a het
        CHECK(mendel_error_word(0, 0, ~0ull, ~0ull, 0, ~0ull, 0) == ~0ull);                  // het children of two hom A1 parents
        CHECK(mendel_error_word(0, 0, mendel_word_mask(1, 70), ~0ull, 0, ~0ull, 0) == 0x3full);   // bits past the last marker are no hets
    }
    CHECK(mendel_word_mask(0, 64) == ~0ull && mendel_word_mask(0, 65) == ~0ull && mendel_word_mask(1, 65) == 1ull);
    CHECK(mendel_word_mask(0, 1) == 1ull && mendel_word_mask(0, 63) == ~0ull >> 1 && mendel_word_mask(1, 64) == 0 && mendel_word_mask(2, 65) == 0);
    CHECK(mendel_word_mask(33554431L, 0x7fffffffL) == ~0ull >> 1);

    // the trio rule
    CHECK(mendel_arg_error(1000, 1) == nullptr && mendel_arg_error(0x7fffffffL, MENDEL_MAX_TRIOS) == nullptr);
    CHECK(says(mendel_arg_error(1L << 31, 1), "2^31") && says(mendel_arg_error(10, 0), "number of trios") && says(mendel_arg_error(10, -1), "number of trios"));
    CHECK(says(mendel_arg_error(10, MENDEL_MAX_TRIOS + 1), "number of trios"));
    CHECK(trios_check({2, 0, 1, 2, 0, 1, 3, -1, 1, 3, 0, -1, 4, -1, -1, 0, 2, 3}, 5) == -1);   // repeats, unknowns, a child that is a parent
    CHECK(trios_check({2, 0, 1, 2, 2, 1}, 5) == 1 && trios_check({2, 0, 2}, 5) == 0 && trios_check({2, 1, 1}, 5) == 0);
    CHECK(trios_check({-1, 0, 1}, 5) == 0 && trios_check({5, 0, 1}, 5) == 0 && trios_check({2, 5, 1}, 5) == 0 && trios_check({2, 0, 5}, 5) == 0);
    CHECK(trios_check({2, -2, 1}, 5) == 0 && trios_check({2, 0, -2}, 5) == 0 && trios_check({0, -1, -1, 4, 3, 4}, 5) == 1);
    CHECK(trios_check({}, 5) == -1);

    // the assignment rule
    CHECK(parentage_arg_error(1000, 1, 1, 0, 0, 0) == nullptr && parentage_arg_error(1000, 1, 0, 1, 1, 1) == nullptr);
    CHECK(says(parentage_arg_error(1L << 31, 1, 1, 1, 1, 0), "2^31 markers"));
    CHECK(says(parentage_arg_error(10, 0, 1, 1, 1, 0), "offspring") && says(parentage_arg_error(10, MENDEL_MAX_TRIOS + 1, 1, 1, 1, 0), "offspring"));
    CHECK(says(parentage_arg_error(10, 1, 0, 0, 1, 0), "both candidate lists are empty"));
    CHECK(says(parentage_arg_error(10, 1, -1, 1, 1, 0), "negative length") && says(parentage_arg_error(10, 1, 1, -1, 1, 0), "negative length"));
    CHECK(parentage_arg_error(10, 1, 46340, 46340, 1, 0) == nullptr && parentage_arg_error(10, 1, 0x7fffffffL, 0, 1, 0) == nullptr);
    CHECK(says(parentage_arg_error(10, 1, 65536, 32768, 1, 0), "below 2^31") && says(parentage_arg_error(10, 1, 1L << 31, 0, 1, 0), "below 2^31"));
    CHECK(says(parentage_arg_error(10, 1, 0x7fffffffL, 0x7fffffffL, 1, 0), "below 2^31"));
    CHECK(says(parentage_arg_error(10, 1, 1, 1, -1, 0), "min_overlap") && says(parentage_arg_error(10, 1, 1, 1, 1L << 31, 0), "min_overlap"));
    CHECK(says(parentage_arg_error(10, 1, 1, 1, 1, 2), "allow_self") && says(parentage_arg_error(10, 1, 1, 1, 1, -1), "allow_self"));
    {
        bool dup = true;
        CHECK(list_check({}, 5, &dup) == -1 && !dup);
        CHECK(list_check({4, 0, 2}, 5, &dup) == -1 && !dup);
        CHECK(list_check({4, 0, 5}, 5, &dup) == 2 && !dup && list_check({-1, 0}, 5, &dup) == 0 && !dup);
        CHECK(list_check({4, 0, 2, 0}, 5, &dup) == 3 && dup);
        CHECK(list_check({3, 3}, 5, &dup) == 1 && dup && list_check({1, 2, 1, 2}, 5, &dup) == 2 && dup);
    }
    CHECK(parentage_ordinal(0, 0, 0) == 0 && parentage_ordinal(7, 0, 0) == 7 && parentage_ordinal(0, 7, 9) == 7 && parentage_ordinal(3, 2, 5) == 17);
    CHECK(parentage_ordinal(46339, 46339, 46340) == 46340L * 46340L - 1 && parentage_ordinal(46339, 46339, 46340) < (1L << 31));

    if (g_fail) {
        fprintf(stderr, "%d mendel host checks FAILED\n", g_fail);
        return 1;
    }
    printf("mendel host checks passed\n");
    return 0;
}
