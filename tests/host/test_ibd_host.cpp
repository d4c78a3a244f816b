// CPU test binary for the HIP-free pieces of eagle_ibd / eagle_bed_ibd (csrc/eagle_host.h: ibd_arg_error, ibd_pair_count,
// ibd_pair_ordinal, ibd_pairs_check, ibd_offsets, ibd_cut_plane), built by tests/test_ibd_abi.py with -fsanitize=address,undefined.
// Exit code 0 = every check passed.
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

// the defaults with field k replaced by v
static const char* rule(int k, int64_t v, long n = 10, long markers = 1000, bool has_pairs = false, long npairs = 0, long seg_cap = 0,
                        bool has_seg = false) {
    int64_t p[5] = {1, 200, 0, 0, 100};
    if (k >= 0) p[k] = v;
    return ibd_arg_error(p, n, markers, has_pairs, npairs, seg_cap, has_seg);
}

// the list lives in a heap block of exactly 2 * npairs entries, so that a read past it is an ASan report
static long pairs_check(const std::vector<int32_t>& flat, long n) {
    int32_t* p = (int32_t*)malloc(sizeof(int32_t) * (flat.size() ? flat.size() : 1));
    for (size_t i = 0; i < flat.size(); i++) p[i] = flat[i];
    const long r = ibd_pairs_check(p, (long)flat.size() / 2, n);
    free(p);
    return r;
}

static std::vector<uint64_t> cuts(const std::vector<int32_t>& chrom, const std::vector<int64_t>& pos, long max_gap, long markers) {
    int32_t* c = chrom.empty() ? nullptr : (int32_t*)malloc(sizeof(int32_t) * chrom.size());
    int64_t* p = pos.empty() ? nullptr : (int64_t*)malloc(sizeof(int64_t) * pos.size());
    for (size_t i = 0; i < chrom.size(); i++) c[i] = chrom[i];
    for (size_t i = 0; i < pos.size(); i++) p[i] = pos[i];
    std::vector<uint64_t> out;
    ibd_cut_plane(c, p, max_gap, markers, out);
    free(c);
    free(p);
    return out;
}

int main() {
    CHECK(rule(-1, 0) == nullptr);
    CHECK(says(rule(0, 0), "mode") && says(rule(0, 3), "mode") && says(rule(0, -1), "mode") && rule(0, 1) == nullptr && rule(0, 2) == nullptr);
    CHECK(says(rule(1, 0), "min_snp") && rule(1, 1) == nullptr);
    CHECK(says(rule(2, -1), "min_len") && rule(2, 0) == nullptr && rule(2, 0x7fffffffffffffffL) == nullptr);
    CHECK(says(rule(3, -1), "max_gap") && rule(3, 0) == nullptr);
    CHECK(says(rule(4, -1), "merge_min") && rule(4, 0) == nullptr && rule(4, 1) == nullptr);
    CHECK(says(rule(-1, 0, 10, 1L << 31), "2^31") && rule(-1, 0, 10, (1L << 31) - 1) == nullptr);
    // all pairs: 2 <= n and n (n - 1) / 2 <= 2^27
    CHECK(says(rule(-1, 0, 1), "two individuals") && rule(-1, 0, 2) == nullptr);
    CHECK(rule(-1, 0, 16384) == nullptr && says(rule(-1, 0, 16385), "2^27") && says(rule(-1, 0, 0x3fffffffL), "2^27"));
    // a list: 1 <= P <= 2^27, whatever n is
    CHECK(says(rule(-1, 0, 10, 1000, true, 0), "number of pairs") && says(rule(-1, 0, 10, 1000, true, -4), "number of pairs"));
    CHECK(rule(-1, 0, 10, 1000, true, 1) == nullptr && rule(-1, 0, 0x3fffffffL, 1000, true, IBD_MAX_PAIRS) == nullptr);
    CHECK(says(rule(-1, 0, 10, 1000, true, IBD_MAX_PAIRS + 1), "number of pairs"));
    CHECK(says(rule(-1, 0, 10, 1000, false, 0, -1, true), "seg_cap"));
    CHECK(says(rule(-1, 0, 10, 1000, false, 0, 1, false), "NULL") && rule(-1, 0, 10, 1000, false, 0, 1, true) == nullptr);

    // pair counts and ordinals: row-major upper triangle
    CHECK(ibd_pair_count(5, false, 77) == 10 && ibd_pair_count(5, true, 77) == 77 && ibd_pair_count(16384, false, 0) == 134209536L);
    {
        long k = 0;
        bool ok = true;
        for (long i = 0; i < 7; i++)
            for (long j = i + 1; j < 7; j++) ok = ok && ibd_pair_ordinal(7, i, j) == k++;
        CHECK(ok && k == 21);
        CHECK(ibd_pair_ordinal(16384, 16382, 16383) == 134209535L);
    }

    // the list: 0 <= i < j < n, duplicates and any order pass; the first offender is named
    CHECK(pairs_check({0, 1, 0, 1, 3, 4, 0, 4}, 5) == -1);
    CHECK(pairs_check({0, 1, 1, 1}, 5) == 1 && pairs_check({0, 1, 2, 1}, 5) == 1 && pairs_check({-1, 1}, 5) == 0);
    CHECK(pairs_check({0, 1, 0, 2, 3, 5}, 5) == 2 && pairs_check({0, 5, 1, 1}, 5) == 0);
    CHECK(pairs_check({}, 5) == -1);

    // exclusive scan of column 0 of the pair table
    {
        int64_t* tab = (int64_t*)malloc(sizeof(int64_t) * 4 * 5);
        int64_t* offs = (int64_t*)malloc(sizeof(int64_t) * 5);
        const int64_t v[5] = {2, 0, 3, 0, 1};
        for (int k = 0; k < 5; k++) { tab[4 * k] = v[k]; tab[4 * k + 1] = 1000; tab[4 * k + 2] = -7; tab[4 * k + 3] = 99; }
        CHECK(ibd_offsets(tab, 5, offs) == 6);
        CHECK(offs[0] == 0 && offs[1] == 2 && offs[2] == 2 && offs[3] == 5 && offs[4] == 5);
        CHECK(ibd_offsets(tab, 0, offs) == 0);
        free(tab);
        free(offs);
    }

    // the cut plane: marker 0, every change of chrom, every gap above max_gap (when it is on); tail bits stay zero
    CHECK((cuts({}, {}, 0, 5) == std::vector<uint64_t>{1ull}));
    CHECK((cuts({3, 3, 1, 1, 3}, {}, 0, 5) == std::vector<uint64_t>{1ull | 1ull << 2 | 1ull << 4}));
    CHECK((cuts({}, {0, 10, 21, 31, 31}, 10, 5) == std::vector<uint64_t>{1ull | 1ull << 2}));
    CHECK((cuts({}, {0, 10, 21, 31, 31}, 0, 5) == std::vector<uint64_t>{1ull}));
    CHECK((cuts({1, 1, 2, 2, 2}, {50, 60, 0, 5, 100}, 20, 5) == std::vector<uint64_t>{1ull | 1ull << 2 | 1ull << 4}));
    {
        std::vector<int32_t> chrom(130, 1);
        chrom[63] = 2;                                   // blocks [0, 63), [63, 64), [64, 130)
        std::vector<int64_t> pos(130);
        for (int m = 0; m < 130; m++) pos[m] = m;
        pos[128] = 500; pos[129] = 501;
        const std::vector<uint64_t> c = cuts(chrom, pos, 100, 130);
        CHECK(c.size() == 3 && c[0] == (1ull | 1ull << 63) && c[1] == 1ull && c[2] == 1ull);
        CHECK(cuts({}, {}, 0, 64).size() == 1 && cuts({}, {}, 0, 65).size() == 2 && cuts({}, {}, 0, 65)[1] == 0);
    }
    if (g_fail) {
        fprintf(stderr, "%d ibd host checks FAILED\n", g_fail);
        return 1;
    }
    printf("ibd host checks passed\n");
    return 0;
}
