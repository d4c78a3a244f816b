// CPU test binary for the HIP-free argument rule of eagle_ld_stats / eagle_bed_ld_stats (csrc/eagle_host.h: ld_stats_arg_error), built by
// tests/test_ld_stats_abi.py with -fsanitize=address,undefined.  Exit code 0 = every check passed.
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

// the edges live in a heap block of exactly nbins + 1 words, so that a read past them is an ASan report
static const char* with_edges(std::vector<int64_t> e, long nbins, bool outs = true, long markers = 1000, long window = 50) {
    int64_t* p = (int64_t*)malloc(sizeof(int64_t) * (e.size() ? e.size() : 1));
    for (size_t i = 0; i < e.size(); i++) p[i] = e[i];
    const char* r = ld_stats_arg_error(markers, window, true, 0, p, nbins, outs);
    free(p);
    return r;
}

int main() {
    CHECK(ld_stats_arg_error(1000, 50, false, 0, nullptr, 0, false) == nullptr);
    CHECK(says(ld_stats_arg_error(1000, 0, false, 0, nullptr, 0, false), "window"));
    CHECK(says(ld_stats_arg_error(1000, 257, false, 0, nullptr, 0, false), "window"));
    CHECK(ld_stats_arg_error(1000, 1, false, 0, nullptr, 0, false) == nullptr && ld_stats_arg_error(1000, 256, false, 0, nullptr, 0, false) == nullptr);
    CHECK(says(ld_stats_arg_error(1L << 31, 1, false, 0, nullptr, 0, false), "2^31"));
    CHECK(says(ld_stats_arg_error(0x7fffffffffffffffL, 256, false, 0, nullptr, 0, false), "2^31"));      // decided before the product is formed
    CHECK(ld_stats_arg_error((1L << 31) - 1, 4, false, 0, nullptr, 0, false) == nullptr);
    CHECK(says(ld_stats_arg_error((1L << 31) - 1, 5, false, 0, nullptr, 0, false), "2^33"));
    CHECK(ld_stats_arg_error(1L << 25, 256, false, 0, nullptr, 0, false) == nullptr);                      // the limit itself
    CHECK(says(ld_stats_arg_error((1L << 25) + 1, 256, false, 0, nullptr, 0, false), "2^33"));
    CHECK(says(ld_stats_arg_error(1000, 50, false, 1, nullptr, 0, false), "max_dist needs pos"));
    CHECK(ld_stats_arg_error(1000, 50, true, 1, nullptr, 0, false) == nullptr);
    CHECK(ld_stats_arg_error(1000, 50, false, 0, nullptr, 0, false) == nullptr && ld_stats_arg_error(1000, 50, false, -5, nullptr, 0, false) == nullptr);
    CHECK(says(ld_stats_arg_error(1000, 50, false, 0, nullptr, -1, false), "nbins"));
    CHECK(says(ld_stats_arg_error(1000, 50, false, 0, nullptr, 513, false), "nbins"));
    CHECK(ld_stats_arg_error(1000, 50, false, 0, nullptr, 512, false) == nullptr);                         // no edges: no decay, nothing read
    CHECK(with_edges({1, 2}, 1) == nullptr);
    CHECK(with_edges({-7, 0, 9000000000L}, 2) == nullptr);
    CHECK(with_edges({1, 2, 3}, 0, false) == nullptr);                                                     // nbins == 0: no decay
    CHECK(says(with_edges({1, 2}, 1, false), "NULL"));
    CHECK(says(with_edges({1, 1}, 1), "strictly increasing"));
    CHECK(says(with_edges({2, 1}, 1), "strictly increasing"));
    CHECK(says(with_edges({1, 2, 3, 3}, 3), "strictly increasing"));                                       // the last pair is looked at
    CHECK(with_edges({1, 2, 3, 3}, 2) == nullptr);                                                         // ... and nothing beyond nbins + 1
    std::vector<int64_t> full(513);
    for (size_t i = 0; i < full.size(); i++) full[i] = (int64_t)i * 45;
    CHECK(with_edges(full, 512) == nullptr);
    full[512] = full[511];
    CHECK(says(with_edges(full, 512), "strictly increasing"));
    if (g_fail) {
        fprintf(stderr, "%d ld stats host checks FAILED\n", g_fail);
        return 1;
    }
    printf("ld stats host checks passed\n");
    return 0;
}
