// CPU test binary for the HIP-free pieces of the PLINK .bed ingestion (csrc/eagle_host.h: bed_check_header, bed_row_bytes,
// bed_expected_size, sidecar_row_bytes, bed_window_markers / bed_window / bed_window_count), built by tests/test_bed_host.py with
// -fsanitize=address,undefined.  Exit code 0 = every check passed.
#include <stdio.h>
#include <stdlib.h>

#include "../../eagleeverything_amd/csrc/eagle_host.h"

static int g_fail = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } \
    } while (0)

static void test_header() {
    // every header lives in a heap block of exactly its length, so that a read past `got` is an ASan report
    auto verdict = [](std::vector<unsigned char> h) {
        unsigned char* p = (unsigned char*)malloc(h.size() ? h.size() : 1);
        for (size_t i = 0; i < h.size(); i++) p[i] = h[i];
        const int v = bed_check_header(p, (long)h.size());
        free(p);
        return v;
    };
    CHECK(verdict({0x6c, 0x1b, 0x01}) == BED_HEADER_OK);
    CHECK(verdict({0x6c, 0x1b, 0x00}) == BED_HEADER_INDIVIDUAL_MAJOR);
    CHECK(verdict({0x6c, 0x1b, 0x02}) == BED_HEADER_MODE);
    CHECK(verdict({0x1b, 0x6c, 0x01}) == BED_HEADER_MAGIC);
    CHECK(verdict({0x6c, 0x1c, 0x01}) == BED_HEADER_MAGIC);
    CHECK(verdict({'0', ' ', '1'}) == BED_HEADER_MAGIC);      // a text table handed over as a bed file
    CHECK(verdict({}) == BED_HEADER_SHORT);
    CHECK(verdict({0x6c}) == BED_HEADER_SHORT);
    CHECK(verdict({0x6c, 0x1b}) == BED_HEADER_SHORT);
}

static void test_sizes() {
    const long ns[6] = {1, 3, 4, 5, 150, 10000};
    const long rb[6] = {1, 1, 1, 2, 38, 2500};          // ceil(n / 4)
    const long rb16[6] = {16, 16, 16, 16, 48, 2512};    // ... padded to 16: the sidecar's stride
    for (int i = 0; i < 6; i++) {
        CHECK(bed_row_bytes(ns[i]) == rb[i]);
        CHECK(sidecar_row_bytes(ns[i]) == rb16[i]);
        CHECK(sidecar_row_bytes(ns[i]) % 16 == 0 && sidecar_row_bytes(ns[i]) >= bed_row_bytes(ns[i]) && sidecar_row_bytes(ns[i]) < bed_row_bytes(ns[i]) + 16);
        CHECK(bed_expected_size(ns[i], 1) == 3 + rb[i]);
        CHECK(bed_expected_size(ns[i], 100) == 3 + 100 * rb[i]);
    }
    CHECK(bed_expected_size(150, 100) == 3803);
    CHECK(bed_expected_size(10000, 1000000) == 2500000003LL);
    CHECK(bed_expected_size(50000, 5000000) == 62500000003LL);   // past 32 bits
}

static long pad256(long x) { return (x + 255) / 256 * 256; }

// the windows of (n, L) under a text capacity and a budget: they tile [0, L) with `real` and [0, L_pad) with `padded`
static void check_windows(long n, long L, size_t text_cap, size_t budget, long expect_w) {
    const long n_pad = pad256(n), L_pad = pad256(L);
    const long w = bed_window_markers(n, n_pad, L_pad, text_cap, budget);
    CHECK(w == expect_w);
    CHECK(w % 256 == 0 && w >= 256 && w <= L_pad);
    const long nwin = bed_window_count(w, L);
    long next = 0, next_pad = 0;
    for (long k = 0; k < nwin; k++) {
        const BedWindow bw = bed_window(k, w, L, L_pad);
        CHECK(bw.c0 == next && bw.c0 == next_pad);
        CHECK(bw.real >= 1 && bw.real <= bw.padded && bw.padded <= w && bw.padded % 256 == 0);
        CHECK(k == nwin - 1 || (bw.real == w && bw.padded == w));
        next += bw.real;
        next_pad += bw.padded;
    }
    CHECK(next == L && next_pad == L_pad);
}

static void test_windows() {
    const size_t none = (size_t)-1, cap = (size_t)67108864;
    check_windows(150, 100, cap, none, 256);           // one window: the whole padded panel
    check_windows(150, 4998, cap, none, 5120);
    check_windows(10000, 1000000, cap, none, 6656);    // 64 MiB / 10,001 = 6,710 -> 6,656; L is not a multiple of it (151 windows)
    CHECK(bed_window_count(6656, 1000000) == 151);
    check_windows(2049, 5000, cap, (size_t)500000, 256);   // a budget below one 256-marker tile still gives 256
    check_windows(301, 1999, cap, (size_t)500000, 768);    // 500,000 / 512 = 976 -> 768; 1,999 = 2 * 768 + 463
    check_windows(300, 1024, cap, (size_t)300000, 512);    // L a multiple of the window
    check_windows(50000, 5000000, cap, none, 1280);
    check_windows(70000000, 300, cap, none, 256);          // a line longer than the text capacity: the minimum window
}

int main(int argc, char** argv) {
    (void)argc; (void)argv;
    test_header();
    test_sizes();
    test_windows();
    if (g_fail) { fprintf(stderr, "%d bed host checks failed\n", g_fail); return 1; }
    printf("bed host checks passed\n");
    return 0;
}
