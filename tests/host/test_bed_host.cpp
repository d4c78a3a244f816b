// CPU test binary for the HIP-free pieces of the PLINK .bed ingestion (csrc/eagle_host.h: bed_check_header, bed_row_bytes,
// bed_expected_size, sidecar_row_bytes, bed_window_markers / bed_window / bed_window_count, bed_stage_rows, bed_panel_file_row /
// bed_panel_window_end), built by tests/test_bed_host.py with
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

// the staging rule of include/eagle_hip.h section 1b'''iv: S = max(1, floor(min(64 MiB, max_memory_in_Gbytes * 1e9 / 4) / rb))
static void test_stage_rows() {
    CHECK(bed_stage_rows(33, 4.0 * 100 * 33 / 1e9) == 100);     // the tests' arithmetic: a quarter of the budget is 100 rows of n = 129
    CHECK(bed_stage_rows(33, 8.0) == 2033601);                  // the 64 MiB cap: 67,108,864 / 33
    CHECK(bed_stage_rows(33, 0.0) == 2033601);                  // no budget given: the cap alone
    CHECK(bed_stage_rows(2500, 8.0) == 26843);
    CHECK(bed_stage_rows(65, 4.0 * 1 * 65 / 1e9) == 1);         // one row
    CHECK(bed_stage_rows(33, 1e-9) == 1);                       // a quarter of a byte: the floor
    CHECK(bed_stage_rows(100000000, 8.0) == 1);                 // a row longer than the cap: the floor
}

// the windows a call walks, next_of(hi) = hi - back: their number, the widest span of file rows, the most panel markers
struct PanelWalk { long windows, span_max, p_max; };
static PanelWalk walk_panel(long need, long back, long wmax, long S, const std::vector<long>& fidx, long linc) {
    PanelWalk w = {0, 0, 0};
    for (long lo = 0; lo < linc;) {
        const long hi = bed_panel_window_end(lo, need, wmax, S, linc, fidx);
        CHECK(hi > lo && hi <= linc);
        if (hi <= lo) break;
        w.windows++;
        w.span_max = std::max(w.span_max, bed_panel_file_row(fidx, hi - 1) - bed_panel_file_row(fidx, lo) + 1);
        w.p_max = std::max(w.p_max, hi - lo);
        lo = hi >= linc ? linc : hi - back;
    }
    return w;
}

static void test_panel_windows() {
    const std::vector<long> all;   // the identity
    // a hole longer than S: file rows [150, 450) of 700 excluded, S = 100, eagle_bed_ld_window at window = 33 (need 34, back 33)
    std::vector<long> hole;
    for (long m = 0; m < 700; m++) if (m < 150 || m >= 450) hole.push_back(m);
    CHECK(hole.size() == 400 && bed_panel_file_row(hole, 149) == 149 && bed_panel_file_row(hole, 150) == 450 && bed_panel_file_row(all, 150) == 150);
    CHECK(bed_panel_window_end(0, 34, 1024, 100, 400, hole) == 100);     // file rows 0 .. 99
    CHECK(bed_panel_window_end(67, 34, 1024, 100, 400, hole) == 150);    // rows 67 .. 166 hold the markers up to the hole
    CHECK(bed_panel_window_end(117, 34, 1024, 100, 400, hole) == 151);   // 33 markers before the hole: need takes the window across it
    CHECK(bed_panel_window_end(149, 34, 1024, 100, 400, hole) == 183);
    CHECK(bed_panel_window_end(150, 34, 1024, 100, 400, hole) == 250);   // file rows 450 .. 549
    CHECK(bed_panel_window_end(351, 34, 1024, 100, 400, hole) == 400);   // file rows 651 .. 699: the panel's end
    const PanelWalk wh = walk_panel(34, 33, 1024, 100, hole, 400);       // lo = 0, 67, 117 .. 149, 150, 217, 284, 351
    CHECK(wh.windows == 39 && wh.span_max == 334 && wh.p_max == 100);    // 334 = rows 117 .. 450: the staging buffer grows past S
    // need past the budget: S = 1 row, every window is the 34 markers the call needs, the next starts one marker on: L - 33 of them
    const PanelWalk wt = walk_panel(34, 33, 1024, 1, all, 700);
    CHECK(wt.windows == 700 - 33 && wt.span_max == 34 && wt.p_max == 34);
    CHECK(bed_panel_window_end(5, 34, 1024, 1, 700, all) == 39);
    // the last window is clipped to linc, by the budget's window and by need alike; wmax caps a window the budget would allow
    CHECK(bed_panel_window_end(134, 34, 1024, 100, 250, all) == 234);
    CHECK(bed_panel_window_end(201, 34, 1024, 100, 250, all) == 250);
    CHECK(bed_panel_window_end(240, 34, 1024, 1, 250, all) == 250);
    CHECK(bed_panel_window_end(0, 34, 50, 100, 250, all) == 50);
    CHECK(walk_panel(34, 33, 1024, 100, all, 250).windows == 4);         // lo = 0, 67, 134, 201
    CHECK(walk_panel(34, 33, 1024, 100, all, 20).windows == 1);          // a panel shorter than need
}

int main(int argc, char** argv) {
    (void)argc; (void)argv;
    test_header();
    test_sizes();
    test_windows();
    test_stage_rows();
    test_panel_windows();
    if (g_fail) { fprintf(stderr, "%d bed host checks failed\n", g_fail); return 1; }
    printf("bed host checks passed\n");
    return 0;
}
