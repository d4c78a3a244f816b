// CPU test binary for the row windows of a pass over an ingested image (csrc/eagle_host.h: RowWindows, row_windows_disjoint /
// row_windows_overlapped / row_windows_cores), built by tests/test_windows_host.py with -fsanitize=address,undefined.  The expected
// lists are written out by hand from the three window loops the entry points used to carry; the sweeps compare with those loops
// themselves, kept here verbatim.  Exit code 0 = every check passed.
#include <stdio.h>
#include <stdlib.h>

#include "../../eagleeverything_amd/csrc/eagle_host.h"

static int g_fail = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } \
    } while (0)

struct Win { long lo, hi, c0, c1; };   // rows held [lo, hi), rows owned [c0, c1)
typedef std::vector<Win> Wins;

static Wins run(RowWindows ws) {
    Wins out;
    RowWindow w;
    while (ws.next(w)) {
        out.push_back({w.lo, w.lo + w.nr, w.c0, w.c1});
        if (out.size() > 100000) { CHECK(!"the windows do not end"); break; }
    }
    CHECK(!ws.next(w));   // and stays at the end
    return out;
}

static bool same(const Wins& a, const Wins& b) {
    if (a.size() != b.size()) return false;
    for (size_t k = 0; k < a.size(); k++)
        if (a[k].lo != b[k].lo || a[k].hi != b[k].hi || a[k].c0 != b[k].c0 || a[k].c1 != b[k].c1) return false;
    return true;
}

// what every sequence owes: the owned ranges tile [0, rows) exactly once and in order; a window holds its owned rows with `back` rows
// before and `fwd` rows behind them, clipped to the file, and nothing else; no window holds more than cap rows
static void check_invariants(const Wins& w, long rows, long cap, long back, long fwd) {
    long next = 0;
    for (const Win& x : w) {
        CHECK(x.c0 == next && x.c1 > x.c0);
        CHECK(x.lo == std::max(0L, x.c0 - back));
        CHECK(x.hi == std::min(rows, x.c1 + fwd));
        CHECK(x.lo <= x.c0 && x.c1 <= x.hi && x.hi <= rows);
        CHECK(x.hi - x.lo >= 1 && x.hi - x.lo <= cap);
        next = x.c1;
    }
    CHECK(next == rows);
}

// the three loops as the entry points wrote them
static Wins loop_disjoint(long L, long w) {
    Wins out;
    for (long r0 = 0; r0 < L; r0 += w) {
        const long nr = std::min(w, L - r0);
        out.push_back({r0, r0 + nr, r0, r0 + nr});
    }
    return out;
}
static Wins loop_overlapped(long L, long w, long window) {   // a window's final rows: all but its last `window`, the last window's all
    Wins out;
    const long step = w - window;
    for (long r0 = 0;; r0 += step) {
        const long nr = std::min(w, L - r0);
        const bool last = r0 + nr >= L;
        out.push_back({r0, r0 + nr, r0, last ? L : r0 + step});
        if (last) break;
    }
    return out;
}
static Wins loop_cores(long L, long held_max, long window) {
    Wins out;
    const long core = held_max >= L ? L : held_max - 2 * window;
    for (long c0 = 0; c0 < L; c0 += core) {
        const long c1 = std::min(L, c0 + core), lo = std::max(0L, c0 - window), hi = std::min(L, c1 + window);
        out.push_back({lo, hi, c0, c1});
    }
    return out;
}

static void test_by_hand() {
    // disjoint, 1531 rows in windows of 256: six, the last of 251 rows
    const Wins d = run(row_windows_disjoint(1531, 256));
    CHECK(same(d, {{0, 256, 0, 256}, {256, 512, 256, 512}, {512, 768, 512, 768}, {768, 1024, 768, 1024}, {1024, 1280, 1024, 1280},
                   {1280, 1531, 1280, 1531}}));
    CHECK(d.size() == 6 && d[5].hi - d[5].lo == 251);
    check_invariants(d, 1531, 256, 0, 0);
    // overlapped, w = 512 every 256 rows: starts 0 .. 1024, the last holds 507 rows and reaches the end: no sixth window
    const Wins o = run(row_windows_overlapped(1531, 512, 256));
    CHECK(same(o, {{0, 512, 0, 256}, {256, 768, 256, 512}, {512, 1024, 512, 768}, {768, 1280, 768, 1024}, {1024, 1531, 1024, 1531}}));
    CHECK(o.size() == 5 && o[4].hi - o[4].lo == 507);
    check_invariants(o, 1531, 512, 0, 256);
    // cores, 1024 rows held at most, halo 256: cores of 512
    const Wins c = run(row_windows_cores(1531, 1024, 256));
    CHECK(same(c, {{0, 768, 0, 512}, {256, 1280, 512, 1024}, {768, 1531, 1024, 1531}}));
    check_invariants(c, 1531, 1024, 256, 256);
    // the ROH shape: 256 rows held, halo 63, cores of 130 rows: twelve of them
    const Wins r = run(row_windows_cores(1531, 256, 63));
    CHECK(r.size() == 12);
    CHECK(r[0].lo == 0 && r[0].hi == 193 && r[0].c0 == 0 && r[0].c1 == 130);
    CHECK(r[1].lo == 67 && r[1].hi == 323 && r[1].c0 == 130 && r[1].c1 == 260);
    CHECK(r[11].lo == 1367 && r[11].hi == 1531 && r[11].c0 == 1430 && r[11].c1 == 1531);
    check_invariants(r, 1531, 256, 63, 63);
}

static void test_edges() {
    const Wins whole = {{0, 300, 0, 300}};
    // rows <= capacity: one window that owns everything, with any halo
    CHECK(same(run(row_windows_disjoint(300, 300)), whole));
    CHECK(same(run(row_windows_disjoint(300, 1024)), whole));
    CHECK(same(run(row_windows_overlapped(300, 512, 256)), whole));
    CHECK(same(run(row_windows_overlapped(300, 300, 1)), whole));
    CHECK(same(run(row_windows_overlapped(300, 300, 256)), whole));
    CHECK(same(run(row_windows_cores(300, 300, 256)), whole));     // twice the halo is more than the file
    CHECK(same(run(row_windows_cores(300, 1024, 63)), whole));
    CHECK(same(run(row_windows_cores(300, 300, 0)), whole));
    CHECK(same(run(row_windows_disjoint(1, 256)), {{0, 1, 0, 1}}));
    CHECK(same(run(row_windows_cores(1, 1, 63)), {{0, 1, 0, 1}}));
    // rows = capacity + 1 with a halo
    CHECK(same(run(row_windows_disjoint(257, 256)), {{0, 256, 0, 256}, {256, 257, 256, 257}}));
    CHECK(same(run(row_windows_overlapped(513, 512, 256)), {{0, 512, 0, 256}, {256, 513, 256, 513}}));
    CHECK(same(run(row_windows_cores(1025, 1024, 256)), {{0, 768, 0, 512}, {256, 1025, 512, 1024}, {768, 1025, 1024, 1025}}));
    CHECK(same(run(row_windows_cores(257, 256, 63)), {{0, 193, 0, 130}, {67, 257, 130, 257}}));
    // halo 0: all three are the disjoint windows
    const Wins z = {{0, 512, 0, 512}, {512, 1024, 512, 1024}, {1024, 1531, 1024, 1531}};
    CHECK(same(run(row_windows_disjoint(1531, 512)), z));
    CHECK(same(run(row_windows_overlapped(1531, 512, 0)), z));
    CHECK(same(run(row_windows_cores(1531, 512, 0)), z));
    // a file that is a multiple of the window: no empty window behind the last
    CHECK(run(row_windows_disjoint(1024, 256)).size() == 4);
    CHECK(same(run(row_windows_overlapped(768, 512, 256)), {{0, 512, 0, 256}, {256, 768, 256, 768}}));
    CHECK(same(run(row_windows_cores(1024, 768, 128)), {{0, 640, 0, 512}, {384, 1024, 512, 1024}}));
}

static void test_sweep() {
    const long rows[] = {1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1531, 4096, 5000};
    const long caps[] = {256, 512, 768, 1024, 1280, 4096};
    const long halos[] = {0, 1, 63, 100, 255, 256};
    for (long L : rows)
        for (long cap : caps) {
            const Wins d = run(row_windows_disjoint(L, cap));
            CHECK(same(d, loop_disjoint(L, cap)));
            check_invariants(d, L, cap, 0, 0);
            const Wins dc = run(row_windows_disjoint(L, std::min(L, cap)));   // the sites that clip their window to the file
            CHECK(same(dc, loop_disjoint(L, std::min(L, cap))));
            check_invariants(dc, L, std::min(L, cap), 0, 0);
            for (long h : halos) {
                if (cap >= 512) {   // the overlapped pass: at least 512 rows, at most 256 of overlap
                    const Wins o = run(row_windows_overlapped(L, cap, h));
                    CHECK(same(o, loop_overlapped(L, cap, h)));
                    check_invariants(o, L, cap, 0, h);
                }
                const long held_max = std::min(L, cap);   // both core passes clip to the file
                if (held_max < L && held_max <= 2 * h) continue;   // below the callers' floors (1,024 rows for 256, 256 for 63)
                const Wins c = run(row_windows_cores(L, held_max, h));
                CHECK(same(c, loop_cores(L, held_max, h)));
                check_invariants(c, L, held_max, h, h);
            }
        }
}

int main(int argc, char** argv) {
    (void)argc; (void)argv;
    test_by_hand();
    test_edges();
    test_sweep();
    if (g_fail) { fprintf(stderr, "%d window host checks failed\n", g_fail); return 1; }
    printf("window host checks passed\n");
    return 0;
}
