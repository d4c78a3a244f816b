// CPU test binary for the HIP-free host pieces of libeaglehip.so (csrc/eagle_host.h), built by tests/test_host_sanitizers.py
// with -fsanitize=address,undefined and, for the Rendezvous cases, -fsanitize=thread.  Exit code 0 = every check passed.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <chrono>
#include <string>

#include "../../eagleeverything_amd/csrc/eagle_host.h"

static int g_fail = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } \
    } while (0)

// ---- Rendezvous --------------------------------------------------------------------------------------------------
// rounds of n workers; worker `bad` reports a failure at its arrival for round `bad_round` (and, like the library's workers,
// keeps arriving).  Returns per worker the verdict it saw per round.
static std::vector<std::vector<int>> run_rounds(int n, int rounds, int bad, int bad_round, bool bad_is_fast) {
    Rendezvous rv;
    rv.n = n;
    std::vector<std::vector<int>> seen((size_t)n, std::vector<int>((size_t)rounds, -1));
    std::vector<std::thread> th;
    for (int k = 0; k < n; k++)
        th.emplace_back([&, k] {
            for (int r = 0; r < rounds; r++) {
                // the slow peers dawdle AFTER waking up from a round, which is when the fast device of the advisor's scenario
                // has already failed and arrived for the next round
                if (bad_is_fast && k != bad) std::this_thread::sleep_for(std::chrono::milliseconds(2));
                const bool ok = !(k == bad && r >= bad_round);
                seen[(size_t)k][(size_t)r] = rv.arrive(ok, (double)(r * 100 + k), (long)(r + k)) ? 1 : 0;
                if (seen[(size_t)k][(size_t)r] == 1 && rv.vmax != (double)(r * 100 + n - 1)) g_fail++;  // the round's maximum, stable until the next arrival
                // ... and the round's SUM (round 4: the markers over the tight threshold, added up over the devices of a scan)
                if (seen[(size_t)k][(size_t)r] == 1 && rv.vsum != (long)n * r + (long)n * (n - 1) / 2) g_fail++;
            }
        });
    for (auto& t : th) t.join();
    return seen;
}

static void test_rendezvous() {
    // no failure: every round true
    for (auto& w : run_rounds(4, 50, -1, 0, false)) for (int v : w) CHECK(v == 1);
    // a device fails between round 2 and round 3 and is FAST (the sticky flag, read after the wake-up, made a slow peer
    // leave round 2 with `false`, skip its round-3 arrival and strand the failed device): every worker must see rounds 0..2 true
    // and rounds 3.. false, and nobody may hang (the join above returning is that check)
    for (int trial = 0; trial < 20; trial++) {
        auto seen = run_rounds(3, 6, 0, 3, true);
        for (auto& w : seen) {
            for (int r = 0; r < 3; r++) CHECK(w[(size_t)r] == 1);
            for (int r = 3; r < 6; r++) CHECK(w[(size_t)r] == 0);
        }
    }
    // the library's control flow: a worker that sees `false` returns early -- legal only if every worker sees the SAME verdict
    // for the same round (else the counts of arrivals diverge and someone waits for ever)
    for (int trial = 0; trial < 20; trial++) {
        Rendezvous rv;
        rv.n = 4;
        std::atomic<int> exits_at[8];
        for (auto& e : exits_at) e = 0;
        std::vector<std::thread> th;
        for (int k = 0; k < 4; k++)
            th.emplace_back([&, k] {
                for (int r = 0; r < 8; r++) {
                    if (k != 1) std::this_thread::sleep_for(std::chrono::microseconds(300 * (k + 1)));
                    const bool ok = !(k == 1 && r == 4);
                    if (!rv.arrive(ok)) { exits_at[r]++; return; }
                }
            });
        for (auto& t : th) t.join();
        for (int r = 0; r < 8; r++) CHECK(exits_at[r] == (r == 4 ? 4 : 0));
    }
    // NaN and -inf values do not disturb the maximum
    {
        Rendezvous rv;
        rv.n = 1;
        CHECK(rv.arrive(true, NAN) && rv.vmax == -HUGE_VAL);
        CHECK(rv.arrive(true, 3.0) && rv.vmax == 3.0);
        CHECK(rv.arrive(true) && rv.vmax == -HUGE_VAL && rv.vsum == 0);
        CHECK(rv.arrive(true, 1.0, 7) && rv.vsum == 7);
        CHECK(rv.arrive(true) && rv.vsum == 0);   // a round's sum does not leak into the next
    }
}

// ---- marker split, selected_loci, chunk rows, tail pieces ---------------------------------------------------------------
static void test_small_rules() {
    std::vector<long> e;
    for (long L : {1L, 255L, 256L, 257L, 1000L, 150001L, 1000000L})
        for (int nd : {1, 2, 3, 5, 8}) {
            split_markers(L, nd, e);
            CHECK((int)e.size() == nd + 1 && e[0] == 0 && e[(size_t)nd] == L);
            for (int k = 0; k < nd; k++) { CHECK(e[(size_t)k] <= e[(size_t)k + 1]); if (k) CHECK(e[(size_t)k] % 256 == 0 || e[(size_t)k] == L); }
        }
    std::vector<long> out;
    const double na = NAN;
    double s1[] = {na, 3, 4};
    CHECK(parse_selected_core(s1, 3, 10, out) == nullptr && out.empty());       // AM()'s c(NA, i1, i2): masking never fires
    double s2[] = {3, 4, 9};
    CHECK(parse_selected_core(s2, 3, 10, out) == nullptr && out.size() == 3 && out[2] == 9);
    double s3[] = {3, na};
    CHECK(parse_selected_core(s3, 2, 10, out) != nullptr);
    double s4[] = {10};
    CHECK(parse_selected_core(s4, 1, 10, out) != nullptr);
    double s5[] = {-1};
    CHECK(parse_selected_core(s5, 1, 10, out) != nullptr);
    CHECK(parse_selected_core(nullptr, 0, 10, out) == nullptr && out.empty());
    CHECK(stream_chunk_rows_core((size_t)-1, 50176, 1 << 30) == (long)(((size_t)8 << 30) / 2 / 50176) / 256 * 256);
    CHECK(stream_chunk_rows_core(1000, 50176, 100000) == 256);                 // never below one tile of rows
    CHECK(stream_chunk_rows_core((size_t)1 << 40, 256, 2048) == 2048);         // never above the file
    CHECK(stream_chunk_rows_core(616562688, 50176, 625152) == 6144);           // the C4 shard in >= 100 chunks
    for (int npair : {1, 2, 5, 20, 100})
        for (int tail = 0; tail < 32; tail++) {
            const int p = vara_tail_pieces(tail, npair);
            CHECK(p >= 1 && p <= std::max(1, std::min(npair, VARA_TAIL_PMAX)));
            for (int q = 1; tail && q <= std::min(npair, VARA_TAIL_PMAX); q++)
                CHECK(((tail * p + 31) >> 5) * q <= ((tail * q + 31) >> 5) * p);
        }
    CHECK(vara_tail_pieces(3, 20) == 10);
}

// ---- line index + tokeniser ----------------------------------------------------------------------------------------
static void test_text() {
    struct Case { std::string text; long nlines; };
    const Case cases[] = {{"", 0}, {"\n", 1}, {"a b\n", 1}, {"a b", 1}, {"a\n\nb\n", 3}, {"0 1 2\n2 1 0\n1 1", 3}, {std::string(100000, 'x') + "\n1 2\n", 2}};
    for (const Case& c : cases)
        for (int threads : {1, 2, 3, 7, 16}) {
            // exact-size heap copy: an over-read by a single byte is an ASan report
            char* buf = (char*)malloc(c.text.size() ? c.text.size() : 1);
            memcpy(buf, c.text.data(), c.text.size());
            LineIndex ix;
            index_lines_buf(buf, c.text.size(), threads, ix);
            CHECK(ix.nlines() == c.nlines);
            std::string rebuilt;
            for (long i = 0; i < ix.nlines(); i++) {
                CHECK(ix.begin(i) <= ix.end(i) && ix.end(i) <= c.text.size());
                rebuilt.append(buf + ix.begin(i), ix.end(i) - ix.begin(i));
                rebuilt.push_back('\n');
            }
            std::string want = c.text;
            if (!want.empty() && want.back() != '\n') want.push_back('\n');
            CHECK(rebuilt == want);
            free(buf);
        }
    // big random text, many threads: the per-thread pieces must concatenate to the sequential index
    std::string big;
    unsigned s = 12345;
    for (int i = 0; i < 400000; i++) { s = s * 1664525u + 1013904223u; big.push_back((s >> 24) % 11 == 0 ? '\n' : (char)('0' + (s >> 24) % 3)); }
    LineIndex a, b;
    index_lines_buf(big.data(), big.size(), 1, a);
    index_lines_buf(big.data(), big.size(), 13, b);
    CHECK(a.starts == b.starts && a.tail == b.tail);
    const char* line = " 0\t1  2\r\n";
    CHECK(count_tokens(line, line + strlen(line)) == 3);
    const char *tok, *p = line;
    long len = 0;
    p = next_token(p, line + strlen(line), &tok, &len);
    CHECK(p && len == 1 && *tok == '0');
    CHECK(count_tokens(line, line) == 0);
    char* tight = (char*)malloc(3);
    memcpy(tight, "A B", 3);                       // no terminator: the tokeniser must stop at `end`
    CHECK(count_tokens(tight, tight + 3) == 2);
    free(tight);
    long total = 0;
    parallel_for(1000, 7, [&](long x, long y, int) { static std::mutex m; std::lock_guard<std::mutex> g(m); total += y - x; });
    CHECK(total == 1000);
}

// ---- loader byte arithmetic (eagle_load.cpp) --------------------------------------------------------------------------
static void test_loader_windows() {
    // runs of a keep list: consecutive source lines merge, gaps split
    {
        const int32_t keep[] = {0, 1, 2, 5, 6, 9, 11, 12};
        std::vector<RowRun> runs;
        append_keep_runs(keep, 8, runs);
        CHECK(runs.size() == 4);
        CHECK(runs[0].src_row == 0 && runs[0].count == 3 && runs[1].src_row == 5 && runs[1].count == 2);
        CHECK(runs[2].src_row == 9 && runs[2].count == 1 && runs[3].src_row == 11 && runs[3].count == 2);
        append_keep_runs(keep + 3, 2, runs);   // appends: the runs of a view window that starts inside the list
        CHECK(runs.size() == 5 && runs[4].src_row == 5 && runs[4].count == 2);
        std::vector<RowRun> none;
        append_keep_runs(keep, 0, none);
        CHECK(none.empty());
    }
    // fixed-width text, width 10: the line end goes along only at the end of the line
    CHECK(text_window_bytes(0, 9, 10, true) == 11);
    CHECK(text_window_bytes(3, 9, 10, true) == 8);
    CHECK(text_window_bytes(3, 5, 10, false) == 3);
    CHECK(text_window_bytes(2, 6, 10, true) == 9);    // a keep-map window that reaches the line end reads through it
    CHECK(text_window_bytes(7, 7, 10, false) == 1);
    // 2-bit sidecar, 37 codes in rows of 16 bytes
    {
        SidecarWindow w = sidecar_window(0, 36, 37, 16);  // whole rows: one contiguous range
        CHECK(w.b0 == 0 && w.nb == 16 && w.shift == 0);
        w = sidecar_window(0, 35, 37, 16);
        CHECK(w.b0 == 0 && w.nb == 9 && w.shift == 0);
        w = sidecar_window(5, 5, 37, 16);
        CHECK(w.b0 == 1 && w.nb == 1 && w.shift == 1);
        w = sidecar_window(7, 8, 37, 16);                 // straddles a byte boundary
        CHECK(w.b0 == 1 && w.nb == 2 && w.shift == 3);
        w = sidecar_window(4, 36, 37, 16);
        CHECK(w.b0 == 1 && w.nb == 9 && w.shift == 0);
    }
}

// ---- the cached S of the scan: s_plan, s_outcome, s_slot_valid ---------------------------------------------------------
// The expectations are written out row by row from the tables of the rule (first row that applies), not taken from s_plan.
struct SWant { SSource source; SVerify verify; bool refresh; };
static SWant s_want(const SCall& c, const SPolicy& p, const SHeld& h) {
    const bool host_verify = !c.rv && !p.no_host_verify;
    const bool cacheable = c.np <= p.max_np && !p.no_scache && h.dev_np == c.np;   // (the two device buffers could be allocated)
    const bool cache_holds_n = h.dev_np == c.np && h.dev_n == c.n, host_holds_n = h.host_n == c.n;
    // source: no S at all
    if (c.w_direct) return {S_NONE, SV_NONE, false};
    // source: device cache, already trusted (the host copy is brought up to date for the calls that follow)
    if (cacheable && c.s_trusted) return {S_CACHE_TRUSTED, SV_NONE, host_verify && !host_holds_n};
    if (cacheable && p.trust_s && cache_holds_n) return {S_CACHE_TRUSTED, SV_NONE, host_verify && !host_holds_n};
    // source: device cache, to be verified -- host memcmp, else the device comparison, inline or deferred
    if (cacheable && cache_holds_n && host_verify && host_holds_n) return {S_CACHE_VERIFY, SV_HOST, false};
    if (cacheable && cache_holds_n && (c.streamed || c.bounds_flow || c.rv)) return {S_CACHE_VERIFY, SV_DEVICE_INLINE, false};
    if (cacheable && cache_holds_n) return {S_CACHE_VERIFY, SV_DEVICE_DEFERRED, false};
    // source: upload into the device cache (the upload leaves no host copy of n behind: refreshed whenever the host verifies)
    if (cacheable) return {S_CACHE_UPLOAD, SV_NONE, host_verify};
    // source: arena slot, to be verified (always by the host)
    if (!p.no_scache && h.slot && host_verify && !c.s_trusted && host_holds_n) return {S_SLOT_VERIFY, SV_HOST, false};
    // source: upload into the arena slot
    return {S_SLOT_UPLOAD, SV_NONE, host_verify && !p.no_scache};
}
static void test_scache_rule() {
    const long n = 900, np = 1024;
    long cases = 0, seen[6] = {0, 0, 0, 0, 0, 0}, seen_v[4] = {0, 0, 0, 0};
    for (int bits = 0; bits < 512; bits++)
        for (long max_np : {0L, 512L, 1024L, 16384L})          // np above, above, AT and below the limit
            for (long dev_np : {0L, 1024L, 2048L})             // no buffers, buffers of this size, of another
                for (long dev_n : {0L, 900L, 700L})            // n equal and unequal to what the cache holds
                    for (long host_n : {0L, 900L, 700L}) {
                        const SCall c = {(bits & 1) != 0, (bits & 2) != 0, n, np, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0};
                        SPolicy p;
                        p.no_scache = (bits & 32) != 0; p.no_host_verify = (bits & 64) != 0; p.trust_s = (bits & 128) != 0; p.max_np = max_np;
                        const SHeld h = {dev_np, dev_n, host_n, (bits & 256) != 0};
                        const SPlan got = s_plan(c, p, h);
                        const SWant want = s_want(c, p, h);
                        CHECK(got.source == want.source && got.verify == want.verify && got.refresh_host == want.refresh);
                        cases++; seen[got.source]++; seen_v[got.verify]++;
                        // the invariants, over the whole enumeration
                        if (c.rv) CHECK(got.verify != SV_DEVICE_DEFERRED);                         // a device of a multi-device call never defers
                        if (got.source == S_SLOT_VERIFY) CHECK(host_n == n && got.verify == SV_HOST);  // no arena-slot source without a host copy for n
                        if (c.w_direct) CHECK(got.source == S_NONE && got.verify == SV_NONE && !got.refresh_host);   // never touches the cache
                        if (c.s_trusted) CHECK(got.verify == SV_NONE);
                        if (p.no_scache && !c.w_direct) CHECK(got.source == S_SLOT_UPLOAD && !got.refresh_host);
                        if (got.refresh_host) CHECK(got.verify == SV_NONE);                         // one helper thread serves both
                        if (got.verify != SV_NONE) CHECK(got.source == S_CACHE_VERIFY || got.source == S_SLOT_VERIFY);
                        // a second attempt verifies nothing (no third): trusted, or the cache forgotten (no device copy, no host copy, no slot)
                        if (dev_n != n && host_n != n) CHECK(got.verify == SV_NONE);
                        if ((got.source == S_CACHE_TRUSTED || got.source == S_CACHE_VERIFY || got.source == S_CACHE_UPLOAD)) CHECK(np <= max_np && dev_np == np);
                    }
    CHECK(cases == 512L * 4 * 27);
    for (long v : seen) CHECK(v > 0);      // every source and every verification occurs
    for (long v : seen_v) CHECK(v > 0);
    // settling
    CHECK(s_outcome(SV_NONE, false) == S_NOTHING && s_outcome(SV_NONE, true) == S_NOTHING);
    for (SVerify v : {SV_HOST, SV_DEVICE_INLINE, SV_DEVICE_DEFERRED}) CHECK(s_outcome(v, false) == S_SAME);
    CHECK(s_outcome(SV_HOST, true) == S_OTHER_FORGOTTEN);            // the caller's S is not on the device
    CHECK(s_outcome(SV_DEVICE_INLINE, true) == S_OTHER_ON_DEVICE && s_outcome(SV_DEVICE_DEFERRED, true) == S_OTHER_ON_DEVICE);
}
// The generation rule.  The model of the arena: a counter bumped by everything that allocates, frees or replaces the block, and an address
// that MAY come back unchanged (the defect this replaces compared addresses).
static void test_scache_slot() {
    struct Arena { unsigned long gen = 1; } ar;
    const size_t o = 0;
    SSlot none;
    CHECK(!s_slot_valid(none, ar.gen, o, 900, 1024));                       // nothing recorded
    CHECK(!s_slot_valid(none, 0, 0, 0, 0));
    SSlot s;
    s.gen = ar.gen; s.off = o; s.n = 900; s.np = 1024;
    CHECK(s_slot_valid(s, ar.gen, o, 900, 1024));                           // valid at (g, o) ...
    CHECK(!s_slot_valid(s, ar.gen, o + 256, 900, 1024));                    // ... and only there
    CHECK(!s_slot_valid(s, ar.gen, o, 901, 1024) && !s_slot_valid(s, ar.gen, o, 900, 1280));
    for (const char* event : {"grow", "replace by prefetch", "drop"}) {     // each bumps the generation; the block's address is not asked
        (void)event;
        const unsigned long before = ar.gen++;
        CHECK(s_slot_valid(s, before, o, 900, 1024) && !s_slot_valid(s, ar.gen, o, 900, 1024));
        SSlot again = s;
        again.gen = ar.gen;                                                  // committed by the scan that went through after the event
        CHECK(s_slot_valid(again, ar.gen, o, 900, 1024));
        s = again;
    }
}

// ---- the modes of a scan attempt: scan_use_i8, scan_plan ----------------------------------------------------------------
// The expectations are written out from the rule (for the route: first row that applies), not taken from scan_plan.
struct ScanWant { bool use_i8; WRoute w; bool bounds_flow; int arrivals; };
static ScanWant scan_want(int scan_mode, long np, int nd, bool rccl, bool rv, bool w_direct, bool w8_wanted, bool streamed) {
    // the int8 scan: the context's mode, while 64 * 512 * np stays below 2^31
    const bool i8 = scan_mode == 1 && np * 32768L < 2147483648L;
    WRoute w;
    if (w_direct) w = W_READY;                                                       // W handed over ready
    else if (rccl && (np / 128) % nd == 0 && !(i8 && w8_wanted)) w = W_SHARED;       // rows shared + all-gather
    else if (w8_wanted) w = W_INT8;                                                  // the int8 engine
    else w = W_FP64;                                                                 // fp64, pipelined under V's upload
    const bool bounds_flow = i8 && (streamed || rv);
    int arrivals = 0;
    if (rv) {
        arrivals = 1;                                // after residency
        if (w == W_SHARED) arrivals++;               // before the all-gather
        if (bounds_flow) arrivals++;                 // with the shard's lower bound
    }
    return {i8, w, bounds_flow, arrivals};
}
static void test_scan_plan() {
    CHECK(scan_use_i8(1, 65408) && !scan_use_i8(1, 65536) && !scan_use_i8(0, 128));   // the largest padded size that takes the int8 scan, the first that does not
    long cases = 0, seen[4] = {0, 0, 0, 0};
    for (int scan_mode : {0, 1})
        for (long np : {128L, 384L, 65408L, 65536L})
            for (int nd : {1, 2, 3, 4})
                for (int bits = 0; bits < 32; bits++) {
                    const bool rccl = (bits & 1) != 0, rv = (bits & 2) != 0, w_direct = (bits & 4) != 0, w8_wanted = (bits & 8) != 0, streamed = (bits & 16) != 0;
                    const ScanPlan got = scan_plan(scan_mode, np, nd, rccl, rv, w_direct, w8_wanted, streamed);
                    const ScanWant want = scan_want(scan_mode, np, nd, rccl, rv, w_direct, w8_wanted, streamed);
                    CHECK(got.use_i8 == want.use_i8 && got.w == want.w && got.bounds_flow == want.bounds_flow && got.arrivals == want.arrivals);
                    CHECK(got.streamed == streamed && got.use_i8 == scan_use_i8(scan_mode, np));
                    cases++;
                    // the invariants, over the whole enumeration
                    CHECK(got.w == W_READY || got.w == W_SHARED || got.w == W_INT8 || got.w == W_FP64);   // exactly one route
                    seen[got.w]++;
                    CHECK((got.w == W_READY) == w_direct);                          // sharing never comes with a ready W ...
                    if (got.w == W_SHARED) CHECK(rccl && !(got.use_i8 && w8_wanted) && (np / 128) % nd == 0);   // ... nor where the int8 engine would run
                    if (got.w == W_INT8) CHECK(w8_wanted && !w_direct);
                    // devices of one call may differ in `streamed` (and an empty shard never streams): the arrivals must not
                    const ScanPlan other = scan_plan(scan_mode, np, nd, rccl, rv, w_direct, w8_wanted, !streamed);
                    CHECK(got.arrivals == other.arrivals && got.w == other.w && got.use_i8 == other.use_i8);
                    if (rv) CHECK(got.bounds_flow == other.bounds_flow);
                    if (!rv) CHECK(got.arrivals == 0);
                    else CHECK(got.arrivals >= 1 && got.arrivals <= 3);
                    if (!got.use_i8) CHECK(!got.bounds_flow);
                }
    CHECK(cases == 2L * 4 * 4 * 32);
    for (long v : seen) CHECK(v > 0);      // every route occurs
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "all";
    if (what == "all" || what == "rendezvous") test_rendezvous();
    if (what == "all" || what == "rules") test_small_rules();
    if (what == "all" || what == "text") test_text();
    if (what == "all" || what == "loader") test_loader_windows();
    if (what == "all" || what == "scache") { test_scache_rule(); test_scache_slot(); }
    if (what == "all" || what == "plan") test_scan_plan();
    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("host checks passed (%s)\n", what.c_str());
    return 0;
}
