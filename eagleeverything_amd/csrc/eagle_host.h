// eagle_host.h -- the HIP-free host pieces of libeaglehip.so: plain C++17, no device types, so that a CPU test binary can build
// them with -fsanitize=address,undefined / -fsanitize=thread (tests/host/, run by tests/test_host_sanitizers.py; GPU sanitizers do
// not exist on the target pool).  Everything here is used by eagle_api.cpp / eagle_load.cpp / eagle_ingest.cpp / eagle_i8mfma.hip as is.
#ifndef EAGLE_HOST_H
#define EAGLE_HOST_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#if defined(__HIPCC__)
#define EAGLE_HD __host__ __device__
#else
#define EAGLE_HD
#endif

// ------------------------------------------------------------------------------------------------
// Layout of the 8 KiB ctx scratch allocation (flags and small reductions of stream-ordered helpers).  One place, no overlap:
// the loaders (load stream) and the scan (compute stream) of ONE call run concurrently, so two users must never share bytes.
// ------------------------------------------------------------------------------------------------
enum : size_t {
    EAGLE_SCR_SYM = 0,             // int[2]: k_sym_check's verdict on S and V                      (eagle_kernels.hip)
    EAGLE_SCR_CERT_TOTALS = 256,   // long[4]: certification counters summed over marker blocks      (eagle_api.cpp scan_once)
    EAGLE_SCR_INGEST = 512,        // u64[2]: first third-allele / first missing position (ped), missing count (bed); double: trace  (eagle_ingest.cpp, eagle_linalg.cpp)
    EAGLE_SCR_LOADER_BAD = 1024,   // int: invalid characters / codes seen by the tile loaders       (eagle_load.cpp, any stream)
    EAGLE_SCR_SCACHE_FLAG = 2048,  // int: cached S differs from the caller's                        (eagle_api.cpp, load stream)
    EAGLE_SCR_DOT_PARTIALS = 4096, // double[256]: partial sums of eagle_dev_dot_matrices            (eagle_kernels.hip)
    EAGLE_SCR_BYTES = 8192
};
static_assert(EAGLE_SCR_SYM + 2 * sizeof(int) <= EAGLE_SCR_CERT_TOTALS, "scratch overlap");
static_assert(EAGLE_SCR_CERT_TOTALS + 4 * sizeof(long) <= EAGLE_SCR_INGEST, "scratch overlap");
static_assert(EAGLE_SCR_INGEST + 2 * sizeof(unsigned long long) <= EAGLE_SCR_LOADER_BAD, "scratch overlap");
static_assert(EAGLE_SCR_LOADER_BAD + sizeof(int) <= EAGLE_SCR_SCACHE_FLAG, "scratch overlap");
static_assert(EAGLE_SCR_SCACHE_FLAG + sizeof(int) <= EAGLE_SCR_DOT_PARTIALS, "scratch overlap");
static_assert(EAGLE_SCR_DOT_PARTIALS + 256 * sizeof(double) <= EAGLE_SCR_BYTES, "scratch overlap");

// ------------------------------------------------------------------------------------------------
// Meeting point of the per-device worker threads of one multi-device call.  arrive(ok, v) blocks until every device has
// arrived and returns the outcome OF THAT ROUND: false if any device had reported a failure by the time the round completed
// (then nobody enters the collective that follows); the largest v of the round is left in `vmax`, the sum of the `add`s in `vsum`.  Every worker calls it the
// same number of times, failed or not.  The outcome is latched per round by the last arriver: a device that leaves round k
// and fails before a slower peer has woken up from round k can only influence round k + 1 -- the peer still sees round k's
// verdict, makes its own round k + 1 arrival, and both leave round k + 1 with `false` (a sticky flag read after the wake-up
// stranded the fast device in round k + 1 for ever).  `failed` stays sticky, so every later round fails too.
// `round_failed` and `vmax` cannot change before the reader's own next arrival: the next round needs it to complete.
// ------------------------------------------------------------------------------------------------
struct Rendezvous {
    std::mutex mu;
    std::condition_variable cv;
    int n = 1, waiting = 0;
    long gen = 0;
    bool failed = false, round_failed = false;
    double acc = -HUGE_VAL, vmax = -HUGE_VAL;
    long sacc = 0, vsum = 0;
    bool arrive(bool ok, double v = -HUGE_VAL, long add = 0) {
        std::unique_lock<std::mutex> lk(mu);
        if (!ok) failed = true;
        if (v == v && v > acc) acc = v;
        sacc += add;
        const long g = gen;
        if (++waiting == n) {
            waiting = 0; vmax = acc; acc = -HUGE_VAL; vsum = sacc; sacc = 0; round_failed = failed; gen++;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return gen != g; });
        }
        return !round_failed;
    }
};

// Contiguous marker ranges, one per device; boundaries at multiples of 256 (kernel tiles, and so that the lead's range is a
// prefix view of a whole-file image the converters may have left resident).
static inline void split_markers(long L, int ndev, std::vector<long>& edge) {
    edge.assign((size_t)ndev + 1, 0);
    const long tiles = (L + 255) / 256;
    for (int k = 1; k < ndev; k++) edge[(size_t)k] = std::min(L, (tiles * k / ndev) * 256);
    edge[(size_t)ndev] = L;
}

// Column groups of eagle_spectral_scan_traits, one pass over Z each: whole traits in order, as many as fit in max_tiles MFMA tiles
// of 16 columns.  A group's lin columns (p_t + 1 per trait) are packed densely and padded to 16 once (ntl tiles); its quad columns
// (one d_t per trait) follow, padded to 16 (nt - ntl tiles).  A trait with p_t <= 31 always fits a group of its own.
#define SPT_MAX_TILES 8
struct SpectralGroup { long t0, t1; int ntl, nt; };
static inline void spectral_trait_groups(long T, const long* p, int max_tiles, std::vector<SpectralGroup>& out) {
    out.clear();
    long t0 = 0, lin = 0;
    auto close = [&](long t1) { out.push_back({t0, t1, (int)((lin + 15) / 16), (int)((lin + 15) / 16 + (t1 - t0 + 15) / 16)}); };
    for (long t = 0; t < T; t++) {
        const long lin2 = lin + p[t] + 1;
        if (t > t0 && (lin2 + 15) / 16 + (t - t0 + 1 + 15) / 16 > max_tiles) {
            close(t);
            t0 = t;
            lin = p[t] + 1;
        } else {
            lin = lin2;
        }
    }
    if (T > 0) close(T);
}
// What k_spectral_finish_traits needs of trait t: its lin columns [off, off + p] and quad column qcol in the pass output of its
// group, C (p x p, row-major) and c1 (p) at par + poff, varG.
struct SpectralTraitDesc { int off, p, qcol, t; long poff; double varG; };

// selected_loci rule (calculateMMt_rcpp.cpp:88; calculate_a_and_vara_rcpp.cpp:79; calculate_reduced_a_rcpp.cpp:74): masking fires
// iff element 0 is not NA (NA arrives as NaN).  Returns nullptr, or the message of the argument error.
static inline const char* parse_selected_core(const double* sel, long nsel, long bound, std::vector<long>& out) {
    out.clear();
    if (nsel <= 0 || !sel || isnan(sel[0])) return nullptr;
    for (long i = 0; i < nsel; i++) {
        if (isnan(sel[i])) return "NA in selected_loci after element 0";
        const long v = (long)sel[i];
        if (v < 0 || v >= bound) return "selected_loci index out of range";
        out.push_back(v);
    }
    return nullptr;
}

// Rows (multiple of 256) of a streamed chunk whose padded row length is `row_bytes`: two chunk buffers share `budget` bytes
// ((size_t)-1: no explicit budget -- streaming because HBM is full -- 8 GiB).
static inline long stream_chunk_rows_core(size_t budget, long row_bytes, long total_rows_pad) {
    if (budget == (size_t)-1) budget = (size_t)8 << 30;
    long rows = (long)(budget / 2 / (size_t)row_bytes) / 256 * 256;
    if (rows < 256) rows = 256;
    return rows < total_rows_pad ? rows : total_rows_pad;
}

// The row windows of one pass over the `rows` lines of an image: window k HOLDS the rows [lo, lo + nr), nr <= cap, and OWNS [c0, c1) --
// the rows whose results are final after its launch.  The owned ranges tile [0, rows) in order; the rows held are the owned ones with
// `back` rows before and `fwd` rows behind them, clipped to the file.  Three makers, one per pattern of the passes (each site brings
// its own capacity: the floor and min(rows, .) are the caller's):
//   row_windows_disjoint(rows, cap)        held = owned, cap rows each;
//   row_windows_overlapped(rows, w, ov)    windows of w rows that start every w - ov rows and end with the first one that reaches the
//                                          last row, which owns the rest (a window's last ov rows are written again by the next one);
//   row_windows_cores(rows, held_max, h)   cores with a halo of h rows on both sides: one window when held_max >= rows, else cores of
//                                          held_max - 2 h rows (>= 1: held_max > 2 h is the caller's floor).
struct RowWindow { long lo, nr, c0, c1; };
struct RowWindows {
    long rows, cap, core, back, fwd;
    bool to_end;     // a window that holds the last row owns everything up to it
    long at = 0;     // c0 of the next window
    bool next(RowWindow& w) {
        if (at >= rows) return false;
        const long c0 = at, lo = std::max(0L, c0 - back);
        long c1 = std::min(rows, c0 + core);
        const long hi = std::min(rows, c1 + fwd);
        if (to_end && hi >= rows) c1 = rows;
        w = {lo, hi - lo, c0, c1};
        at = c1;
        return true;
    }
};
static inline RowWindows row_windows_disjoint(long rows, long cap) { return {rows, cap, cap, 0, 0, false}; }
static inline RowWindows row_windows_overlapped(long rows, long w, long overlap) { return {rows, w, w - overlap, 0, overlap, true}; }
static inline RowWindows row_windows_cores(long rows, long held_max, long halo) {
    return {rows, held_max, held_max >= rows ? rows : held_max - 2 * halo, halo, halo, false};
}

// The marker ranges of the admixture step's Q kernel (include/eagle_hip.h section 1b''''v): ceil(n / 16) tiles of individuals do not
// fill the card, so [0, L) is cut into S ranges of `len` markers (a multiple of 16; the last one is shorter), range s = [s len,
// min(L, (s + 1) len)).  A function of (n, L) alone: the sums of a tile depend on it and on nothing else.  S aims at
// ADMIX_PLAN_WAVES waves and keeps the partials buffer part[S][n16][16] fp64, n16 = n rounded up to 16, within admix_part_cap(n):
// ADMIX_PART_BYTES, or one range's worth where that alone is more.
#define ADMIX_PLAN_WAVES 2048L
#define ADMIX_PART_BYTES (64L << 20)
struct AdmixPlan { long S, len; };
static inline long admix_part_cap(long n) {
    const long one = (n + 15) / 16 * 16 * 16 * 8;
    return one > ADMIX_PART_BYTES ? one : ADMIX_PART_BYTES;
}
static inline AdmixPlan admix_range_plan(long n, long L) {
    const long tiles = (n + 15) / 16, mt = (L + 15) / 16, one = tiles * 16 * 16 * 8;
    long want = (ADMIX_PLAN_WAVES + tiles - 1) / tiles;
    want = std::min(want, std::max(1L, admix_part_cap(n) / one));
    want = std::max(1L, std::min(want, mt));
    const long len_t = (mt + want - 1) / want;               // 16-marker tiles per range
    return {(mt + len_t - 1) / len_t, len_t * 16};
}

// Pieces per worker of an XCD's last, partly filled round of `tail` workers on 32 CUs (0 < tail < 32): the workers are cut along
// their column-tile pairs into p equal pieces, the tail * p pieces run in ceil(tail * p / 32) rounds of 1/p worker-time each; p <=
// min(npair, VARA_TAIL_PMAX) minimising that cost (p = 1: one whole worker-time for a round that may be 1/32 full; large p: tail/32).
#define VARA_TAIL_PMAX 16
EAGLE_HD static inline int vara_tail_pieces(int tail, int npair) {
    if (tail <= 0) return 1;
    int best = 1, bn = 1, bd = 1;  // cost bn / bd
    const int pmax = npair < VARA_TAIL_PMAX ? npair : VARA_TAIL_PMAX;
    for (int p = 2; p <= pmax; p++) {
        const int rounds = (tail * p + 31) >> 5;
        if (rounds * bd < bn * p) { best = p; bn = rounds; bd = p; }
    }
    return best;
}

// ------------------------------------------------------------------------------------------------
// The cached S of the scan (SCache, eagle_api.cpp): S = inv_MMt_sqrt is the same matrix in every find_qtl call of an AM() run, so the
// last call's copy stays on the device -- in a buffer of its own up to max_np padded individuals, else where the scan left it in the
// arena -- and the next call computes on it while the caller's matrix is compared with it.  s_plan decides from plain values where a
// call's S comes from, how the caller's matrix is verified and when that is settled; s_outcome what settling means; s_slot_valid
// whether the arena still holds the slot.  No pointer, no device: tests/host/test_host.cpp enumerates all of it.
// ------------------------------------------------------------------------------------------------
struct SPolicy {               // the environment switches, read once per call (tests toggle them between calls of one process)
    bool no_scache = false;    // EAGLE_HIP_NO_SCACHE: every call uploads S
    long max_np = 16384;       // EAGLE_HIP_SCACHE_MAX_NP: above it no second device copy (20 GB at n = 50,000): the arena slot
    bool no_host_verify = false;  // EAGLE_HIP_NO_HOST_SVERIFY: always the device comparison
    bool trust_s = false;      // EAGLE_HIP_EXPERIMENT_TRUST_S: measurement only -- a changed S would go unnoticed
};
struct SCall { bool w_direct, s_trusted; long n, np; bool rv, streamed, bounds_flow; };
struct SHeld {      // what the cache holds
    long dev_np;    // the two device buffers are np x np (0: none -- an allocation failure falls through to the arena slot)
    long dev_n;     // ... and the first holds the S of a call with that many individuals (0: none)
    long host_n;    // the host copy holds one (0: none)
    bool slot;      // the arena slot holds this call's (n, np) (s_slot_valid)
};
enum SSource { S_NONE, S_CACHE_TRUSTED, S_CACHE_VERIFY, S_CACHE_UPLOAD, S_SLOT_VERIFY, S_SLOT_UPLOAD };
// host memcmp on the cores that idle while the card works, settled at the end of the call; else the device comparison under the scan,
// settled right behind W when the host is in the loop anyway (marker blocks, several devices), else at the end from a helper thread
enum SVerify { SV_NONE, SV_HOST, SV_DEVICE_INLINE, SV_DEVICE_DEFERRED };
struct SPlan { SSource source = S_NONE; SVerify verify = SV_NONE; bool refresh_host = false; };
static inline SPlan s_plan(const SCall& c, const SPolicy& p, const SHeld& h) {
    SPlan r;
    if (c.w_direct) return r;   // W arrives ready: no S at all
    const bool host_verify = !c.rv && !p.no_host_verify;
    const bool buffers = h.dev_np == c.np, on_device = buffers && h.dev_n == c.n, on_host = h.host_n == c.n;
    const SVerify device = (c.streamed || c.bounds_flow || c.rv) ? SV_DEVICE_INLINE : SV_DEVICE_DEFERRED;   // (a device of a multi-device call never defers)
    if (c.np <= p.max_np && !p.no_scache && buffers) {
        if (c.s_trusted || (p.trust_s && on_device)) { r.source = S_CACHE_TRUSTED; r.refresh_host = host_verify && !on_host; }
        else if (on_device) { r.source = S_CACHE_VERIFY; r.verify = (host_verify && on_host) ? SV_HOST : device; }
        else { r.source = S_CACHE_UPLOAD; r.refresh_host = host_verify; }   // (the upload has invalidated the host copy)
    } else if (!p.no_scache && h.slot && host_verify && !c.s_trusted && on_host) {
        r.source = S_SLOT_VERIFY; r.verify = SV_HOST;
    } else {
        r.source = S_SLOT_UPLOAD; r.refresh_host = host_verify && !p.no_scache;
    }
    return r;
}
// S_SAME: a hit.  S_OTHER_ON_DEVICE: the device comparison has left the caller's S in the scratch buffer -- the two buffers are swapped and
// the work is redone on it (settled inline: only the operands; at the end: the whole scan a second time, s_trusted).  S_OTHER_FORGOTTEN:
// the host comparison: the caller's S is not on the device -- the cache forgets what it holds, the scan runs a second time and uploads.
enum SOutcome { S_NOTHING, S_SAME, S_OTHER_ON_DEVICE, S_OTHER_FORGOTTEN };
static inline SOutcome s_outcome(SVerify how, bool differs) {
    return how == SV_NONE ? S_NOTHING : !differs ? S_SAME : how == SV_HOST ? S_OTHER_FORGOTTEN : S_OTHER_ON_DEVICE;
}
// The arena slot of S, valid by GENERATION and not by address: eagle_ctx::arena_gen counts every allocation, release or replacement of
// the arena (a freed block's address may come back), and the record holds only at the generation and offset it was made at.
struct SSlot { unsigned long gen = 0; size_t off = 0; long n = 0, np = 0; };   // n = 0: none
static inline bool s_slot_valid(const SSlot& s, unsigned long gen, size_t off, long n, long np) {
    return s.n > 0 && s.gen == gen && s.off == off && s.n == n && s.np == np;
}

// ------------------------------------------------------------------------------------------------
// The modes of one scan attempt on one device (scan_once, eagle_api.cpp), decided here from plain values and only read by the stages.
// scan_use_i8 is known before the file is looked at (the residency step sizes its arena estimate with it); scan_plan is made once
// the residency step has said whether the shard is streamed.  No pointer, no device: tests/host/test_host.cpp enumerates all of it.
//   use_i8       the digit-slice scan on the int8 MFMA: the context's mode, and 64 * 512 * np below 2^31 (the kernel's int32 sums).
//   w            where W comes from, exactly one route:
//                  W_READY    eagle_scan_with_W handed W and v over: only the fold;
//                  W_SHARED   fp64 products, 1/nd of W's rows per device + ONE all-gather -- needs device collectives and np / 128 rows
//                             blocks that divide by nd, and is never taken where the int8 engine would run: those products cost half
//                             as much and are a deterministic function of S and V, so every device forms them itself;
//                  W_INT8     the int8 engine (which may decline at run time and then runs the fp64 products: the route's business);
//                  W_FP64     the fp64 products, pipelined under V's upload.
//   bounds_flow  a digit-slice scan that does not see all its markers at once -- marker blocks of a streamed file, shards of several
//                devices -- keeps per-marker bounds and certifies against ONE lower bound of the maximum after the last block.
//   arrivals     rendezvous rounds of the call (0 without a rendezvous): one after residency, one before the all-gather, one with the
//                shard's lower bound.  Devices of one call may differ in `streamed` -- the count must not, and does not: with a
//                rendezvous bounds_flow is use_i8.
// ------------------------------------------------------------------------------------------------
enum WRoute { W_READY, W_SHARED, W_INT8, W_FP64 };
struct ScanPlan { bool use_i8 = false; WRoute w = W_FP64; bool streamed = false, bounds_flow = false; int arrivals = 0; };
static inline bool scan_use_i8(int scan_mode, long np) { return scan_mode == 1 && 64.0 * 512.0 * (double)np < 2147483648.0; }
// rccl: live device collectives; rv: the call has a rendezvous; w8_wanted: eagle_w8_wanted's answer for np
static inline ScanPlan scan_plan(int scan_mode, long np, int nd, bool rccl, bool rv, bool w_direct, bool w8_wanted, bool streamed) {
    ScanPlan p;
    p.use_i8 = scan_use_i8(scan_mode, np);
    const bool share_w = !w_direct && rccl && (np / 128) % nd == 0 && !(p.use_i8 && w8_wanted);   // the same answer on every device
    p.w = w_direct ? W_READY : share_w ? W_SHARED : w8_wanted ? W_INT8 : W_FP64;
    p.streamed = streamed;
    p.bounds_flow = p.use_i8 && (streamed || rv);
    p.arrivals = rv ? 1 + (share_w ? 1 : 0) + (p.bounds_flow ? 1 : 0) : 0;
    return p;
}

// What the int8 W engine keeps WITH S (eagle_w8.hip): the digit image of S, its row statistics and W8Stats, S 1 and S^T 1 -- everything
// eagle_w8_begin computes from S alone.  The record says which S they were made from and where they lie; a call may skip the S work only
// if w8_keep_valid says so.  s_gen names the CONTENT of the image at Sa: the owner of S (the SCache of the reference-shaped call,
// eagle_dev_declare_s of the device-resident one) gives every new content a new non-zero number, and 0 = "nobody vouches for it":
// never valid, nothing recorded.  ws_gen counts every allocation or release of the w8 workspace (a freed block's address may come back).
struct W8Keep { const void* Sa = nullptr; long n = 0, np = 0; const void* ws = nullptr; unsigned long ws_gen = 0, s_gen = 0; const void* stream = nullptr; };
static inline bool w8_keep_valid(const W8Keep& k, const void* Sa, long n, long np, const void* ws, unsigned long ws_gen, unsigned long s_gen,
                                 const void* stream) {
    return s_gen != 0 && k.s_gen == s_gen && k.Sa != nullptr && k.Sa == Sa && k.n == n && k.np == np && k.ws != nullptr && k.ws == ws &&
           k.ws_gen == ws_gen && k.stream == stream;
}
static inline void w8_keep_forget(W8Keep& k) { k = W8Keep(); }   // (workspace gone, S forgotten, the engine declined)
// eagle_dev_declare_s: the caller's promise that the image at Sa is S and stays as it is.  It vouches for exactly that (pointer, n, n_pad).
struct W8Declared { const void* Sa = nullptr; long n = 0, np = 0; unsigned long s_gen = 0; };
static inline unsigned long w8_declared_gen(const W8Declared& d, const void* Sa, long n, long np) {
    return (d.s_gen != 0 && d.Sa == Sa && d.n == n && d.np == np) ? d.s_gen : 0;
}

// ------------------------------------------------------------------------------------------------
// Text side of the ingestion (eagle_ingest.cpp): line index of a memory-mapped file and the whitespace tokeniser.
// ------------------------------------------------------------------------------------------------
static inline void parallel_for(long n, int threads, const std::function<void(long, long, int)>& fn) {
    if (n <= 0) return;
    if (threads <= 1 || n < 2 * threads) { fn(0, n, 0); return; }
    std::vector<std::thread> pool;
    const long per = (n + threads - 1) / threads;
    for (int t = 0; t < threads; t++) {
        const long a = t * per, b = std::min(n, a + per);
        if (a >= b) break;
        pool.emplace_back(fn, a, b, t);
    }
    for (auto& th : pool) th.join();
}

// getline() semantics: lines end at '\n'; a non-empty tail without '\n' is a line too.  starts has nlines+1 entries,
// line i is [starts[i], starts[i+1] - 1) except for an unterminated last line, whose end is the file size (`tail`).
struct LineIndex {
    std::vector<size_t> starts;
    bool tail = false;
    size_t size = 0;
    long nlines() const { return (long)starts.size() - 1; }
    size_t begin(long i) const { return starts[(size_t)i]; }
    size_t end(long i) const { return (tail && i == nlines() - 1) ? size : starts[(size_t)i + 1] - 1; }
};

static inline void index_lines_buf(const char* base, size_t size, int threads, LineIndex& ix) {
    ix.size = size;
    ix.tail = false;
    std::vector<std::vector<size_t>> part((size_t)std::max(1, threads));
    parallel_for((long)size, threads, [&](long a, long b, int t) {
        auto& v = part[(size_t)t];
        const char* p = base + a;
        const char* e = base + b;
        while (p < e) {
            const char* q = (const char*)memchr(p, '\n', (size_t)(e - p));
            if (!q) break;
            v.push_back((size_t)(q - base) + 1);
            p = q + 1;
        }
    });
    ix.starts.clear();
    ix.starts.push_back(0);
    for (auto& v : part) ix.starts.insert(ix.starts.end(), v.begin(), v.end());
    if (ix.starts.back() < size) { ix.starts.push_back(size + 1); ix.tail = true; }
    if (size == 0) ix.starts.assign(1, 0);
}

static inline bool is_ws(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }
static inline const char* next_token(const char* p, const char* end, const char** tok, long* len) {
    while (p < end && is_ws(*p)) p++;
    if (p >= end) return nullptr;
    *tok = p;
    while (p < end && !is_ws(*p)) p++;
    *len = p - *tok;
    return p;
}
static inline long count_tokens(const char* p, const char* end) {
    const char* tok;
    long len, n = 0;
    while ((p = next_token(p, end, &tok, &len)) != nullptr) n++;
    return n;
}

// ------------------------------------------------------------------------------------------------
// PLINK binary genotypes (.bed) in front of the ingestion (eagle_create_ascii_from_bed): 3 header bytes, then in SNP-major mode
// one row per marker of ceil(n/4) bytes, individual 4b+q at bits 2q of byte b; codes 00 hom A1, 01 missing, 10 het, 11 hom A2.
// ------------------------------------------------------------------------------------------------
enum { BED_HEADER_OK = 0, BED_HEADER_SHORT = 1, BED_HEADER_MAGIC = 2, BED_HEADER_INDIVIDUAL_MAJOR = 3, BED_HEADER_MODE = 4 };
#define BED_HEADER_BYTES 3
// verdict on the first `got` bytes of the file (got < 3: the file ends inside its header)
static inline int bed_check_header(const unsigned char* h, long got) {
    if (got < BED_HEADER_BYTES) return BED_HEADER_SHORT;
    if (h[0] != 0x6c || h[1] != 0x1b) return BED_HEADER_MAGIC;
    if (h[2] == 0x00) return BED_HEADER_INDIVIDUAL_MAJOR;
    return h[2] == 0x01 ? BED_HEADER_OK : BED_HEADER_MODE;
}
static inline long bed_row_bytes(long n) { return (n + 3) / 4; }
static inline long long bed_expected_size(long n, long L) { return BED_HEADER_BYTES + (long long)L * bed_row_bytes(n); }
// Row stride of the 2-bit sidecar of a text file of `cols` characters per line: the packed bytes padded to 16.
static inline long sidecar_row_bytes(long cols) { return ((cols + 3) / 4 + 15) / 16 * 16; }
// Marker windows of the bed ingestion: w markers (a multiple of 256, at least 256, at most L_pad) whose text, w x (n + 1) bytes,
// fits `text_cap` bytes and whose int8 tile, w x n_pad, obeys `budget` ((size_t)-1: none).  Window k starts at marker k * w and
// holds `real` markers of the file in `padded` tile rows: the last window reaches L_pad, so that the windows tile the padded image.
static inline long bed_window_markers(long n, long n_pad, long L_pad, size_t text_cap, size_t budget) {
    long w = (long)(text_cap / (size_t)(n + 1)) / 256 * 256;
    if (budget != (size_t)-1) w = std::min(w, (long)(budget / (size_t)n_pad) / 256 * 256);
    if (w < 256) w = 256;
    return w > L_pad ? L_pad : w;
}
struct BedWindow { long c0, real, padded; };
static inline BedWindow bed_window(long k, long w, long L, long L_pad) {
    const long c0 = k * w;
    return {c0, std::min(w, L - c0), std::min(w, L_pad - c0)};
}
static inline long bed_window_count(long w, long L) { return (L + w - 1) / w; }
// The staging rule of every eagle_bed_* call (the loaders' rule): the file rows of rb bytes a staging window holds -- 64 MiB of them, or
// a quarter of max_memory_in_Gbytes when that is less, never fewer than one -- before the caller's own caps.
static inline long bed_stage_rows(long rb, double mem_gb) {
    double cap = 67108864.0;
    if (mem_gb > 0) cap = std::min(cap, mem_gb * 1e9 / 4.0);
    return std::max(1L, (long)cap / rb);
}
// The panel windows of include/eagle_hip.h section 1b'''iv.  fidx: panel marker -> file row, increasing; empty: the identity.  The window
// that starts at panel marker lo ends at the largest hi <= linc with hi - lo <= wmax whose file rows span at most S rows, but it holds
// at least `need` markers (what the call needs to advance) or the rest of the panel.
static inline long bed_panel_file_row(const std::vector<long>& fidx, long p) { return fidx.empty() ? p : fidx[(size_t)p]; }
static inline long bed_panel_window_end(long lo, long need, long wmax, long S, long linc, const std::vector<long>& fidx) {
    const long floor_hi = std::min(linc, lo + need);
    long hi = std::min(linc, lo + wmax);
    if (fidx.empty()) hi = std::min(hi, lo + S);
    else hi = (long)(std::upper_bound(fidx.begin() + lo, fidx.begin() + hi, fidx[(size_t)lo] + S - 1) - fidx.begin());
    return std::max(hi, floor_hi);
}

// ------------------------------------------------------------------------------------------------
// Byte arithmetic of the genotype loader (eagle_load.cpp).
// ------------------------------------------------------------------------------------------------
// `count` consecutive source lines from `src_row`, loaded to consecutive destination rows.
struct RowRun { long src_row, count; };
// Runs of consecutive values of keep[0 .. n): the source lines of n consecutive lines of an M view.
static inline void append_keep_runs(const int32_t* keep, long n, std::vector<RowRun>& runs) {
    for (long i = 0; i < n;) {
        long j = i + 1;
        while (j < n && keep[j] == keep[j - 1] + 1) j++;
        runs.push_back({(long)keep[i], j - i});
        i = j;
    }
}
// Bytes read of every line of fixed-width text (`width` characters + '\n') for the characters [c_first, c_last]: from c_first on.
// A window that reaches the line end takes the '\n' along, and the decode kernels check it: that is what detects text that is not
// fixed-width after all.
static inline long text_window_bytes(long c_first, long c_last, long width, bool at_end) { return (at_end ? width + 1 : c_last + 1) - c_first; }
// Bytes read of every row of the 2-bit sidecar (4 codes per byte, `cols` codes in `row_bytes` bytes) for the characters
// [c_first, c_last]: nb bytes from byte b0, the first wanted code at 2-bit position `shift` of byte b0.  Whole rows are read
// whole, so that consecutive rows are one contiguous byte range.
struct SidecarWindow { long b0, nb; int shift; };
static inline SidecarWindow sidecar_window(long c_first, long c_last, long cols, long row_bytes) {
    const long b0 = c_first / 4;
    const bool whole_rows = c_first == 0 && c_last + 1 == cols;
    return {b0, whole_rows ? row_bytes : c_last / 4 + 1 - b0, (int)(c_first % 4)};
}

// ------------------------------------------------------------------------------------------------
// LD scores and the LD decay curve (include/eagle_hip.h section 1b'''v): the argument rule of eagle_ld_stats / eagle_bed_ld_stats.
// ------------------------------------------------------------------------------------------------
// What is wrong with a call over `markers` panel markers, or NULL: window in [1, 256]; markers < 2^31; markers * window <= 2^33 (at
// most that many pairs of at most 2^30 each: no bin sum passes 2^63); max_dist > 0 needs pos; nbins in [0, 512]; with edges and
// nbins > 0 the nbins + 1 edges increase strictly and both bin outputs are given.  Reads edges[0 .. nbins] and nothing else.
static inline const char* ld_stats_arg_error(long markers, long window, bool has_pos, long max_dist, const int64_t* edges, long nbins,
                                             bool has_bin_outputs) {
    if (window < 1 || window > 256) return "window must be in [1, 256]";
    if (markers > 0x7fffffffL) return "2^31 markers or more";
    if (markers * window > (1L << 33)) return "markers x window above 2^33 (a bin sum could pass 2^63)";
    if (max_dist > 0 && !has_pos) return "max_dist needs pos";
    if (nbins < 0 || nbins > 512) return "nbins outside [0, 512]";
    if (edges && nbins > 0) {
        if (!has_bin_outputs) return "NULL argument (the bin outputs, with edges given)";
        for (long b = 0; b < nbins; b++)
            if (!(edges[b] < edges[b + 1])) return "edges must be strictly increasing";
    }
    return nullptr;
}

// ------------------------------------------------------------------------------------------------
// The exact line-score pass (include/eagle_hip.h section 1b''''i): the argument rule of eagle_sample_scores / eagle_marker_scores and
// the balanced base-256 digits of a weight.
// ------------------------------------------------------------------------------------------------
#define SCORES_MAX_COLUMNS 64L
#define SCORES_MAX_WEIGHT 1073741824L   /* 2^30 */
#define SCORES_MAX_LINE 8388480L        /* the largest multiple of 128 below 2^23 */
// Digit p (0 .. 3) of w = d0 + 256 d1 + 256^2 d2 + 256^3 d3, d in [-128, 127]:  d_p = ((w_p + 128) & 255) - 128,  w_{p+1} = (w_p - d_p) >> 8
// (the difference is a multiple of 256, so the shift is exact).  Four digits hold every |w| <= 2^30: the largest four-digit number is
// 127 (256^4 - 1) / 255 > 2^30 and the smallest -128 (256^4 - 1) / 255 < -2^30.
EAGLE_HD static inline int score_digit(int32_t w, int p) {
    int32_t x = w, d = 0;
    for (int q = 0; q <= p; q++) {
        d = ((x + 128) & 255) - 128;
        x = (x - d) >> 8;
    }
    return d;
}
// The four digits of w; returns what is left of w behind them (0 for every |w| <= 2^30).
static inline int32_t score_digits(int32_t w, int8_t d[4]) {
    int32_t x = w;
    for (int p = 0; p < 4; p++) {
        const int32_t dp = ((x + 128) & 255) - 128;
        d[p] = (int8_t)dp;
        x = (x - dp) >> 8;
    }
    return x;
}
// What is wrong with a call over `lines` lines of `line_len` characters, T weight columns and the T x line_len weights w (may be NULL: not
// checked), or NULL.  plane_mask (may be NULL): bit p set iff digit plane p is not zero over all the weights.
static inline const char* scores_arg_error(long lines, long line_len, long T, const int32_t* w, int* plane_mask) {
    if (lines <= 0 || line_len <= 0) return "dims must be positive";
    if (T < 1 || T > SCORES_MAX_COLUMNS) return "T outside [1, 64]";
    if (line_len > SCORES_MAX_LINE) return "a line longer than EAGLE_SCORES_MAX_LINE = 8,388,480 characters";
    if (lines > 0x7fffffffL) return "2^31 lines or more";
    int mask = 0;
    if (w) {
        const long count = T * line_len;
        for (long i = 0; i < count; i++) {
            const int32_t x = w[i];
            if (x > SCORES_MAX_WEIGHT || x < -SCORES_MAX_WEIGHT) return "a weight beyond +-2^30";
            if (x == 0 || mask == 15) continue;
            int8_t d[4];
            (void)score_digits(x, d);
            for (int p = 0; p < 4; p++) if (d[p]) mask |= 1 << p;
        }
    }
    if (plane_mask) *plane_mask = mask;
    return nullptr;
}

// ------------------------------------------------------------------------------------------------
// Runs of homozygosity (include/eagle_hip.h section 1b'''vi): the argument rule of eagle_roh / eagle_bed_roh, the block table of rule 2
// and the check of pos.
// ------------------------------------------------------------------------------------------------
#define ROH_MAX_WINDOW 64L
#define ROH_MAX_DENSITY 2147483648L   /* 2^31 */
// The nine fields of eagle_roh_params in their order: w, win_het, win_miss, thr16, min_snp, min_len, max_gap, max_density, max_het.
// What is wrong with a call over `markers` panel markers, or NULL.
static inline const char* roh_arg_error(const int64_t p[9], long markers, long seg_cap, bool has_seg_out) {
    if (p[0] < 1 || p[0] > ROH_MAX_WINDOW) return "w must be in [1, 64]";
    if (p[1] < 0) return "win_het must not be negative";
    if (p[2] < 0) return "win_miss must not be negative";
    if (p[3] < 0 || p[3] > 65536) return "thr16 must be in [0, 65536]";
    if (p[4] < 1) return "min_snp must be at least 1";
    if (p[5] < 0) return "min_len must not be negative";
    if (p[6] < 0) return "max_gap must not be negative";
    if (p[7] < 0 || p[7] > ROH_MAX_DENSITY) return "max_density must be in [0, 2^31]";
    if (markers > 0x7fffffffL) return "2^31 markers or more";
    if (seg_cap < 0) return "seg_cap must not be negative";
    if (seg_cap > 0 && !has_seg_out) return "NULL argument (seg_out, with seg_cap > 0)";
    return nullptr;
}
// Block bounds of rule 2: blk[0] = 0 < blk[1] < ... < blk[nb] = markers, a block a maximal run of equal chrom (NULL: one block).
static inline void roh_block_table(const int32_t* chrom, long markers, std::vector<int32_t>& blk) {
    blk.clear();
    blk.push_back(0);
    if (chrom)
        for (long m = 1; m < markers; m++)
            if (chrom[m] != chrom[m - 1]) blk.push_back((int32_t)m);
    blk.push_back((int32_t)markers);
}
// The first marker m with pos[m] < pos[m - 1] inside a block, or -1 (pos NULL: -1).  Block edges are not compared across.
static inline long roh_pos_check(const int64_t* pos, const std::vector<int32_t>& blk) {
    if (!pos) return -1;
    for (size_t b = 0; b + 1 < blk.size(); b++)
        for (long m = (long)blk[b] + 1; m < (long)blk[b + 1]; m++)
            if (pos[m] < pos[m - 1]) return m;
    return -1;
}
// Exclusive scan of the segment counts by (individual, block), in that order; returns the total.
static inline int64_t roh_offsets(const int32_t* cnt, size_t cells, int64_t* offs) {
    int64_t t = 0;
    for (size_t c = 0; c < cells; c++) { offs[c] = t; t += cnt[c]; }
    return t;
}

// ------------------------------------------------------------------------------------------------
// Pairwise IBD-type segments (include/eagle_hip.h section 1b'''vii): the argument rule of eagle_ibd / eagle_bed_ibd, the check of a pair
// list and the scan of the per-pair counts.  Blocks and pos are those of ROH (roh_block_table, roh_pos_check).
// ------------------------------------------------------------------------------------------------
#define IBD_MAX_PAIRS 134217728L   /* 2^27 */
// The five fields of eagle_ibd_params in their order: mode, min_snp, min_len, max_gap, merge_min.  npairs counts the list, or is ignored
// when has_pairs is false (all pairs of n individuals).  What is wrong with a call over `markers` panel markers, or NULL.
static inline const char* ibd_arg_error(const int64_t p[5], long n, long markers, bool has_pairs, long npairs, long seg_cap, bool has_seg_out) {
    if (p[0] != 1 && p[0] != 2) return "mode must be 1 (ibs1) or 2 (ibs2)";
    if (p[1] < 1) return "min_snp must be at least 1";
    if (p[2] < 0) return "min_len must not be negative";
    if (p[3] < 0) return "max_gap must not be negative";
    if (p[4] < 0) return "merge_min must not be negative";
    if (markers > 0x7fffffffL) return "2^31 markers or more";
    if (has_pairs) {
        if (npairs < 1 || npairs > IBD_MAX_PAIRS) return "the number of pairs must be in [1, 2^27]";
    } else {
        if (n < 2) return "all pairs need at least two individuals";
        if (n > 16385L) return "more than 2^27 pairs: give a list";   /* 16385 * 16384 / 2 == 2^27 + 8192 > 2^27 >= 16384 * 16383 / 2 */
        if (n * (n - 1) / 2 > IBD_MAX_PAIRS) return "more than 2^27 pairs: give a list";
    }
    if (seg_cap < 0) return "seg_cap must not be negative";
    if (seg_cap > 0 && !has_seg_out) return "NULL argument (seg_out, with seg_cap > 0)";
    return nullptr;
}
// The number of pairs of a call: the list's, or n (n - 1) / 2.
static inline long ibd_pair_count(long n, bool has_pairs, long npairs) { return has_pairs ? npairs : n * (n - 1) / 2; }
// The ordinal of (i, j), 0 <= i < j < n, among all pairs in row-major upper-triangle order.
static inline long ibd_pair_ordinal(long n, long i, long j) { return i * n - i * (i + 1) / 2 + (j - i - 1); }
// The first list entry that is not 0 <= i < j < n, or -1.
static inline long ibd_pairs_check(const int32_t* pairs, long npairs, long n) {
    for (long k = 0; k < npairs; k++) {
        const long i = pairs[2 * k], j = pairs[2 * k + 1];
        if (i < 0 || i >= j || j >= n) return k;
    }
    return -1;
}
// Exclusive scan of the segment counts (column 0 of the P x 4 pair table) by pair ordinal; returns the total.
static inline int64_t ibd_offsets(const int64_t* pair_tab, size_t P, int64_t* offs) {
    int64_t t = 0;
    for (size_t k = 0; k < P; k++) { offs[k] = t; t += pair_tab[4 * k]; }
    return t;
}
// The cut plane of rule 3 (the device builds the same in k_ibd_cuts): bit m set where a piece starts.
static inline void ibd_cut_plane(const int32_t* chrom, const int64_t* pos, long max_gap, long markers, std::vector<uint64_t>& cut) {
    cut.assign((size_t)((markers + 63) / 64), 0);
    for (long m = 0; m < markers; m++) {
        bool c = m == 0;
        if (m > 0 && chrom && chrom[m] != chrom[m - 1]) c = true;
        if (m > 0 && pos && max_gap > 0 && pos[m] - pos[m - 1] > max_gap) c = true;
        if (c) cut[(size_t)(m >> 6)] |= 1ull << (m & 63);
    }
}

// ------------------------------------------------------------------------------------------------
// Mendel errors and parentage assignment (include/eagle_hip.h section 1b'''viii): the error word of rule 3 on the bit planes (shared
// with the kernels of eagle_mendel.hip), the argument rules of eagle_mendel / eagle_parentage, the checks of a trio list and of a
// candidate list, and the ordinal of a candidate pair.
// ------------------------------------------------------------------------------------------------
#define MENDEL_MAX_TRIOS 134217728L   /* 2^27 */
// The wave-uniform part of rule 3 for one (child, father): hc = the child's hets, E = x | u & Bm | v & Am.
struct MendelXUV { uint64_t x, u, v; };
static inline EAGLE_HD MendelXUV mendel_xuv(uint64_t ac, uint64_t bc, uint64_t cc, uint64_t af, uint64_t bf) {
    const uint64_t hc = cc & ~ac & ~bc;
    return MendelXUV{(ac & bf) | (bc & af), ac | (hc & bf), bc | (hc & af)};
}
// Bit m set where the trio has a Mendel error at marker m of the word.  A and B imply called, so the parents' C planes are not needed.
static inline EAGLE_HD uint64_t mendel_error_word(uint64_t ac, uint64_t bc, uint64_t cc, uint64_t af, uint64_t bf, uint64_t am, uint64_t bm) {
    const MendelXUV t = mendel_xuv(ac, bc, cc, af, bf);
    return t.x | (t.u & bm) | (t.v & am);
}
// The bits of word w that are panel markers: all ones but for the last word of a panel whose length is no multiple of 64.
static inline EAGLE_HD uint64_t mendel_word_mask(long w, long markers) {
    const long left = markers - 64 * w;
    return left >= 64 ? ~0ull : (left <= 0 ? 0ull : (1ull << left) - 1ull);
}
// What is wrong with a call of eagle_mendel / eagle_bed_mendel over `markers` panel markers, or NULL.
static inline const char* mendel_arg_error(long markers, long ntrios) {
    if (markers > 0x7fffffffL) return "2^31 markers or more";
    if (ntrios < 1 || ntrios > MENDEL_MAX_TRIOS) return "the number of trios must be in [1, 2^27]";
    return nullptr;
}
// The first trio (c, f, m) that is not 0 <= c < n, -1 <= f, m < n, c != f, c != m, f != m unless both are -1; or -1.
static inline long mendel_trios_check(const int32_t* trios, long ntrios, long n) {
    for (long k = 0; k < ntrios; k++) {
        const long c = trios[3 * k], f = trios[3 * k + 1], m = trios[3 * k + 2];
        if (c < 0 || c >= n || f < -1 || f >= n || m < -1 || m >= n || c == f || c == m || (f == m && f >= 0)) return k;
    }
    return -1;
}
// What is wrong with a call of eagle_parentage / eagle_bed_parentage, or NULL.  An empty list is one unknown parent.
static inline const char* parentage_arg_error(long markers, long n_o, long n_s, long n_d, long min_overlap, long allow_self) {
    if (markers > 0x7fffffffL) return "2^31 markers or more";
    if (n_o < 1 || n_o > MENDEL_MAX_TRIOS) return "the number of offspring must be in [1, 2^27]";
    if (n_s < 0 || n_d < 0) return "a candidate list has a negative length";
    if (n_s == 0 && n_d == 0) return "both candidate lists are empty";
    if (n_s > 0x7fffffffL || n_d > 0x7fffffffL || (n_s > 0 ? n_s : 1) * (n_d > 0 ? n_d : 1) > 0x7fffffffL)
        return "sires x dams must be below 2^31";
    if (min_overlap < 0 || min_overlap > 0x7fffffffL) return "min_overlap must be in [0, 2^31)";
    if (allow_self != 0 && allow_self != 1) return "allow_self must be 0 or 1";
    return nullptr;
}
// The first entry of a list of individual indices that is outside [0, n) (*dup = false) or repeats an earlier entry (*dup = true); or -1.
static inline long parentage_list_check(const int32_t* list, long cnt, long n, bool* dup) {
    *dup = false;
    if (cnt <= 0) return -1;
    for (long k = 0; k < cnt; k++)
        if (list[k] < 0 || list[k] >= n) return k;
    std::vector<int32_t> s(list, list + cnt);
    std::sort(s.begin(), s.end());
    int32_t twice = -1;
    for (size_t k = 1; k < s.size(); k++)
        if (s[k] == s[k - 1]) { twice = s[k]; break; }
    if (twice < 0) return -1;
    *dup = true;
    bool seen = false;
    for (long k = 0; k < cnt; k++)
        if (list[k] == twice) { if (seen) return k; seen = true; }
    return -1;
}
// The ordinal of the candidate (s_idx-th sire, d_idx-th dam): ties in the error count go to the smaller one.
static inline EAGLE_HD long parentage_ordinal(long s_idx, long d_idx, long n_d) { return s_idx * (n_d > 0 ? n_d : 1) + d_idx; }

// ------------------------------------------------------------------------------------------------
// Epistasis (include/eagle_hip.h section 1b''''ii): the argument rule of eagle_epistasis_loci / eagle_epistasis_pairs, the balanced
// base-128 digits of the trait, t53 and the 128-bit rule of the statistic.  epi_stat is the ONE statement of the rule in C++: the tile
// kernel's epilogue (eagle_epi.hip) and the CPU test binary call it as is.
// ------------------------------------------------------------------------------------------------
#define EPI_MAX_N 65535L
#define EPI_YMAX 1000000
#define EPI_MAX_LOCI 64L
// What is wrong with the dims and the trait of a call, or NULL.  y may be NULL: not checked.
static inline const char* epi_arg_error(long n, long L, const int32_t* y) {
    if (n <= 0 || L <= 0) return "dims must be positive";
    if (L > 0x7fffffffL) return "2^31 markers or more";
    if (n > EPI_MAX_N) return "more than EAGLE_EPI_MAX_N = 65535 individuals";
    if (y)
        for (long k = 0; k < n; k++)
            if (y[k] > EPI_YMAX || y[k] < -EPI_YMAX) return "a trait value beyond EAGLE_EPI_YMAX = 1000000 in absolute value";
    return nullptr;
}
static inline const char* epi_loci_arg_error(long L, const long* loci, long nloci) {
    if (nloci < 1 || nloci > EPI_MAX_LOCI) return "the number of loci must be in [1, 64]";
    for (long k = 0; k < nloci; k++)
        if (loci[k] < 0 || loci[k] >= L) return "locus outside [0, L)";
    return nullptr;
}
static inline const char* epi_pairs_arg_error(long gap, double min_stat, long hit_cap, bool has_tables) {
    if (gap < 0) return "gap must not be negative";
    if (min_stat != min_stat) return "min_stat is NaN";
    if (hit_cap < 0) return "hit_cap must not be negative";
    if (hit_cap > 0 && !has_tables) return "hit_cap > 0 needs hit_ij, hit_stat and hit_mom";
    return nullptr;
}
// y = d0 + 128 d1 + 128^2 d2 with d in [-64, 63]: d_p = ((y_p + 64) & 127) - 64, y_{p+1} = (y_p - d_p) >> 7 (the difference is a multiple
// of 128, so the shift is exact).  Three digits hold [-64 * 16513, 63 * 16513] = [-1056832, 1040319], which contains every |y| <= 10^6;
// returns what is left of y behind them (0 there).
static inline EAGLE_HD int32_t epi_digits(int32_t y, int8_t d[3]) {
    for (int p = 0; p < 3; p++) {
        const int32_t dp = ((y + 64) & 127) - 64;
        d[p] = (int8_t)dp;
        y = (y - dp) >> 7;
    }
    return y;
}
typedef __int128 epi_i128;
// x truncated toward zero to its top 53 bits, as a double: |x| = m 2^sh + (the sh low bits dropped) with m < 2^53; both factors are
// exact in fp64 and so is their product (|x| < 2^127).
static inline EAGLE_HD double epi_t53(epi_i128 x) {
    const bool neg = x < 0;
    const unsigned __int128 m = neg ? (unsigned __int128)0 - (unsigned __int128)x : (unsigned __int128)x;
    const uint64_t hi = (uint64_t)(m >> 64), lo = (uint64_t)m;
    int bits = 0;
    if (hi) bits = 128 - __builtin_clzll(hi);
    else if (lo) bits = 64 - __builtin_clzll(lo);
    const int sh = bits > 53 ? bits - 53 : 0;
    const uint64_t top = (uint64_t)(m >> sh);
    const uint64_t pw = (uint64_t)(1023 + sh) << 52;           // 2^sh
    double p;
    memcpy(&p, &pw, sizeof p);
    const double v = (double)top * p;                           // exact
    return neg ? -v : v;
}
#if defined(__HIP_DEVICE_COMPILE__)
#define EPI_DIV(a, b) __ddiv_rn((a), (b))
#define EPI_MUL(a, b) __dmul_rn((a), (b))
#define EPI_SUB(a, b) __dadd_rn((a), -(b))
#else
#define EPI_DIV(a, b) ((a) / (b))
#define EPI_MUL(a, b) ((a) * (b))
#define EPI_SUB(a, b) ((a) - (b))
#endif
struct EpiTrait { long n; int64_t Y, T; };                     // n, sum y, sum y^2
struct EpiMarker { int64_t s, q, u; };                          // sum g, sum g^2, sum y g
// The statistic of one pair from its exact sums (rules 1 - 5 of the section): NaN where the pair is undefined.  S (may be NULL): Delta,
// Sxx, Sxy, Syy as computed, for the tests.  No product feeds a sum in the fp64 part, so nothing can contract into an FMA on the host.
static inline EAGLE_HD double epi_stat(const EpiTrait& t, const EpiMarker& a, const EpiMarker& b, int64_t d, int64_t e, int64_t f, int64_t h,
                                       int64_t z, epi_i128* S) {
    const int64_t n = t.n;
    const int64_t A00 = a.q * b.q - d * d, A01 = d * b.s - a.s * b.q, A02 = a.s * d - a.q * b.s;
    const int64_t A11 = n * b.q - b.s * b.s, A12 = a.s * b.s - n * d, A22 = n * a.q - a.s * a.s;
    const int64_t Delta = n * A00 + a.s * A01 + b.s * A02;
    const int64_t Ac0 = A00 * d + A01 * e + A02 * f, Ac1 = A01 * d + A11 * e + A12 * f, Ac2 = A02 * d + A12 * e + A22 * f;
    const epi_i128 cAc = (epi_i128)d * Ac0 + (epi_i128)e * Ac1 + (epi_i128)f * Ac2;
    const epi_i128 cAu = (epi_i128)t.Y * Ac0 + (epi_i128)a.u * Ac1 + (epi_i128)b.u * Ac2;
    const epi_i128 Au0 = (epi_i128)A00 * t.Y + (epi_i128)A01 * a.u + (epi_i128)A02 * b.u;
    const epi_i128 Au1 = (epi_i128)A01 * t.Y + (epi_i128)A11 * a.u + (epi_i128)A12 * b.u;
    const epi_i128 Au2 = (epi_i128)A02 * t.Y + (epi_i128)A12 * a.u + (epi_i128)A22 * b.u;
    const epi_i128 uAu = Au0 * t.Y + Au1 * a.u + Au2 * b.u;
    const epi_i128 Sxx = (epi_i128)Delta * h - cAc, Sxy = (epi_i128)Delta * z - cAu, Syy = (epi_i128)Delta * t.T - uAu;
    if (S) { S[0] = Delta; S[1] = Sxx; S[2] = Sxy; S[3] = Syy; }
    const uint64_t nanbits = 0x7ff8000000000000ull, infbits = 0x7ff0000000000000ull;
    double out;
    if (!(n > 4 && Delta > 0 && Sxx > 0)) { memcpy(&out, &nanbits, sizeof out); return out; }
    const double xy = epi_t53(Sxy);
    const double r2 = EPI_MUL(EPI_DIV(xy, epi_t53(Sxx)), EPI_DIV(xy, epi_t53(Syy)));
    if (!(r2 < 1.0)) { memcpy(&out, &infbits, sizeof out); return out; }
    return EPI_DIV(EPI_MUL((double)(n - 4), r2), EPI_SUB(1.0, r2));
}
// Whether the pair i < j is tested: not skipped by the gap rule.
static inline EAGLE_HD bool epi_pair_tested(long i, long j, const int32_t* chrom, long gap) {
    return !(j - i <= gap && (!chrom || chrom[i] == chrom[j]));
}

// ------------------------------------------------------------------------------------------------
// max(T) permutation testing (include/eagle_hip.h section 1b''''vi): the mixer and the sort key of the seeded permutations, the
// sign-magnitude base-128 digits of the trait, the check of an explicit permutation row and the argument rule of eagle_maxt.  The
// kernels of eagle_maxt.hip call the first three as they stand.
// ------------------------------------------------------------------------------------------------
#define MAXT_MAX_N 65535L
#define MAXT_TMAX 1000000
#define MAXT_RMAX 1024L
// h(seed, r, j): the top 32 bits of the splitmix64 finaliser of seed + (r 2^16 + j + 1) 0x9E3779B97F4A7C15 (mod 2^64)
static inline EAGLE_HD uint32_t maxt_mix(uint64_t seed, uint64_t r, uint64_t j) {
    uint64_t z = seed + ((r << 16) + j + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(z >> 32);
}
static inline EAGLE_HD uint64_t maxt_key64(uint64_t seed, uint64_t r, uint64_t j, uint32_t stratum) {
    return ((uint64_t)stratum << 48) | ((uint64_t)maxt_mix(seed, r, j) << 16) | j;
}
// t = sign(t) (m0 + 128 m1 + 16384 m2) with m in [0, 127]: digit p = sign(t) m_p lies in [-127, 127]; |t| <= 2,097,151
static inline EAGLE_HD void maxt_digits(int32_t t, int8_t d[3]) {
    const int32_t m = t < 0 ? -t : t, sg = t < 0 ? -1 : 1;
    d[0] = (int8_t)(sg * (m & 127));
    d[1] = (int8_t)(sg * ((m >> 7) & 127));
    d[2] = (int8_t)(sg * ((m >> 14) & 127));
}
// the planes a trait of largest magnitude tmax needs: 1 up to 127, 2 up to 16,383, else 3
static inline int maxt_planes(int64_t tmax) { return tmax <= 127 ? 1 : (tmax <= 16383 ? 2 : 3); }
// |d| = |N c - S T| <= 2 N^2 tmax: below 2^53 with N <= 65535 and tmax <= 10^6, so d converts to fp64 exactly
static inline bool maxt_bound_ok(int64_t N, int64_t tmax) { return 2.0 * (double)N * (double)N * (double)tmax < 9007199254740992.0; }
// whether row[0 .. N) is a permutation of 0 .. N - 1; seen: N bytes of scratch
static inline bool maxt_is_permutation(const int32_t* row, long N, uint8_t* seen) {
    memset(seen, 0, (size_t)N);
    for (long k = 0; k < N; k++) {
        if (row[k] < 0 || row[k] >= N || seen[row[k]]) return false;
        seen[row[k]] = 1;
    }
    return true;
}
// What is wrong with a call of eagle_maxt, or NULL; *N_out = the used individuals, *tmax_out = max |t| among them.
static inline const char* maxt_arg_error(long n, long L, const int32_t* t, const uint8_t* used, const int32_t* strata, long first, long R,
                                         const int32_t* perm, long* N_out, int64_t* tmax_out) {
    if (n <= 0 || L <= 0) return "dims must be positive";
    if (L > 0x7fffffffL) return "2^31 markers or more";
    if (n > MAXT_MAX_N) return "more than 65535 individuals";
    if (first < 1) return "first must be at least 1";
    if (R < 1 || R > MAXT_RMAX) return "R outside [1, EAGLE_MAXT_RMAX = 1024]";
    if (first + R > 2147483648L) return "first + R above 2^31";
    long N = 0, k0 = -1;
    int64_t tmax = 0;
    bool constant = true;
    for (long i = 0; i < n; i++) {
        if (used && !used[i]) continue;
        if (t[i] > MAXT_TMAX || t[i] < -MAXT_TMAX) return "a trait value beyond EAGLE_MAXT_TMAX = 1000000 in absolute value";
        if (!perm && strata && (strata[i] < 0 || strata[i] > 65535)) return "a stratum outside [0, 2^16)";
        if (k0 < 0) k0 = i;
        else if (t[i] != t[k0]) constant = false;
        tmax = std::max<int64_t>(tmax, t[i] < 0 ? -(int64_t)t[i] : t[i]);
        N++;
    }
    if (N < 3) return "fewer than 3 used individuals";
    if (constant) return "the trait is constant among the used individuals (W = 0)";
    if (perm) {
        std::vector<uint8_t> seen((size_t)N);
        for (long r = 0; r < R; r++)
            if (!maxt_is_permutation(perm + (size_t)r * (size_t)N, N, seen.data())) return "a row of perm is no permutation of 0 .. N - 1";
    }
    *N_out = N;
    *tmax_out = tmax;
    return nullptr;
}

// ------------------------------------------------------------------------------------------------
// Transmission disequilibrium test of trios (include/eagle_hip.h section 1b''''viii): the transmission words of rule 2 on the bit planes
// (shared with the kernels of eagle_tdt.hip), the family rule and the sign rule of the flips (rule 5) and the argument rule of
// eagle_tdt / eagle_bed_tdt.
// ------------------------------------------------------------------------------------------------
#define TDT_MAX_FLIP_TRIOS 65535L
// k: complete and free of a Mendel error; hf / hm: the informative het parents; pt / pu, mt / mu: the father / the mother passed A2 / A1;
// w: het x het -> het.  The arguments are the A, B and C words of the child, the father and the mother (an unknown parent: all zero).
struct TdtWords { uint64_t k, hf, hm, pt, pu, mt, mu, w; };
static inline EAGLE_HD TdtWords tdt_words(uint64_t ac, uint64_t bc, uint64_t cc, uint64_t af, uint64_t bf, uint64_t cf, uint64_t am, uint64_t bm,
                                          uint64_t cm) {
    TdtWords t;
    t.k = cc & cf & cm & ~mendel_error_word(ac, bc, cc, af, bf, am, bm);
    const uint64_t hc = cc & ~ac & ~bc;
    t.hf = cf & ~af & ~bf & t.k;
    t.hm = cm & ~am & ~bm & t.k;
    t.pt = t.hf & (bc | (hc & am));
    t.pu = t.hf & (ac | (hc & bm));
    t.mt = t.hm & (bc | (hc & af));
    t.mu = t.hm & (ac | (hc & bf));
    t.w = t.hf & t.hm & hc;
    return t;
}
// d of rule 2 at bit b of the four transmission words: PT + MT - PU - MU in [-2, 2]
static inline EAGLE_HD int tdt_d_bit(const TdtWords& t, int b) {
    return (int)((t.pt >> b) & 1ull) + (int)((t.mt >> b) & 1ull) - (int)((t.pu >> b) & 1ull) - (int)((t.mu >> b) & 1ull);
}
// The sign of family phi in flip r >= 1: -1 when bit 31 of h(seed, r, phi) is set (maxt_mix: counter = r 2^16 + phi + 1), else +1.
static inline EAGLE_HD int tdt_sign(uint64_t seed, uint64_t r, uint32_t phi) { return (maxt_mix(seed, r, phi) >> 31) ? -1 : 1; }
// The families of a trio list without family ids: the smallest list position with the same (father, mother), so full sibs flip together.
static inline void tdt_families(const int32_t* trios, long ntrios, int32_t* fam_out) {
    std::vector<std::pair<uint64_t, int32_t>> key((size_t)ntrios);
    for (long k = 0; k < ntrios; k++)
        key[(size_t)k] = {((uint64_t)(uint32_t)trios[3 * k + 1] << 32) | (uint32_t)trios[3 * k + 2], (int32_t)k};
    std::sort(key.begin(), key.end());                    // by couple, then by position: the first of a run is the smallest position
    for (size_t i = 0, first = 0; i < key.size(); i++) {
        if (key[i].first != key[first].first) first = i;
        fam_out[key[i].second] = key[first].second;
    }
}
// What is wrong with a call of eagle_tdt / eagle_bed_tdt over `markers` panel markers, or NULL.  family may be NULL.
static inline const char* tdt_arg_error(long markers, long ntrios, const int32_t* family, long first, long R) {
    if (markers > 0x7fffffffL) return "2^31 markers or more";
    if (R < 0) return "R must not be negative";
    if (ntrios < 1 || ntrios > MENDEL_MAX_TRIOS) return "the number of trios must be in [1, 2^27]";
    if (R == 0) return nullptr;
    if (ntrios > TDT_MAX_FLIP_TRIOS) return "more than 65535 trios with flips (R >= 1)";
    if (R > MAXT_RMAX) return "R outside [0, EAGLE_MAXT_RMAX = 1024]";
    if (first < 1) return "first must be at least 1";
    if (first + R > 2147483648L) return "first + R above 2^31";
    if (family)
        for (long k = 0; k < ntrios; k++)
            if (family[k] < 0 || family[k] > 65535) return "a family outside [0, 65535]";
    return nullptr;
}

// ------------------------------------------------------------------------------------------------
// VCF text in front of eagle_vcf_to_bed (include/eagle_hip.h section 1b-vcf): the line splitter of a staged window, the header line,
// the nine fixed fields of a data line and the verdict on them.  The sample fields are the device's (eagle_vcf.hip).
// ------------------------------------------------------------------------------------------------
#define VCF_A2_ALT 1
#define VCF_SNPS_ONLY 2
#define VCF_PASS_ONLY 4
#define VCF_FLAGS_ALL 7
// The line of buf[0, size) that starts at pos: [*b, *e) without its '\n' and without a '\r' in front of it; *next = where the following
// line starts.  A tail without '\n' is a line only when `last` (the buffer ends the file); else false: the line is not whole.
static inline bool vcf_next_line(const char* buf, size_t size, size_t pos, bool last, size_t* b, size_t* e, size_t* next) {
    if (pos >= size) return false;
    const char* q = (const char*)memchr(buf + pos, '\n', size - pos);
    if (!q && !last) return false;
    size_t end = q ? (size_t)(q - buf) : size;
    *next = q ? end + 1 : size;
    if (end > pos && buf[end - 1] == '\r') end--;
    *b = pos;
    *e = end;
    return true;
}
// Where the last whole line of buf[0, size) ends (the offset behind its '\n'), 0 when the buffer holds no '\n'.
static inline size_t vcf_whole_lines(const char* buf, size_t size) {
    for (size_t i = size; i > 0; i--)
        if (buf[i - 1] == '\n') return i;
    return 0;
}
struct VcfSpan { const char* p; long len; };
static inline bool vcf_span_is(const VcfSpan& s, const char* lit) { const size_t n = strlen(lit); return (size_t)s.len == n && memcmp(s.p, lit, n) == 0; }
// The first `want` tab-separated fields of [p, e) -> f[0 .. want); returns how many there are (at most `want`), and in *rest the byte
// behind the tab that ends field `want` - 1, or nullptr when the line ends with that field (or before it).
static inline int vcf_split_tabs(const char* p, const char* e, VcfSpan* f, int want, const char** rest) {
    int k = 0;
    *rest = nullptr;
    while (k < want) {
        const char* t = (const char*)memchr(p, '\t', (size_t)(e - p));
        f[k].p = p;
        f[k].len = (t ? t : e) - p;
        k++;
        if (!t) return k;
        p = t + 1;
    }
    *rest = p;
    return k;
}
// The #CHROM line [p, e) -> the sample names; nullptr, or what is wrong with it.
static inline const char* vcf_header_error(const char* p, const char* e, std::vector<VcfSpan>& names) {
    names.clear();
    VcfSpan f[9];
    const char* rest;
    if (e - p < 6 || memcmp(p, "#CHROM", 6) != 0) return "no #CHROM line in front of the data";
    if (vcf_split_tabs(p, e, f, 9, &rest) < 9 || !rest) return "the #CHROM line has fewer than 10 columns";
    while (rest) {
        VcfSpan s;
        const char* r2;
        vcf_split_tabs(rest, e, &s, 1, &r2);
        if (s.len == 0) return "an empty sample name";
        if (memchr(s.p, ' ', (size_t)s.len)) return "a sample name that contains a blank";
        names.push_back(s);
        rest = r2;
    }
    return nullptr;
}
enum VcfVerdict { VCF_KEEP = 0, VCF_MULTIALLELIC, VCF_NO_ALT, VCF_NO_GT, VCF_NOT_SNP, VCF_FILTERED };
static inline bool vcf_is_base(const VcfSpan& s) {
    if (s.len != 1) return false;
    const char c = (char)(s.p[0] & ~0x20);
    return c == 'A' || c == 'C' || c == 'G' || c == 'T';
}
// The verdict on a data line from its nine fixed fields (CHROM POS ID REF ALT QUAL FILTER INFO FORMAT), the first reason that holds.
static inline VcfVerdict vcf_verdict(const VcfSpan f[9], int flags) {
    const VcfSpan &ref = f[3], &alt = f[4], &filter = f[6], &format = f[8];
    if (memchr(alt.p, ',', (size_t)alt.len)) return VCF_MULTIALLELIC;
    if (vcf_span_is(alt, ".")) return VCF_NO_ALT;
    if (!(vcf_span_is(format, "GT") || (format.len >= 3 && memcmp(format.p, "GT:", 3) == 0))) return VCF_NO_GT;
    if ((flags & VCF_SNPS_ONLY) && !(vcf_is_base(ref) && vcf_is_base(alt))) return VCF_NOT_SNP;
    if ((flags & VCF_PASS_ONLY) && !(vcf_span_is(filter, "PASS") || vcf_span_is(filter, "."))) return VCF_FILTERED;
    return VCF_KEEP;
}
// Tab-separated fields of [p, e): the tabs + 1 (an empty range is one empty field).
static inline long vcf_count_fields(const char* p, const char* e) {
    long k = 1;
    while (p < e && (p = (const char*)memchr(p, '\t', (size_t)(e - p))) != nullptr) { k++; p++; }
    return k;
}
// Bytes a staging window of eagle_vcf_to_bed holds: chunk_bytes, or when that is 0 the staging rule of the eagle_bed_* calls (64 MiB, a
// quarter of max_memory_in_Gbytes if less); never below 4096.  vcf_line_fits: a window grows to a line only inside that quarter.
static inline long vcf_window_bytes(long chunk_bytes, double mem_gb) {
    if (chunk_bytes > 0) return chunk_bytes;
    double cap = 67108864.0;
    if (mem_gb > 0) cap = std::min(cap, mem_gb * 1e9 / 4.0);
    return std::max(4096L, (long)cap);
}
static inline bool vcf_line_fits(long line_bytes, double mem_gb) { return mem_gb <= 0 || (double)line_bytes <= mem_gb * 1e9 / 4.0; }
// Kept lines a window of `cap` text bytes can hold when every kept line carries n sample fields: a field and its separator are two bytes.
static inline long vcf_window_lines(long cap, long n) { return cap / (2 * n) + 1; }

// EAGLE_HIP_POISON (eagle_ctx.h, "The allocation path"): the fill byte its value names, or -1 = no fill.  A value is one to three
// decimal digits that make a number in 0 .. 255 and nothing else; unset, empty, out of range or anything with another character in it
// leaves the hook off (a test hook that half understands its value would fill with a byte nobody asked for).
static inline int poison_parse(const char* e) {
    if (!e || !e[0]) return -1;
    int v = 0, k = 0;
    for (; e[k]; k++) {
        if (e[k] < '0' || e[k] > '9' || k >= 3) return -1;
        v = 10 * v + (e[k] - '0');
    }
    return v <= 255 ? v : -1;
}
#endif
