// eagle_ctx.h -- the context object and small host helpers shared by eagle_api.cpp, eagle_load.cpp and eagle_ingest.cpp
// (private to libeaglehip.so; the public ABI only sees the opaque eagle_ctx*).
#ifndef EAGLE_CTX_H
#define EAGLE_CTX_H
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/types.h>
#include <time.h>

#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/eagle_hip.h"
#include "eagle_internal.h"
#include "eagle_host.h"
#include "eagle_w8.h"

struct GenoEntry {
    std::string path;
    off_t size = 0;
    long mtime_ns = 0;
    long rows = 0, cols = 0;          // logical tile held: `rows` lines from line row0, `cols` characters from character col0
    long row0 = 0, col0 = 0;          // (0, 0) and the whole file for a single-device ctx; a marker shard in a multi-device one
    long rows_pad = 0, ld = 0;
    int8_t* dev = nullptr;
    int8_t* dev_s = nullptr;    // re-centred image m - c_i (eagle_dev_marker_shift), made on the first digit-slice scan of the file
    int8_t* cshift = nullptr;   // c_i per row
    int32_t* l1 = nullptr;      // {sum_j |m_ij - c_i|, sum_j (m_ij - c_i)^2} per row (error bounds of the digit-slice scan)
    void* dev_f4 = nullptr;     // fp4 image of `dev` (two genotypes per byte): operand of the MM^T kernel, made by the first calculateMMt on the file
};

// A VIEW alias of eagle_reshape_m: the file ReshapeM_rcpp would write, served from the source file (or its resident image)
// through a keep-map.  axis 0: the lines of M.ascii (individuals), axis 1: the characters of every line of Mt.ascii.
struct ViewAlias {
    std::string alias, src;
    off_t src_size = 0;
    long src_mtime_ns = 0;
    int axis = 0;
    std::vector<int32_t> keep;        // source line (axis 0) / character (axis 1) of every line / character of the alias, increasing
    long lines = 0;                   // lines of the alias
    mutable int32_t* d_keep = nullptr;   // the keep-map in HBM (axis 1; made on first use)
};

// The one owner of the cached S (the rule: s_plan in eagle_host.h; the methods: eagle_api.cpp, "The cached S").  A scan calls acquire, then
// begin_verify behind W, settle where the plan says, commit when it has gone through; leave() on every way out.
struct SCache {
    double* d_S = nullptr; double* d_scr = nullptr;   // device copy of the last call's S and the scratch the caller's is compared in (np x np each)
    long dev_n = 0, dev_np = 0;                       // ... holding an n-individual S (0: none) / allocated for np (0: not)
    double* h_S = nullptr; long h_n = 0; size_t h_cap = 0;   // host copy (n x n as the caller passed it) for the memcmp; h_n = 0: none
    SSlot slot;                                       // above max_np: where the last scan left S in the arena
    int* h_flag = nullptr;                            // 64 pinned bytes: where the device comparison's flag lands
    long hits = 0, misses = 0;                        // (eagle_scan_operand_cache_stats)
    unsigned long s_gen = 0;                          // the number of the content where a call's S lies (eagle_ctx::w8_s_gen_next; w8_keep_valid)
    // this call
    SPlan plan;
    std::thread helper; int helper_rc = 0;            // issues a deferred device comparison, or runs the host comparison / the refresh of the host copy
    bool pending = false;                             // something was started that settle() has to collect
    int host_differs = 0;
    int acquire(eagle_ctx* ctx, const SCall& call, const SPolicy& pol, const double* S_host, double* slot_S, double** Sa);
    int begin_verify(eagle_ctx* ctx, const double* S_host, long n, long np);
    int settle(eagle_ctx* ctx, int rc, SOutcome* out);
    void commit(const eagle_ctx* ctx, const double* slot_S, long n, long np);
    void leave();
    void forget_host();
    void release();
};

// The kernel-form switch of a context (eagle_ctx::tune; eagle_dev_set_tune, EAGLE_HIP_TUNE): which of several forms of the same
// computation the launch code picks.  Every form gives the same bits; the values other than the default exist for the tests and tools
// that compare two forms.  The predicates below the context are the only code that reads the switch.  (_lib.TUNE mirrors the list.)
enum EagleTune {
    TUNE_SHIPPED = 0,             // the shipped form of everything
    TUNE_VARA_256 = 8,            // scan: k_vara_i8 (256 x 256 tile) at any size
    TUNE_COMPILER_SCHEDULED = 9,  // scan: k_vara_i8w below 32,768 padded individuals (k_vara_i8 from there up); MM^T: k_syrk_f4
    TUNE_SYRK_F4P = 10,           // MM^T: k_syrk_f4p (256 x 256 tile, pipelined k-step) at any size
    TUNE_SYRK_F4W = 11,           // MM^T: k_syrk_f4w (384 x 256 tile) below 3,072 padded individuals too
    TUNE_VARA_PACED = 14,         // scan: the paced k_vara_i8p<true> at any size
    TUNE_SPECTRAL_OFF = 29,       // scan prepare: no digit saved under the spectral bound
    TUNE_W8_UNPIPED = 31,         // W engine: the product on the compiler-scheduled 256 x 256 k_w8_gemm
    TUNE_W8_ROWPASS_SPLIT = 32,   // W engine: row statistics and digit slices as two kernels (k_w8_rowstats, k_w8_slice)
    TUNE_GRAM_TWICE = 33,         // scan prepare: k_gram_hi_i8 forms the last digit's Gram a second time
    TUNE_VARA_UPPER = 34,         // scan: the upper image of W's digits, every tile from stage 0
};
// v if the enum names it, else the default: a number of a form that has left the library selects the shipped forms
static inline int tune_known(int v) {
    switch (v) {
        case TUNE_VARA_256: case TUNE_COMPILER_SCHEDULED: case TUNE_SYRK_F4P: case TUNE_SYRK_F4W: case TUNE_VARA_PACED: case TUNE_SPECTRAL_OFF:
        case TUNE_W8_UNPIPED: case TUNE_W8_ROWPASS_SPLIT: case TUNE_GRAM_TWICE: case TUNE_VARA_UPPER:
            return v;
        default: return TUNE_SHIPPED;
    }
}

struct eagle_ctx {
    int device = -1;
    // multi-device: the ctx eagle_open_devices returns is the LEAD (first device); it owns one sub-context per further device.
    std::vector<eagle_ctx*> peers;
    eagle_ctx* lead = nullptr;           // set in sub-contexts
    double* d_Z = nullptr; long z_L = 0, z_n = 0, z_first = 0; long spectral_L = 0;  // Z = Mt U of the opt-in spectral scan (eagle_spectral.hip), L_pad x n_pad fp64
    void* blas_handle = nullptr;         // rocblas_handle of the opt-in device model algebra (eagle_linalg.cpp)
    void* rccl = nullptr;                // RcclState* of the lead (communicators, one per device), or NULL: host-staged sums
    long scan_first = 0;                 // global index of the first marker of this device's last scan
    int32_t* d_c32 = nullptr; size_t c32_cap = 0;      // partial MM^T accumulator (grow-only, kept between calls)
    int32_t* d_pack = nullptr; size_t pack_cap = 0;    // packed upper tiles of it (multi-device sum)
    int32_t* d_pack2 = nullptr; size_t pack2_cap = 0;  // lead: landing buffer of a peer's packed tiles (host-staged sum)
    hipStream_t stream = nullptr;
    hipStream_t load_stream = nullptr;  // tile loads of the streamed (out-of-core) paths run here, under the kernels of `stream`
    char err[1024] = {0};
    eagle_message_fn msg_fn = nullptr;
    void* msg_user = nullptr;
    int scan_mode = 1;   // 1 = int8 digit slices on the int8 MFMA (default), 0 = fp64 MFMA
    int scan_slices = 0; // 0 = chosen per call from the error bound (3..7), 1..8 = fixed
    int scan_stochastic = 0;  // 1 = digits of W rounded at random (unbiased): probabilistic certificate, one digit fewer (opt-in)
    double scan_budget = 5e-7;  // relative digit budget of the int8 scan (eagle_set_scan_budget): half of the path's 1e-6 tolerance
    double scan_budget_tight = 1e-7;  // tried first (round 4): the budget in force is this one whenever the digits that run certify it too; eagle_set_scan_budget sets both
    double scan_budget_enforced = 0.0; long cert_over_tight = 0;   // (eagle_last_scan_enforced)
    double scan_budget_used = 0.0; int scan_bound_level = 0; double scan_w_err = 0.0;   // of the last digit-slice scan (eagle_last_scan_budget)
    bool spectral_off = false;  // a scan that took a digit off under the spectral bound fell back to fp64: this context stops trying
    std::vector<GenoEntry> cache;
    std::vector<ViewAlias> views;        // eagle_reshape_m(..., EAGLE_RESHAPE_VIEW, ...) aliases of this device
    long view_loads[4] = {0, 0, 0, 0};   // view windows loaded, by source (EAGLE_VIEW_RESIDENT ... in eagle_hip.h; eagle_view_load_counts)
    // results of the last calls, kept in HBM
    double* d_mmt = nullptr; long mmt_n = 0; double* d_mmt_max = nullptr;
    double* d_a = nullptr; double* d_vara = nullptr; long scan_L = 0; long scan_cap = 0;
    double* d_bound = nullptr;  // a-posteriori error bound of every vara_i of the last digit-slice scan that ran in marker blocks / device shards
    long cert_reevaluated = 0, cert_flagged = 0; int cert_fell_back = 0;  // certification counters of the last digit-slice scan
    int scan_digits_used = 0, scan_digits_cut = 0; double scan_specH = 0.0;  // digit slices of the last digit-slice scan (eagle_last_scan_digits)
    double scan_phase_ms[8] = {0}; long scan_blocks = 0;                  // phase clock of the last scan on this device (eagle_last_scan_timing)
    double scan_host_setup_s = 0, scan_range_wall_s = 0, scan_call_wall_s = 0;
    SCache scache;   // S = inv_MMt_sqrt of the last scan, kept for the next one (below)
    // out-of-core bookkeeping of the last streamed call on this device (eagle_last_stream_stats)
    long st_chunks = 0, st_file_bytes = 0;
    double st_pread_s = 0, st_load_wall_s = 0, st_wait_s = 0, st_compute_s = 0, st_total_s = 0, st_starved_s = 0, st_load_first_s = 0;
    void* d_scratch = nullptr;
    void* argmax_ws = nullptr;   // block partials + result of eagle_last_scan_argmax (ctx-owned: no allocation per call)
    void* arena = nullptr; size_t arena_cap = 0, arena_off = 0;  // grow-only device workspace reused across calls
    unsigned long arena_gen = 1;      // counts every allocation, release or replacement of the arena (what SCache's slot is valid by)
    void* arena_prefetch = nullptr;   // ArenaPrefetch* (eagle_api.cpp): a background hipMalloc of the arena in flight
    void* f4_buf = nullptr; size_t f4_cap = 0;  // fp4 image of the tile eagle_dev_mmt_accumulate is working on
    void* gemm_scratch = nullptr; size_t gemm_scratch_cap = 0;  // split-K partial tiles of the fp64 GEMM's last wave
    void* gemv_ws = nullptr;  // 16 digit-slice rows of the GEMV vectors + their exponents (k_gemv_mfma)
    void* stage_pin[2] = {nullptr, nullptr}; void* stage_raw[2] = {nullptr, nullptr}; size_t stage_cap = 0;  // tile streamer
    // per-device launch state (a process may hold one ctx per GPU): dynamic-LDS attributes set on this device, the kernel-form
    // switch (an EagleTune; written through tune_known only)
    bool attr_vara[7] = {false, false, false, false, false, false, false};   // by VaraKernel
    bool attr_syrk_f4w = false, attr_zbuild_i8 = false, attr_vara_f6 = false, attr_gemv = false, attr_gemv2 = false, attr_w8_gemm = false, attr_knn_rows = false, attr_knn_rows_dist = false, attr_ldknn = false;
    uint32_t attr_bedld = 0;   // k_bedld_tile<NB, R2>: bit 2 (NB - 2) + R2
    int tune = TUNE_SHIPPED;
    // W = S (V S) on the int8 engine (eagle_w8.hip): workspace, and what the last call left for the scan that follows it
    int w_mode = 1;            // 0 = always the fp64 GEMM, 1 = int8 digit slices from 4,096 padded individuals up, 2 = int8 at any size (tests)
    void* w8_ws = nullptr; size_t w8_ws_cap = 0; void* w8_host = nullptr;
    bool w8_active = false;    // Wu of the last scan_operands call came from the int8 engine:
    double w8_eta = 0.0;       //   || folded image - truth ||_F <= w8_eta (the per-marker certificate adds w8_eta sum_j m'_j^2)
    const double* w8_r = nullptr;   //   r = S (V (S 1)) in fp64 (the correction vector of the re-centred markers comes from it)
    const double* w8_Wu = nullptr; const double* w8_Sa = nullptr; const double* w8_Va = nullptr; long w8_n = 0;   //   the image it describes, and the operands
    double* w8_tmp = nullptr; void* w8_true_ws = nullptr; size_t w8_true_cap = 0;
    W8Info w8_info;
    void* w8_pipe = nullptr;            // W8Pipe* (eagle_w8.hip): the state between eagle_w8_begin / _vrows / _finish
    int w8_guess_c1 = -1; long w8_guess_np = 0;   // the first product's configuration of the last call: what a pipelined call starts on
    // what is kept with S between calls (w8_keep_valid, eagle_host.h): the record, the workspace's generation, the caller's declaration
    // (eagle_dev_declare_s), the counter new S contents take their number from, and how often a call reused / recomputed the S products
    W8Keep w8_keep; unsigned long w8_ws_gen = 0; W8Declared w8_declared; unsigned long w8_s_gen_next = 1;
    long w8_keep_hits = 0, w8_keep_misses = 0;
    size_t attr_w8_rowpass = 0;     // dynamic LDS k_w8_rowpass has been allowed on this device
    bool w8_maxabs_ready = false;   // the w8 workspace holds max |off-diagonal| of the Wu eagle_w8_finish just made (k_w8_combine2)
    const unsigned long long* w8_maxabs = nullptr;
    char arch[64] = {0};
    int cu_count = 0;
    int64_t hbm_bytes = 0;
};

// Not a value of the switch (its list of names is closed): EAGLE_HIP_STAGE_GLUE=1 in the environment, read at every launch as the other
// test hooks are, runs k_vara_i8p and k_w8_gemm_p in the form before the engine's stage step (eagle_t8.h) -- the DMA state and the read
// addresses re-derived in C++ between the k-steps of every stage.  Same bits; A/B runs and tests/test_gpu_stage_step.py.
static inline bool stage_glue_form() { const char* e = getenv("EAGLE_HIP_STAGE_GLUE"); return e && atoi(e) != 0; }
// ---- what the switch decides: one predicate per question the launch code asks ----
// The digit-slice scan (eagle_i8mfma.hip): its kernel, and with it the layout of W's digits, the image orientation and the pacing.
// Decided by this one function at prepare (layout, orientation) and at launch; `ext`: the compact image of the digit extension.
//   the pipelined 384 x 256 k_vara_i8p below 65,536 padded individuals (above: the int32 range of its tile row-dots), unless the switch
//   asks for k_vara_i8 or k_vara_i8w; the lower image (each column tile from its diagonal block down to the last live stage of W,
//   DESIGN 4.3) unless it asks for the upper one; paced workers from 32,768 padded individuals up -- under TUNE_SHIPPED and
//   TUNE_VARA_UPPER only: every other value leaves the pacing off at any size (known behaviour of the A/B values)
enum VaraKernel { VARA_I8 = 0, VARA_I8W, VARA_I8P, VARA_I8P_PACED, VARA_I8P_EXT,   // k_vara_i8, k_vara_i8w, k_vara_i8p<false>, <true>, <false, true>
                  VARA_I8P_GLUE, VARA_I8P_EXT_GLUE };                                // k_vara_i8p<false, false, true>, <false, true, true> (stage_glue_form)
struct VaraForm {
    VaraKernel kernel;
    bool lower;                                       // the lower image and its walk (k_vara_i8p only)
    bool piped() const { return kernel >= VARA_I8P; } // k_slice_w lays the digits out for the 384 x 256 pipelined kernel
};
static inline VaraForm vara_form(const eagle_ctx* ctx, long n_pad, bool ext) {
    const int t = ctx->tune;
    if (t == TUNE_VARA_256 || t == TUNE_COMPILER_SCHEDULED || n_pad >= 65536)
        return {t == TUNE_COMPILER_SCHEDULED && n_pad < 32768 ? VARA_I8W : VARA_I8, false};
    const bool paced = !ext && (t == TUNE_VARA_PACED || ((t == TUNE_SHIPPED || t == TUNE_VARA_UPPER) && n_pad >= 32768));
    if (stage_glue_form()) return {ext ? VARA_I8P_EXT_GLUE : VARA_I8P_GLUE, true};   // (unpaced, lower image)
    return {paced ? VARA_I8P_PACED : (ext ? VARA_I8P_EXT : VARA_I8P), t != TUNE_VARA_UPPER};
}
// MM^T on fp4 operands: the 384 x 256 k_syrk_f4w from 3,072 padded individuals up while its row offsets fit (`wide_fits`), below
// that the 256 x 256 k_syrk_f4p (the wide tiles pad too much there and leave too few workgroups)
enum MmtKernel { MMT_F4, MMT_F4P, MMT_F4W };
static inline MmtKernel tune_mmt_kernel(const eagle_ctx* ctx, long n_pad, bool wide_fits) {
    const int t = ctx->tune;
    if (t == TUNE_COMPILER_SCHEDULED) return MMT_F4;
    if (t == TUNE_SYRK_F4P) return MMT_F4P;
    return (n_pad >= 3072 || t == TUNE_SYRK_F4W) && wide_fits ? MMT_F4W : MMT_F4P;
}
static inline bool tune_w8_piped(const eagle_ctx* ctx) { return ctx->tune != TUNE_W8_UNPIPED; }              // k_w8_gemm_p (while it fits)
static inline bool tune_w8_rowpass_once(const eagle_ctx* ctx) { return ctx->tune != TUNE_W8_ROWPASS_SPLIT; }  // k_w8_rowpass (while a row fits LDS)
static inline bool tune_spectral_allowed(const eagle_ctx* ctx) { return ctx->tune != TUNE_SPECTRAL_OFF; }
static inline bool tune_gram_once(const eagle_ctx* ctx) { return ctx->tune != TUNE_GRAM_TWICE; }

extern thread_local char g_open_err[512];
static inline int host_threads() { unsigned h = std::thread::hardware_concurrency(); return h == 0 ? 1 : (h > 16 ? 16 : (int)h); }

static inline int failf(eagle_ctx* ctx, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    if (ctx) vsnprintf(ctx->err, sizeof ctx->err, fmt, ap);
    va_end(ap);
    return code;
}
static inline void say(eagle_ctx* ctx, const char* fmt, ...) {
    if (!ctx->msg_fn) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    ctx->msg_fn(buf, ctx->msg_user);
}

#define HIPCHK(ctx, call)                                              \
    do {                                                               \
        hipError_t e__ = (call);                                       \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, #call); \
    } while (0)

// ---- The allocation path ----
// Every device and pinned allocation of the library is made by the two functions below, and nowhere else (tests/test_poison_host.py
// holds the sources to that).  EAGLE_HIP_POISON=<0..255> in the environment, read at every allocation as the other test hooks are,
// fills what they return with that byte; dev_scratch_handout / pin_scratch_handout do the same where a buffer the context keeps is handed
// out again as scratch without a new allocation (which buffers are scratch, which are state and never filled).  The fill
// waits for the device before and behind it -- the buffer may still be read by work in flight on either stream, and is written next on
// any of them.  Unset: one getenv per allocation and nothing else.
static inline int poison_byte() { return poison_parse(getenv("EAGLE_HIP_POISON")); }
static inline hipError_t dev_poison(void* p, size_t bytes, int byte) {
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemset(p, byte, bytes);
    return e == hipSuccess ? hipDeviceSynchronize() : e;
}
static inline hipError_t dev_alloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    const int byte = poison_byte();
    if (e != hipSuccess || byte < 0 || !bytes) return e;
    const hipError_t ef = dev_poison(*p, bytes, byte);
    if (ef != hipSuccess) { (void)hipFree(*p); *p = nullptr; }   // a block that could not be filled is no allocation: the callers treat it as failed
    return ef;
}
template <class T> static inline hipError_t dev_alloc(T** p, size_t bytes) { return dev_alloc((void**)p, bytes); }
static inline hipError_t pin_alloc(void** p, size_t bytes) {
    const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    const int byte = poison_byte();
    if (e == hipSuccess && byte >= 0) memset(*p, byte, bytes);
    return e;
}
template <class T> static inline hipError_t pin_alloc(T** p, size_t bytes) { return pin_alloc((void**)p, bytes); }
// `bytes` of a kept buffer about to be used as scratch again (no-ops with the hook unset, or p null)
static inline hipError_t dev_scratch_handout(void* p, size_t bytes) {
    const int byte = poison_byte();
    return byte >= 0 && p && bytes ? dev_poison(p, bytes, byte) : hipSuccess;
}
// A sub-region of the context's scratch page as its user takes it (EAGLE_SCR_*, eagle_host.h: every region runs to the next one)
static inline void* scr_take(eagle_ctx* ctx, size_t off) {
    static const size_t at[] = {EAGLE_SCR_SYM, EAGLE_SCR_CERT_TOTALS, EAGLE_SCR_INGEST, EAGLE_SCR_LOADER_BAD, EAGLE_SCR_SCACHE_FLAG,
                                EAGLE_SCR_DOT_PARTIALS, EAGLE_SCR_BYTES};
    void* p = (char*)ctx->d_scratch + off;
    for (int k = 0; k < 6; k++) if (at[k] == off) (void)dev_scratch_handout(p, at[k + 1] - off);
    return p;
}
static inline void pin_scratch_handout(void* p, size_t bytes) {
    const int byte = poison_byte();
    if (byte >= 0 && p && bytes && hipDeviceSynchronize() == hipSuccess) memset(p, byte, bytes);
}

// RAII device / pinned buffers so every error path frees what it took
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return dev_alloc(&p, bytes ? bytes : 16); }
    template <class T> T* as() { return (T*)p; }
};
struct PinBuf {
    void* p = nullptr;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t bytes) { return pin_alloc(&p, bytes ? bytes : 16); }
};
// the two events of a double-buffered pipeline: e[b] is recorded behind the last stream work that touches buffer b
struct EventPair {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~EventPair() { for (int b = 0; b < 2; b++) if (e[b]) (void)hipEventDestroy(e[b]); }
    hipError_t create() {
        hipError_t r = hipEventCreateWithFlags(&e[0], hipEventDisableTiming);
        return r != hipSuccess ? r : hipEventCreateWithFlags(&e[1], hipEventDisableTiming);
    }
};

// Registers a device image (rows_pad x ld int8, zero padded) as the resident copy of the text file at `path`
// (rows lines x cols characters); takes ownership of `dev`.  Stale entries of the same path are dropped.
int eagle_cache_adopt(eagle_ctx* ctx, const char* path, long rows, long cols, long rows_pad, long ld, int8_t* dev);
// Resident copy of a file if the cache holds one that matches the file's current size and mtime, else nullptr.
const GenoEntry* eagle_cache_find(eagle_ctx* ctx, const char* path, long rows, long cols);
int eagle_stage_ensure(eagle_ctx* ctx, size_t need);

// 2-bit sidecar "<text file>.e2b": 64-byte header + rows x row_bytes packed genotype codes.  It is only trusted while
// the text file it was made from still has the recorded size and mtime.
struct E2bHeader {
    char magic[8];        // "EAGLE2B\0"
    uint32_t version;     // 1
    uint32_t reserved;
    uint64_t rows, cols, row_bytes;
    uint64_t src_size;
    int64_t src_mtime_ns;
    uint64_t pad;
};
static_assert(sizeof(E2bHeader) == 64, "E2bHeader is the 64-byte file header");
extern "C" int eagle_dev_pack2b(eagle_ctx* ctx, const int8_t* in, long rows, long cols, long ld_in, uint8_t* out, long row_bytes, void* stream);
extern "C" int eagle_dev_unpack2b(eagle_ctx* ctx, const uint8_t* raw, long rows, long cols, long stride, int shift, int8_t* out,
                                  long ld_out, int* bad_dev, void* stream);
// `real` SNP-major .bed rows of ceil(n/4) bytes -> int8 tile (rows x ld, zero beyond real / n), sidecar rows at stride rb16 (or
// null) and the count of missing genotypes added to *n_missing (or null); k_bed_decode in eagle_kernels.hip.
extern "C" int eagle_dev_bed_decode(eagle_ctx* ctx, const uint8_t* bed, long real, long rows, long n, int8_t* tile, long ld, uint8_t* packed,
                                    long rb16, unsigned long long* n_missing, void* stream);
// Marker QC (eagle_qc.hip): per-marker genotype counts of an int8 Mt tile (counts[rows][3] = n0, n1, n2) and of raw SNP-major .bed rows
// (counts[rows][4] = hom A1, het, hom A2, missing), and the rows map[0 .. nrows) of an image copied to consecutive rows of `out`
// (zero rows up to rows_out).
extern "C" int eagle_dev_marker_counts(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, int32_t* counts, void* stream);
extern "C" int eagle_dev_bed_marker_counts(eagle_ctx* ctx, const uint8_t* bed, long rows, long n, int32_t* counts, void* stream);
// VCF sample fields (eagle_vcf.hip; include/eagle_hip.h section 1b-vcf), device pointers throughout.  text: a staged window, readable up to the
// next multiple of 16 behind the largest table entry; table[lines][2] = [beg, end) of every kept line from its first sample field;
// codes[lines][n]: one .bed code per byte; cnt[lines][4] = (fields found, missing, haploid, malformed); bed[lines][ceil(n/4)].
extern "C" int eagle_dev_vcf_fields(eagle_ctx* ctx, const uint8_t* text, const int64_t* table, long lines, long n, int a2_alt, uint8_t* codes,
                                    int32_t* cnt, void* stream);
extern "C" int eagle_dev_vcf_pack(eagle_ctx* ctx, const uint8_t* codes, long lines, long n, uint8_t* bed, void* stream);
extern "C" int eagle_dev_gather_rows_i8(eagle_ctx* ctx, const int8_t* src, long ld_src, const int32_t* map, long nrows, long rows_out,
                                        int8_t* out, long ld_out, void* stream);
// Per-group counts (eagle_groups.hip; include/eagle_hip.h section 1b''''iii), device pointers throughout.  labels[n] in [-1, K) (the CALLER's
// check), sizes[K] = the individuals per group.  onehot: 64 x ld int8, byte (k, i) = 1 iff labels[i] == k; counts[rows][K][3] = (n0, n1,
// n2) of an int8 Mt tile per group.  planes: K x ceil(ceil(n/4) / 4) dwords, bit 2q of byte b of plane k set iff individual 4b + q is in
// group k; counts[rows][K][4] = (hom A1, het, hom A2, missing) of raw .bed rows per group.  p[L] = Fisher's exact test of tables[L][4].
extern "C" int eagle_dev_group_onehot(eagle_ctx* ctx, const int32_t* labels, long n, int8_t* onehot, long ld, void* stream);
extern "C" int eagle_dev_group_counts(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, const int8_t* onehot, long ld_onehot, int K,
                                      const int32_t* sizes, int32_t* counts, void* stream);
extern "C" int eagle_dev_group_bedmask(eagle_ctx* ctx, const int32_t* labels, long n, int K, uint32_t* planes, void* stream);
extern "C" int eagle_dev_bed_group_counts(eagle_ctx* ctx, const uint8_t* bed, long rows, long n, int K, const uint32_t* planes, const int32_t* sizes,
                                          int32_t* counts, void* stream);
extern "C" int eagle_dev_fisher_2x2(eagle_ctx* ctx, const int32_t* tables, long L, double* p, void* stream);
// max(T) permutation testing (eagle_maxt.hip; include/eagle_hip.h section 1b''''vi), device pointers throughout.  keys: nr x NP2 uint64,
// NP2 = the power of two >= N, sorted per row on return (the low 16 bits of a row = pi).  op: int8 [P][Rtot][ld], rows r0 .. r0 + nr
// written from the sorted keys, an int32 table perm[nr][N], or the identity (both NULL); rank[n] = position of an individual or -1, tu[N]
// = the trait of the used individuals.  counts[rows][1][3] of the `used` group -> S, V.  The tile: obs = 1 writes dobs / keyobs from the
// one-arrangement operand of the trait itself, obs = 0 reads dobs, adds to count1 and writes one (key, marker) partial per tile and
// permutation at tile_base + tile; S, V, dobs, keyobs, count1 start at the window's first row, row_base = that row's marker index.
extern "C" int eagle_dev_maxt_permutations(eagle_ctx* ctx, uint64_t seed, long r_first, long nr, long N, long NP2, const uint16_t* strata_u,
                                           uint64_t* keys, void* stream);
extern "C" int eagle_dev_maxt_operand(eagle_ctx* ctx, const uint64_t* keys, long NP2, const int32_t* perm, long N, const int32_t* rank,
                                      const int32_t* tu, long n, long ld, int P, long Rtot, long r0, long nr, int8_t* op, void* stream);
extern "C" int eagle_dev_maxt_sv(eagle_ctx* ctx, const int32_t* counts, long rows, long N, int32_t* S, int64_t* V, void* stream);
extern "C" int eagle_dev_maxt_width(int P);
extern "C" int eagle_dev_maxt_tile(eagle_ctx* ctx, int obs, const int8_t* Mt8, long rows, long n, long ld, const int8_t* op, long ldop, int P, long R,
                                   long Rstride, long N, long T, const int32_t* S, const int64_t* V, int64_t* dobs, double* keyobs, int32_t* count1,
                                   double* pkey, int32_t* parg, long tile_base, long row_base, void* stream);
extern "C" int eagle_dev_maxt_finish(eagle_ctx* ctx, const double* pkey, const int32_t* parg, long ntiles, long R, double* maxkey, int32_t* argmax,
                                     void* stream);
// Logistic regression per marker (eagle_logit.hip; include/eagle_hip.h section 1b''''iv), device pointers throughout, one row window.
// X16: n64 x 16 fp64, n64 = n rounded up to 64, row i = the c = p - 1 covariates of individual i then zeros; valid_y: n64 bytes, 0 = not
// used, 2 = control, 3 = case; both zero from individual n on, and the X16 rows of unused individuals zero.  beta0[c]: the start.
// stat[rows][4] = (gamma, se, score, loglik), info[rows][2] = (code, evaluations); firth = 0 (ML), 1 (Firth), 2 (fallback).
extern "C" int eagle_dev_logistic(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, const double* X16, const uint8_t* valid_y,
                                  const double* beta0, int p, int firth, double tol, int max_iter, double* stat, int32_t* info, void* stream);
// Saddlepoint deviates of the score test under the logistic mixed model (eagle_glmm.hip; include/eagle_hip.h section 1d'''), device
// pointers throughout, one row window.  X16: n64 x 16 fp64 as eagle_dev_logistic takes it; P4: n64 x 4 fp64 = (mu, 1 - mu, mu (1 - mu),
// y - mu) per individual and (1/2, 1/2, 0, 0) from individual n on; A16: 16 x 16 fp64 = (X'DX)^-1, zero outside c x c; vara: rows fp64
// or NULL.  stat[rows][7] = (T, V*, z, zeta_up, r*_up, zeta_lo, r*_lo), info[rows][2] = (code, evaluations).
extern "C" int eagle_dev_glmm_spa(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, const double* X16, const double* P4,
                                  const double* A16, int c, const double* vara, double cutoff, double tol, int max_iter, double* stat, int32_t* info,
                                  void* stream);
// One EM step of the admixture model (eagle_admix.hip; include/eagle_hip.h section 1b''''v), device pointers throughout.  Q16: n16 x 16
// and Fin / Fout: L16 x 16 fp64 (n16, L16 = n, L rounded up to 16), columns >= K and the rows beyond n / L zero.  _window: the rows
// [row0, row0 + rows) of the image, row0 a multiple of 16 and rows one too unless the window ends the panel; llpart[L16 / 16] takes the
// likelihood of every 16-marker tile, and with update Fout the new frequencies of the window's markers and part[S][n16][16] the Q
// accumulators of the ranges of admix_range_plan (eagle_host.h).  _finish, once per pass: *ll_out = the sum of llpart, and with update
// Qout = the new fractions.
extern "C" int eagle_dev_admix_window(eagle_ctx* ctx, const int8_t* Mt8, long row0, long rows, long n, long L, long ld, int K, int update,
                                      const double* Q16, const double* Fin, double* Fout, double* llpart, double* part, int S, long range_len,
                                      void* stream);
extern "C" int eagle_dev_admix_finish(eagle_ctx* ctx, long n, long L, int K, int update, const double* llpart, double* ll_out, const double* part,
                                      int S, const double* Qin, double* Qout, void* stream);
// The exact mixed-model test per marker (include/eagle_hip.h section 1d').  eagle_lmm.hip: rows of Z (ldz fp64 each, ldz >= n64) against the
// staged image B16 (n64 x 16 fp64: U^T X, a zero column for z, U^T y) and lam64 (n64, +inf from n on), n64 = n rounded up to 64; idx:
// count device longs or NULL = rows 0 .. count - 1  ->  stat[count][5], info[count][2].
extern "C" int eagle_dev_lmm(eagle_ctx* ctx, const double* Z, long ldz, const double* B16, const double* lam64, long n, int c, int reml,
                             double theta0, double tol, int max_iter, const long* idx, long count, double* stat, int32_t* info, void* stream);
// Sample QC.  eagle_qc.hip: counts[n][4] (hom A1, het, hom A2, missing per INDIVIDUAL; zeroed by the caller before a file's first
// window) += the counts over `rows` raw .bed rows; ibs0 / hethet (n x n int32, full and symmetric) from the Gram accumulators D32, Q32
// (n_pad x n_pad, upper 256-tiles live) and the marker count L; p[L] = the Hardy-Weinberg exact test of counts[L][stride] (stride 3
// or 4, the first three columns used).  eagle_i8mfma.hip: rows x row_bytes of an fp4 image copied with every code's sign bit cleared.
// eagle_api.cpp: both Gram products of M.ascii and the finish, resident or streamed (the host side of eagle_sample_ibs).
extern "C" int eagle_dev_bed_sample_counts(eagle_ctx* ctx, const uint8_t* bed, long rows, long n, int32_t* counts, void* stream);
extern "C" int eagle_dev_ibs_finish(eagle_ctx* ctx, const int32_t* D32, const int32_t* Q32, long n, long n_pad, long L, int32_t* ibs0,
                                    int32_t* hethet, void* stream);
extern "C" int eagle_dev_hwe_exact(eagle_ctx* ctx, const int32_t* counts, long L, int stride, double* p, void* stream);
extern "C" int eagle_dev_f4_abs(eagle_ctx* ctx, const void* src4, long ld4_src, long rows, long row_bytes, void* dst4, long ld4_dst, void* stream);
int eagle_ibs_counts(eagle_ctx* ctx, const char* path, long n, long L, double mem_gb, int threads, int32_t* ibs0_out, int32_t* hethet_out);
// kNN imputation (eagle_impute.hip; include/eagle_hip.h section 1b'''i), device pointers throughout.  nbr[n][K] from the n x n int32 matrices
// of eagle_dev_ibs_finish.  out = `rows` raw .bed rows with every missing genotype filled, counts[rows][2] = (by vote, by fallback), from
// the rows, their counts mcounts[rows][4] (eagle_dev_bed_marker_counts) and a neighbour table whose entries the CALLER has checked to lie
// in [-1, n): the kernel indexes the staged rows with them.
extern "C" int eagle_dev_knn_rows(eagle_ctx* ctx, const int32_t* ibs0, const int32_t* hethet, long n, int K, int32_t* nbr, void* stream);
extern "C" int eagle_dev_knn_rows_dist(eagle_ctx* ctx, const uint32_t* dist, long n, int K, int32_t* nbr, void* stream);
extern "C" int eagle_dev_bed_impute(eagle_ctx* ctx, const uint8_t* bed, long rows, long n, const int32_t* nbr, int K, int k, int min_votes,
                                    const int32_t* mcounts, uint8_t* out, int32_t* counts, void* stream);
// LD-kNNi (eagle_ldknn.hip; the header's section on LD-kNNi), device pointers throughout.  `bed` holds `staged` raw rows from marker h_lo of the
// file on; the `rows` rows from row `first` of them (marker m0 = h_lo + first) are patched into out, counts[rows][2] = (by vote, by
// fallback), mcounts[rows][4] their counts.  partners = L x l by the file's marker; the CALLER has checked that every entry of the rows
// patched is -1 or names a staged row: the kernel indexes the staged rows with them.
extern "C" int eagle_dev_bed_impute_ldknn(eagle_ctx* ctx, const uint8_t* bed, long staged, long first, long rows, long m0, long h_lo, long n,
                                          const int32_t* partners, int l, int k, int min_votes, int min_overlap, const int32_t* mcounts,
                                          uint8_t* out, int32_t* counts, void* stream);
// Pairwise-complete LD from a .bed file (eagle_bedld.hip; include/eagle_hip.h section 1b'''iv), device pointers throughout.  X / C / U: the
// three marker-major int8 operand images (P x ld, ld % 16 == 0, zero from individual n on) of the staged rows offsets[0 .. P) of `bed`
// (`staged` raw rows; offsets null: rows 0 .. P - 1), each checked by the CALLER to lie in [0, staged).  band / r2band: k_ld_tile's two
// outputs for `rows` consecutive panel markers from the six pairwise-complete sums; min_overlap >= 1.
extern "C" int eagle_dev_bed_ld_pack(eagle_ctx* ctx, const uint8_t* bed, long staged, const long* offsets, long P, long n, long ld, int8_t* X,
                                     int8_t* C, int8_t* U, void* stream);
extern "C" int eagle_dev_bedld_band(eagle_ctx* ctx, const int8_t* X, const int8_t* C, const int8_t* U, long rows, long n, long ld, long window,
                                    double t, long min_overlap, uint64_t* mask, long words_per_row, void* stream);
extern "C" int eagle_dev_bedld_r2band(eagle_ctx* ctx, const int8_t* X, const int8_t* C, const int8_t* U, long rows, long n, long ld, long window,
                                      long min_overlap, double* band, void* stream);
// Runs of homozygosity (eagle_roh.hip; include/eagle_hip.h section 1b'''vi), device pointers throughout.  planes: 3 x markers x ceil(n / 64)
// uint64 (flagged, het, miss), marker-major; blk: the nb + 1 block bounds of rule 2.  The flags calls write the planes' rows of the panel
// markers [c0, c1) from a source whose row 0 is panel marker g0 and which holds the markers [max(0, c0 - (w - 1)), min(markers, c1 + w -
// 1)) at least: an int8 Mt image, or raw .bed rows (the row of marker g0 + p at offsets[p], null: row p; checked by the CALLER).  The
// segments call is the count pass (fill == 0: cnt n x nb written, ind n x 4 added to -- zero it first) or the fill pass (rows of seg from
// the exclusive scan offs of cnt).
extern "C" int eagle_dev_roh_flags_i8(eagle_ctx* ctx, const int8_t* Mt8, long ld, long n, long g0, long c0, long c1, const int32_t* blk, long nb,
                                      const eagle_roh_params* prm, uint64_t* planes, long markers, void* stream);
extern "C" int eagle_dev_roh_flags_bed(eagle_ctx* ctx, const uint8_t* bed, const long* offsets, long n, long g0, long c0, long c1,
                                       const int32_t* blk, long nb, const eagle_roh_params* prm, uint64_t* planes, long markers, void* stream);
extern "C" int eagle_dev_roh_segments(eagle_ctx* ctx, const uint64_t* planes, long markers, long n, const int32_t* blk, long nb, const int64_t* pos,
                                      const eagle_roh_params* prm, int fill, int32_t* cnt, int64_t* ind, const int64_t* offs, int32_t* seg,
                                      void* stream);
// Pairwise IBD-type segments (eagle_ibd.hip; include/eagle_hip.h section 1b'''vii), device pointers throughout.  planes: A (hom A1), B (hom
// A2) and from the .bed file C (called), each ceil(markers / 64) x np uint64 with np = n rounded up to 64, WORD-MAJOR: word w of individual i
// at w * np + i.  The planes calls write the words of the individuals [r0, r0 + nr) from an individual-major int8 image whose row 0 is
// individual r0, or the words [w0, w1) of everybody from raw .bed rows (the row of panel marker g0 + p at offsets[p], null: row p; checked
// by the CALLER).  The walk is the count pass (fill == 0: tot P x 4 written) or the fill pass (rows of seg from the exclusive scan offs of
// the counts); pairs null = all pairs, P = n (n - 1) / 2; cut = the cut plane of rule 3 (ibd_cut_plane).
extern "C" int eagle_dev_ibd_planes_i8(eagle_ctx* ctx, const int8_t* img, long ld, long r0, long nr, long n, long L, uint64_t* planes,
                                       void* stream);
extern "C" int eagle_dev_ibd_planes_bed(eagle_ctx* ctx, const uint8_t* bed, const long* offsets, long n, long g0, long w0, long w1, long L,
                                        uint64_t* planes, void* stream);
extern "C" int eagle_dev_ibd_walk(eagle_ctx* ctx, const uint64_t* planes, int nplanes, const uint64_t* cut, long n, long L, const int32_t* pairs,
                                  long P, const int32_t* blk, long nb, const int64_t* pos, const eagle_ibd_params* prm, int fill, int64_t* tot,
                                  const int64_t* offs, int32_t* seg, void* stream);
// Mendel errors and parentage assignment (eagle_mendel.hip; include/eagle_hip.h section 1b'''viii) on the planes above, device pointers
// throughout.  trios: T x 3 int32; out: T x 6 int32; marker: L int32 ZEROED by the caller, or null.  The gather writes the sub-planes of an
// index list (-1: zero words), nplanes x ceil(L / 64) x cnt rounded up to 64 words.  The parentage call works on the offspring [o0, o0 + no)
// (no <= 65535) of the gathered lists (ns / nd = 0: the sub-planes of the one index -1): part_k / part_n hold 2 no eagle_parentage_parts(ns,
// nd) entries; best: n_o x 8 int32.
extern "C" int eagle_dev_mendel_trios(eagle_ctx* ctx, const uint64_t* planes, int nplanes, long n, long L, const int32_t* trios, long T, int32_t* out,
                                      int32_t* marker, void* stream);
extern "C" int eagle_dev_plane_gather(eagle_ctx* ctx, const uint64_t* planes, int nplanes, long n, long L, const int32_t* idx, long cnt, uint64_t* dst,
                                      void* stream);
extern "C" long eagle_parentage_parts(long ns, long nd);
// Transmission disequilibrium test (eagle_tdt.hip; include/eagle_hip.h section 1b''''viii) on the same planes, device pointers throughout.
// trios: T x 3 int32; out: T x 6 int32; marker: L x 5 int32 ZEROED by the caller.  The finish turns marker into dobs / V / keyobs (L each).
// The image: rows [m0, m0 + rows) of D[m][t] = d of rule 2, int8 with leading dimension ld = a multiple of 16 >= T, m0 a multiple of 64,
// every byte of the rows written.  The signs: op [R][ldop] of +-1 for the flips first .. first + R - 1 of the families fam[T], zeros
// from T on.
extern "C" int eagle_dev_tdt_trios(eagle_ctx* ctx, const uint64_t* planes, int nplanes, long n, long L, const int32_t* trios, long T, int32_t* out,
                                   int32_t* marker, void* stream);
extern "C" int eagle_dev_tdt_finish(eagle_ctx* ctx, const int32_t* marker, long L, int64_t* dobs, int64_t* V, double* keyobs, void* stream);
extern "C" int eagle_dev_tdt_image(eagle_ctx* ctx, const uint64_t* planes, int nplanes, long n, long L, const int32_t* trios, long T, long m0,
                                   long rows, int8_t* img, long ld, void* stream);
extern "C" int eagle_dev_tdt_signs(eagle_ctx* ctx, const int32_t* fam, long T, uint64_t seed, long first, long R, int8_t* op, long ldop,
                                   void* stream);
extern "C" int eagle_dev_parentage(eagle_ctx* ctx, const uint64_t* O, long n_o, const uint64_t* S, long ns, const uint64_t* D, long nd, int nplanes, long L,
                                   const int32_t* oidx, const int32_t* sidx, const int32_t* didx, long o0, long no, int min_overlap, int allow_self,
                                   uint64_t* part_k, int32_t* part_n, int32_t* best, void* stream);
// Epistasis (eagle_epi.hip; include/eagle_hip.h section 1b''''ii): msu[3 r ..] = (sum g, sum g^2, sum y g) of the rows of an int8 Mt tile, y n int32
// on the device.  The tile kernel is launched by the two entry points in the same file.
extern "C" int eagle_dev_epi_marker(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, const int32_t* y, int64_t* msu, void* stream);
// Pairwise-complete IBS counts from a .bed file (eagle_bedibs.hip; include/eagle_hip.h section 1b'''ii), device pointers throughout.  The
// four fp4 operand images (g, u, h, c; plane p at M4 + p * plane_bytes, n_pad rows of ld4 bytes, L_pad markers written) of `rows` raw
// .bed rows, `include` one byte per row or null; the four n x n int32 results and dist (or null) from the four Gram accumulators
// (n_pad x n_pad, upper 256-tiles live).  eagle_api.cpp: the finish and the download of the results from the accumulators acc4 (D, Q, H,
// N side by side, pad256(n)^2 int32 each): the tail of eagle_bed_sample_ibs.
extern "C" int eagle_dev_bed_pack_fp4(eagle_ctx* ctx, const uint8_t* bed, long rows, long n, const uint8_t* include, long n_pad, long L_pad,
                                      void* M4, long ld4, long plane_bytes, void* stream);
extern "C" int eagle_dev_bed_ibs_finish(eagle_ctx* ctx, const int32_t* D32, const int32_t* Q32, const int32_t* H32, const int32_t* N32, long n,
                                        long n_pad, long linc, int min_overlap, int32_t* ncalled, int32_t* ibs0, int32_t* hethet, int32_t* hetsum,
                                        uint32_t* dist, void* stream);
int eagle_bed_ibs_results(eagle_ctx* ctx, const int32_t* acc4, long n, long linc, int min_overlap, int32_t* ncalled_out, int32_t* ibs0_out,
                          int32_t* hethet_out, int32_t* hetsum_out, uint32_t* dist_out);
// GRM (eagle_grm.hip; include/eagle_hip.h section 1b'''').  B[r][c] = digit[c] * A[r][c] for the rows [0, rows) and 16-byte column groups of
// an individual-major int8 window (A in {-1, 0, +1}, digit in [0, 127]; rows [n, rows) of B are written as zeros); the NT product
// C32[i][j] += sum_k A[i][k] B[j][k] on the tile engine of k_syrk_i8 (upper 256-tiles live); Q = C0 + 128 C1 + 128^2 C2 (a NULL plane
// is zero) as the full symmetric n x n int64 matrix.  eagle_api.cpp: the windows of M.ascii, resident or streamed (eagle_weighted_gram).
extern "C" int eagle_dev_scale_cols_i8(eagle_ctx* ctx, const int8_t* A, long ldA, long n, long rows, long cols, const uint8_t* digit, int8_t* B,
                                       long ldB, void* stream);
extern "C" int eagle_dev_gram_i8ab(eagle_ctx* ctx, const int8_t* A, long ldA, const int8_t* B, long ldB, long n_pad, long K_pad, int32_t* C32,
                                   void* stream);
extern "C" int eagle_dev_wgram_finish(eagle_ctx* ctx, const int32_t* C0, const int32_t* C1, const int32_t* C2, long n, long n_pad, int64_t* Q,
                                      void* stream);
int eagle_wgram(eagle_ctx* ctx, const char* path, long n, long L, const uint32_t* q, double mem_gb, int threads, int64_t* Q_out);
// eagle_i8mfma.hip: the upper-triangular 256-tile pairs (ti << 16 | tj) of an nt x nt tile grid in super-tile order, cached per device
int syrk_pair_table(eagle_ctx* ctx, int nt, const int** out, hipStream_t stream);
inline bool eagle_sidecar_enabled() { const char* e = getenv("EAGLE_HIP_SIDECAR"); return !(e && e[0] == '0'); }
// Whole-file resident copy (loads it if needed); EAGLE_OK, 2 (too large for HBM: stream it) or an error.
int eagle_get_resident(eagle_ctx* ctx, const char* path, long rows, long cols, double max_mem_gb, int threads, const GenoEntry** out);
// The same for the window [row0, row0+rows) x [col0, col0+cols) of the file (a marker shard of a multi-device context).
int eagle_get_resident_window(eagle_ctx* ctx, const char* path, long row0, long rows, long col0, long cols, double max_mem_gb, int threads,
                              const GenoEntry** out);
size_t eagle_resident_budget();
// The VIEW alias `path` names on this context, or nullptr.
static inline const ViewAlias* eagle_view_find(const eagle_ctx* ctx, const char* path) {
    for (auto& v : ctx->views) if (v.alias == path) return &v;
    return nullptr;
}
// Size and mtime that key the cache entries of `path`: the file's own, or for a VIEW alias its source's as recorded at
// registration.  EAGLE_ERR_OPEN if the file is missing, EAGLE_ERR_FORMAT if an alias's source changed since.
int eagle_file_key(eagle_ctx* ctx, const char* path, off_t* size, long* mtime_ns);
size_t eagle_drop_f4_images(eagle_ctx* ctx);   // frees the fp4 MM^T operand images kept with resident files; bytes given back

static inline double now_s() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}
static inline int ndev_of(eagle_ctx* ctx) { return 1 + (int)ctx->peers.size(); }
static inline eagle_ctx* dev_ctx(eagle_ctx* ctx, int k) { return k == 0 ? ctx : ctx->peers[k - 1]; }
// this device's resident genotype copies only (safe from a per-device worker thread)
static inline void drop_cache_local(eagle_ctx* ctx) {
    (void)hipSetDevice(ctx->device);
    for (auto& g : ctx->cache) { if (g.dev) (void)hipFree(g.dev); if (g.dev_s) (void)hipFree(g.dev_s); if (g.cshift) (void)hipFree(g.cshift); if (g.l1) (void)hipFree(g.l1); if (g.dev_f4) (void)hipFree(g.dev_f4); }
    ctx->cache.clear();
    if (ctx->f4_buf) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(ctx->f4_buf); ctx->f4_buf = nullptr; ctx->f4_cap = 0; }
}
#define EAGLE_STREAM 2
// Resident int8 image of a window of a genotype file (eagle_load.cpp); reserve_bytes: HBM the caller still needs.
int get_resident(eagle_ctx* ctx, const char* path, long row0, long rows, long col0, long cols, double max_mem_gb, int threads,
                 GenoEntry** out, size_t reserve_bytes = (size_t)1 << 30);
// The lines `runs` (disjoint, in any order) of the genotype file or VIEW alias `path`, characters [col0, col0 + ncols), to consecutive
// rows of dst (eagle_dev_load_ascii is one run).
int eagle_load_rows(eagle_ctx* ctx, const char* path, const std::vector<RowRun>& runs, long col0, long ncols, int8_t* dst, long ld,
                    double max_mem_gb, int threads);
#endif
