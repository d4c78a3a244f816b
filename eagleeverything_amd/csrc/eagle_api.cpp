// eagle_api.cpp -- host side of libeaglehip.so: context, streamed marker chunks, and the
// reference-shaped entry points of section 1 of include/eagle_hip.h.
//
// What is replaced (E/ = MyPackage/Eagle/ of the reference):
//   eagle_read_block ............. E/src/ReadBlock.cpp:16-68
//   eagle_calculateMMt ........... E/src/calculateMMt_rcpp.cpp:19-185
//   eagle_calculate_a_and_vara ... E/src/calculate_a_and_vara_rcpp.cpp:22-241
//   eagle_calculate_reduced_a .... E/src/calculate_reduced_a_rcpp.cpp:20-171
//   eagle_last_scan_argmax ....... E/R/find_qtl.R:71-83
//   eagle_last_mmt_normalised .... E/R/calcMMt.R:13
//
// Design: the reference re-parses the text file into an n x L (or L x n) matrix of doubles on every call and,
// when that does not fit `availmemGb`, re-scans the file from line 0 once per block.  Here a text tile is
// pread() into pinned memory by `num_cores` threads, copied to HBM, decoded on the device to int8 {-1,0,1} and
// kept resident (one byte per genotype: 10k x 1M = 10 GB of the 288 GB) for every later call on the same file.
// All arithmetic happens in the HIP kernels of eagle_kernels.hip; there is no host compute path.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <stdlib.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "eagle_ctx.h"
#include "eagle_reshape.h"

thread_local char g_open_err[512];
extern "C" int eagle_fail(eagle_ctx* ctx, int code, const char* msg) {
    if (ctx) snprintf(ctx->err, sizeof ctx->err, "%s", msg);
    return code;
}
extern "C" int eagle_fail_hip(eagle_ctx* ctx, hipError_t e, const char* where) {
    if (ctx) snprintf(ctx->err, sizeof ctx->err, "HIP error in %s: %s", where, hipGetErrorString(e));
    return EAGLE_ERR_HIP;
}

// Grow-only device arena: the n x n operand images and kernel workspaces of a call are carved from one allocation that
// survives between calls (a find_qtl iteration would otherwise pay ~10 hipMalloc/hipFree pairs of 100s of MB each).
// The first allocation of a large arena is the slowest thing a first find_qtl call does (3-6 s for 100 GB at 50,000 individuals:
// the driver maps the pages).  Whoever knows the problem size earlier -- eagle_calculateMMt (AM() calls it once, then spends seconds in
// the host's eigen-decomposition), eagle_prepare_scan, EAGLE_HIP_ARENA_GB at eagle_open -- starts it on a background thread;
// arena_reserve collects it.
struct ArenaPrefetch { std::thread th; void* p = nullptr; size_t bytes = 0; hipError_t e = hipSuccess; };
static void arena_collect(eagle_ctx* ctx) {
    ArenaPrefetch* pf = (ArenaPrefetch*)ctx->arena_prefetch;
    if (!pf) return;
    ctx->arena_prefetch = nullptr;
    if (pf->th.joinable()) pf->th.join();
    if (pf->e == hipSuccess && pf->p) {
        if (pf->bytes > ctx->arena_cap) {
            if (ctx->arena) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(ctx->arena); }
            ctx->arena = pf->p;
            ctx->arena_gen++;
            ctx->arena_cap = pf->bytes;
        } else (void)hipFree(pf->p);
    } else (void)hipGetLastError();
    delete pf;
}
static void arena_prefetch(eagle_ctx* ctx, size_t total, bool only_if_roomy = false) {
    if (ctx->arena_prefetch || total <= ctx->arena_cap || total < ((size_t)4 << 30)) return;
    if (only_if_roomy) {   // a guess about what the caller does next must not crowd the card: at most half of what is free now
        size_t freeb = 0, totalb = 0;
        if (hipMemGetInfo(&freeb, &totalb) != hipSuccess || total > freeb / 2) { (void)hipGetLastError(); return; }
    }
    ArenaPrefetch* pf = new ArenaPrefetch;
    pf->bytes = total;
    const int device = ctx->device;
    pf->th = std::thread([pf, device] {
        pf->e = hipSetDevice(device);
        if (pf->e == hipSuccess) pf->e = dev_alloc(&pf->p, pf->bytes);
    });
    ctx->arena_prefetch = pf;
}
// Frees the fp4 operand images of MM^T kept with the resident files (GenoEntry.dev_f4: n L / 2 bytes each, 5 GB at 10,000 x 1,000,000;
// the next calculateMMt on the file re-makes its image in 3 ms).  Returns the bytes given back.
size_t eagle_drop_f4_images(eagle_ctx* ctx) {
    size_t freed = 0;
    for (GenoEntry& g : ctx->cache)
        if (g.dev_f4) {
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipFree(g.dev_f4);
            g.dev_f4 = nullptr;
            freed += (size_t)g.rows_pad * (size_t)g.ld / 2;
        }
    return freed;
}
static int prepare_scan(eagle_ctx* ctx, long n, long L, bool only_if_roomy);
static int arena_reserve(eagle_ctx* ctx, size_t total) {
    ctx->arena_off = 0;
    arena_collect(ctx);
    if (total <= ctx->arena_cap) return EAGLE_OK;
    if (ctx->arena) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(ctx->arena); ctx->arena = nullptr; ctx->arena_cap = 0; }
    ctx->arena_gen++;
    hipError_t e = dev_alloc(&ctx->arena, total);
    if (e != hipSuccess && eagle_drop_f4_images(ctx) > 0) {   // the fp4 MM^T operand images kept with resident files are not in any budget
        (void)hipGetLastError();
        e = dev_alloc(&ctx->arena, total);
    }
    if (e != hipSuccess) return eagle_fail_hip(ctx, e, "arena hipMalloc");
    ctx->arena_cap = total;
    return EAGLE_OK;
}
static size_t arena_round(size_t b) { return (b + 255) / 256 * 256; }
// (`kept`: the block holds what an earlier call left for this one -- the cached S in its slot -- and is not scratch: DESIGN 3a)
template <class T> static T* arena_take(eagle_ctx* ctx, size_t bytes, bool kept = false) {
    T* p = (T*)((char*)ctx->arena + ctx->arena_off);
    ctx->arena_off += arena_round(bytes);
    if (!kept) (void)dev_scratch_handout(p, bytes);
    return p;
}
static bool timing_on() { static int v = -1; if (v < 0) v = getenv("EAGLE_HIP_TIMING") ? 1 : 0; return v == 1; }

// ------------------------------------------------------------------------------------------------
extern "C" const char* eagle_open_error(void) { return g_open_err; }

extern "C" eagle_ctx* eagle_open(int device) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        snprintf(g_open_err, sizeof g_open_err, "no HIP device available (%s); libeaglehip has no CPU fallback",
                 e != hipSuccess ? hipGetErrorString(e) : "0 devices");
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        snprintf(g_open_err, sizeof g_open_err, "device %d out of range (0..%d)", device, ndev - 1);
        return nullptr;
    }
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) {
        snprintf(g_open_err, sizeof g_open_err, "hipGetDeviceProperties: %s", hipGetErrorString(e));
        return nullptr;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        snprintf(g_open_err, sizeof g_open_err, "device %d is %s; this library is built for gfx950 (MI355X) only", device,
                 prop.gcnArchName);
        return nullptr;
    }
    if ((e = hipSetDevice(device)) != hipSuccess) {
        snprintf(g_open_err, sizeof g_open_err, "hipSetDevice: %s", hipGetErrorString(e));
        return nullptr;
    }
    eagle_ctx* ctx = new eagle_ctx();
    ctx->device = device;
    snprintf(ctx->arch, sizeof ctx->arch, "%s", prop.gcnArchName);
    ctx->cu_count = prop.multiProcessorCount;
    ctx->hbm_bytes = (int64_t)prop.totalGlobalMem;
    if ((e = dev_alloc(&ctx->d_scratch, EAGLE_SCR_BYTES)) != hipSuccess) {
        snprintf(g_open_err, sizeof g_open_err, "hipMalloc: %s", hipGetErrorString(e));
        delete ctx;
        return nullptr;
    }
    // EAGLE_HIP_TUNE=9 (TUNE_COMPILER_SCHEDULED): the compiler-scheduled forms of the two hand-scheduled kernels (k_vara_i8w, k_syrk_f4) for
    // a whole session: same results bit for bit, 3-8 % slower; a switch for ruling the inline-asm kernels out when chasing a problem
    if (const char* tv = getenv("EAGLE_HIP_TUNE")) ctx->tune = tune_known(atoi(tv));
    if (const char* ag = getenv("EAGLE_HIP_ARENA_GB")) {   // reserve the scan arena at open (background thread), e.g. 100 for 50,000 individuals
        const double gb = atof(ag);
        if (gb > 0.0 && gb < 4096.0) arena_prefetch(ctx, (size_t)(gb * 1e9));
    }
    if (const char* wm = getenv("EAGLE_HIP_W_MODE")) {   // 0 / 1 / 2: eagle_set_w_mode for an R session that has no call for it
        const int m = atoi(wm);
        if (m >= 0 && m <= 2) ctx->w_mode = m;
    }
    // EAGLE_HIP_SCAN_BUDGET=1e-7: the digit budget of the int8 scan for an R session that has no call for it (eagle_set_scan_budget)
    if (const char* bv = getenv("EAGLE_HIP_SCAN_BUDGET")) {
        const double b = atof(bv);
        if (b >= 1e-12 && b <= 5e-7) ctx->scan_budget = ctx->scan_budget_tight = b;
    }
    // the loader stream outranks the compute stream: its decode / unpack / fill kernels are microseconds of work that must get
    // onto CUs the scan kernel's long-lived workgroups fill completely (2 waves x 256 VGPRs per SIMD), as soon as one retires
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipStreamCreateWithPriority(&ctx->load_stream, hipStreamNonBlocking, prio_greatest)) != hipSuccess) {
        snprintf(g_open_err, sizeof g_open_err, "hipStreamCreate: %s", hipGetErrorString(e));
        delete ctx;
        return nullptr;
    }
    return ctx;
}

// ------------------------------------------------------------------------------------------------
// Several GPUs behind ONE context (the hook the reference left unused: AM(..., ngpu), E/R/AM.R:185-196, hard-wired to 0 at :214
// and handed to .find_qtl at :450-455).  The lead context owns one sub-context per further device; eagle_calculateMMt,
// eagle_calculate_a_and_vara and eagle_calculate_reduced_a split the file's markers into contiguous ranges (boundaries at
// multiples of 256), one per device, worked by one host thread + stream per device that are joined before the call returns.
// Exchange steps: ONE sum of the partial int32 MM^T (upper tiles) to the lead, the rows of W = S V S shared and all-gathered,
// the lower bounds of the shards' tsq maxima (8 bytes per device, on the host).  Between distinct devices the two device
// collectives are RCCL (ncclReduce / ncclAllGather over xGMI, communicators from ncclCommInitAll, the library dlopen()ed on
// first use); when the list names one card twice (how the path is tested on a one-GPU box) or EAGLE_HIP_COLLECTIVES=host,
// the sum is staged by device-to-device copies and W is computed on every device.
// ------------------------------------------------------------------------------------------------
#include <dlfcn.h>
#include <rccl/rccl.h>
struct RcclState {
    void* lib = nullptr;
    std::vector<ncclComm_t> comms;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;   // optional: a library without it keeps the old behaviour
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::mutex abort_mutex;
    std::atomic<bool> dead{false};   // the communicators were aborted: every later call takes the host-staged exchange
};
// A device whose collective could not be enqueued AFTER the rendezvous that precedes it would leave its peers blocked inside
// theirs: abort every communicator (the peers' collectives end with an error, their calls return it) and retire the RCCL leg of
// this context.  Once, whoever comes first.
static void rccl_abort_all(RcclState* r) {
    std::lock_guard<std::mutex> lock(r->abort_mutex);
    if (r->dead.exchange(true)) return;
    for (ncclComm_t& c : r->comms)
        if (c) { if (r->CommAbort) (void)r->CommAbort(c); c = nullptr; }
}
// The communicator of device k for the collective a worker is about to enqueue, or NULL when the leg was aborted meanwhile (ADVICE r3:
// a peer used to read comms[k] unlocked while rccl_abort_all was writing it).  A handle taken here can still be aborted before the
// enqueue -- RCCL then returns an error from the call, which is the outcome the abort exists for.
static ncclComm_t rccl_comm(RcclState* r, int k) {
    std::lock_guard<std::mutex> lock(r->abort_mutex);
    return r->dead.load() ? nullptr : r->comms[(size_t)k];
}
// EAGLE_HIP_FAULT=reduce | allgather [:<device index>]: the named collective reports a failure instead of running -- on every device,
// or on the one named, while its peers go on into theirs (tests of the abort path; never set in production).
static bool rccl_fault(const char* which, int k) {
    const char* e = getenv("EAGLE_HIP_FAULT");   // (tests set and unset it between calls of one process: a cached copy would go stale)
    if (!e) return false;
    const size_t n = strlen(which);
    if (strncmp(e, which, n) != 0) return false;
    if (e[n] == '\0') return true;
    return e[n] == ':' && atoi(e + n + 1) == k;
}
static RcclState* rccl_open(const int* devices, int ndev, char* err, size_t errlen) {
    RcclState* r = new RcclState();
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
        if ((r->lib = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
    if (!r->lib) { snprintf(err, errlen, "cannot load librccl: %s", dlerror()); delete r; return nullptr; }
    r->CommInitAll = (decltype(r->CommInitAll))dlsym(r->lib, "ncclCommInitAll");
    r->CommDestroy = (decltype(r->CommDestroy))dlsym(r->lib, "ncclCommDestroy");
    r->Reduce = (decltype(r->Reduce))dlsym(r->lib, "ncclReduce");
    r->AllGather = (decltype(r->AllGather))dlsym(r->lib, "ncclAllGather");
    r->GetErrorString = (decltype(r->GetErrorString))dlsym(r->lib, "ncclGetErrorString");
    r->CommAbort = (decltype(r->CommAbort))dlsym(r->lib, "ncclCommAbort");
    if (!r->CommInitAll || !r->CommDestroy || !r->Reduce || !r->AllGather || !r->GetErrorString) {
        snprintf(err, errlen, "librccl lacks an entry point");
        dlclose(r->lib); delete r; return nullptr;
    }
    r->comms.resize(ndev);
    ncclResult_t rc = r->CommInitAll(r->comms.data(), ndev, devices);
    if (rc != ncclSuccess) {
        snprintf(err, errlen, "ncclCommInitAll: %s", r->GetErrorString(rc));
        dlclose(r->lib); delete r; return nullptr;
    }
    return r;
}

extern "C" eagle_ctx* eagle_open_devices(const int* devices, int ndev) {
    if (!devices || ndev <= 0 || ndev > 64) { snprintf(g_open_err, sizeof g_open_err, "eagle_open_devices: bad device list"); return nullptr; }
    eagle_ctx* lead = eagle_open(devices[0]);
    if (!lead) return nullptr;
    for (int k = 1; k < ndev; k++) {
        eagle_ctx* sub = eagle_open(devices[k]);
        if (!sub) { eagle_close(lead); return nullptr; }
        sub->lead = lead;
        lead->peers.push_back(sub);
    }
    bool distinct = true;
    for (int a = 0; a < ndev; a++) for (int b = a + 1; b < ndev; b++) if (devices[a] == devices[b]) distinct = false;
    const char* env = getenv("EAGLE_HIP_COLLECTIVES");
    // EAGLE_HIP_COLLECTIVES=host: host-staged stand-in instead of RCCL; =rccl with ONE device: the exchange steps run anyway, on
    // a communicator of one rank (what a one-GPU box can exercise of the RCCL leg: tests/test_multi_device.py)
    const bool force1 = ndev == 1 && env && strcmp(env, "rccl") == 0;
    if ((ndev > 1 || force1) && distinct && !(env && strcmp(env, "host") == 0)) {
        lead->rccl = rccl_open(devices, ndev, g_open_err, sizeof g_open_err);
        if (!lead->rccl) { eagle_close(lead); return nullptr; }
    }
    (void)hipSetDevice(devices[0]);
    return lead;
}
// EAGLE_HIP_DEVICES="0,1,2,3" (several GPUs), else EAGLE_HIP_DEVICE=<d>, else device 0: what the R-side shim opens.
extern "C" eagle_ctx* eagle_open_env(void) {
    std::vector<int> devs;
    if (const char* e = getenv("EAGLE_HIP_DEVICES")) {
        for (const char* p = e; *p;) {
            char* end = nullptr;
            long v = strtol(p, &end, 10);
            if (end == p) { snprintf(g_open_err, sizeof g_open_err, "EAGLE_HIP_DEVICES: cannot parse '%s'", e); return nullptr; }
            devs.push_back((int)v);
            p = end;
            while (*p == ',' || *p == ' ') p++;
        }
    }
    if (devs.empty()) { const char* d = getenv("EAGLE_HIP_DEVICE"); devs.push_back(d ? atoi(d) : 0); }
    return devs.size() == 1 ? eagle_open(devs[0]) : eagle_open_devices(devs.data(), (int)devs.size());
}
extern "C" int eagle_device_count(eagle_ctx* ctx) { return ctx ? 1 + (int)ctx->peers.size() : 0; }

// fn(k, ctx_k) on every device: the lead's share on the calling thread (the only one that may send messages to R), one
// worker thread per further device; all joined before return.  First hard error wins, then the soft sentinel.
template <class F> static int run_on_devices(eagle_ctx* ctx, F fn) {
    const int nd = ndev_of(ctx);
    std::vector<int> rc(nd, 0);
    std::vector<std::thread> th;
    for (int k = 1; k < nd; k++) th.emplace_back([&rc, &fn, ctx, k] { rc[k] = fn(k, dev_ctx(ctx, k)); });
    rc[0] = fn(0, ctx);
    for (auto& t : th) t.join();
    (void)hipSetDevice(ctx->device);
    for (int k = 0; k < nd; k++)
        if (rc[k] < 0) {
            if (k) { char buf[1024]; snprintf(buf, sizeof buf, "device %d: %s", dev_ctx(ctx, k)->device, dev_ctx(ctx, k)->err); snprintf(ctx->err, sizeof ctx->err, "%s", buf); }
            return rc[k];
        }
    for (int k = 0; k < nd; k++) if (rc[k] > 0) return rc[k];
    return EAGLE_OK;
}

// The resident genotype files AND what this context holds between calls (the scan arena -- a background reservation in flight included
// --, the workspace of the int8 W products, the host copy of the cached S): everything a caller can get back without closing the context.
static void drop_workspaces(eagle_ctx* c) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    arena_collect(c);
    if (c->arena) { (void)hipFree(c->arena); c->arena = nullptr; c->arena_cap = 0; c->arena_off = 0; c->arena_gen++; }
    c->scache.forget_host();
    if (c->w8_ws) { (void)hipFree(c->w8_ws); c->w8_ws = nullptr; c->w8_ws_cap = 0; c->w8_ws_gen++; }
    w8_keep_forget(c->w8_keep);   // (what was kept with S lay in that workspace)
    c->w8_maxabs_ready = false;
    if (c->w8_true_ws) { (void)hipFree(c->w8_true_ws); c->w8_true_ws = nullptr; c->w8_true_cap = 0; }
    c->w8_active = false;
}
// The device-resident caller's promise about S (include/eagle_hip.h).  Every declaration is a new content number: declaring again after
// rewriting the image in place is how the caller says "S changed".
extern "C" int eagle_dev_declare_s(eagle_ctx* ctx, const double* Sa, long n, long n_pad) {
    if (!ctx) return EAGLE_ERR_ARG;
    if (!Sa || n <= 0 || n > n_pad) return eagle_fail(ctx, EAGLE_ERR_ARG, "declare_s: bad image or sizes");
    ctx->w8_declared.Sa = Sa; ctx->w8_declared.n = n; ctx->w8_declared.np = n_pad;
    ctx->w8_declared.s_gen = ctx->w8_s_gen_next++;
    return EAGLE_OK;
}
extern "C" int eagle_dev_forget_s(eagle_ctx* ctx) {
    if (!ctx) return EAGLE_ERR_ARG;
    ctx->w8_declared = W8Declared();
    w8_keep_forget(ctx->w8_keep);
    return EAGLE_OK;
}
extern "C" int eagle_w8_keep_stats(eagle_ctx* ctx, long* hits, long* misses) {
    if (!ctx) return EAGLE_ERR_ARG;
    long h = ctx->w8_keep_hits, m = ctx->w8_keep_misses;
    for (eagle_ctx* p : ctx->peers) { h += p->w8_keep_hits; m += p->w8_keep_misses; }
    if (hits) *hits = h;
    if (misses) *misses = m;
    return EAGLE_OK;
}
extern "C" void eagle_drop_cache(eagle_ctx* ctx) {
    if (!ctx) return;
    for (eagle_ctx* p : ctx->peers) { drop_cache_local(p); drop_workspaces(p); }
    drop_cache_local(ctx);
    drop_workspaces(ctx);
    (void)hipSetDevice(ctx->device);
}

extern "C" void eagle_close(eagle_ctx* ctx) {
    if (!ctx) return;
    if (ctx->rccl) {
        RcclState* r = (RcclState*)ctx->rccl;
        for (ncclComm_t c : r->comms) if (c) (void)r->CommDestroy(c);
        delete r;  // the library stays loaded
        ctx->rccl = nullptr;
    }
    for (eagle_ctx* p : ctx->peers) eagle_close(p);
    ctx->peers.clear();
    (void)hipSetDevice(ctx->device);
    eagle_linalg_release(ctx);
    eagle_spectral_release(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    eagle_drop_cache(ctx);
    for (auto& v : ctx->views) if (v.d_keep) (void)hipFree(v.d_keep);
    ctx->views.clear();
    if (ctx->d_mmt) (void)hipFree(ctx->d_mmt);
    if (ctx->d_mmt_max) (void)hipFree(ctx->d_mmt_max);
    if (ctx->d_a) (void)hipFree(ctx->d_a);
    if (ctx->d_vara) (void)hipFree(ctx->d_vara);
    if (ctx->d_bound) (void)hipFree(ctx->d_bound);
    if (ctx->argmax_ws) (void)hipFree(ctx->argmax_ws);
    if (ctx->d_scratch) (void)hipFree(ctx->d_scratch);
    ctx->scache.release();
    arena_collect(ctx);
    if (ctx->arena) (void)hipFree(ctx->arena);
    if (ctx->gemv_ws) (void)hipFree(ctx->gemv_ws);
    if (ctx->f4_buf) (void)hipFree(ctx->f4_buf);
    if (ctx->gemm_scratch) (void)hipFree(ctx->gemm_scratch);
    eagle_w8_release(ctx);
    if (ctx->w8_ws) (void)hipFree(ctx->w8_ws);
    if (ctx->w8_true_ws) (void)hipFree(ctx->w8_true_ws);
    if (ctx->w8_host) (void)hipHostFree(ctx->w8_host);
    if (ctx->d_c32) (void)hipFree(ctx->d_c32);
    if (ctx->d_pack) (void)hipFree(ctx->d_pack);
    if (ctx->d_pack2) (void)hipFree(ctx->d_pack2);
    for (int b = 0; b < 2; b++) { if (ctx->stage_pin[b]) (void)hipHostFree(ctx->stage_pin[b]); if (ctx->stage_raw[b]) (void)hipFree(ctx->stage_raw[b]); }
    (void)hipStreamDestroy(ctx->stream);
    if (ctx->load_stream) (void)hipStreamDestroy(ctx->load_stream);
    delete ctx;
}

extern "C" void* eagle_ctx_scratch(eagle_ctx* ctx) { return ctx->d_scratch; }
extern "C" void* eagle_ctx_f4_buffer(eagle_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->f4_cap) {
        const hipError_t eh = dev_scratch_handout(ctx->f4_buf, bytes);
        if (eh != hipSuccess) { (void)eagle_fail_hip(ctx, eh, "fp4 image hand-out"); return nullptr; }
        return ctx->f4_buf;
    }
    if (ctx->f4_buf) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(ctx->f4_buf); ctx->f4_buf = nullptr; ctx->f4_cap = 0; }
    hipError_t e = dev_alloc(&ctx->f4_buf, bytes);
    if (e != hipSuccess) { (void)eagle_fail_hip(ctx, e, "fp4 image hipMalloc"); ctx->f4_buf = nullptr; return nullptr; }
    ctx->f4_cap = bytes;
    return ctx->f4_buf;
}
extern "C" const char* eagle_last_error(eagle_ctx* ctx) { return ctx ? ctx->err : g_open_err; }
extern "C" void eagle_set_message_callback(eagle_ctx* ctx, eagle_message_fn fn, void* user) {
    if (ctx) { ctx->msg_fn = fn; ctx->msg_user = user; }
}
extern "C" int eagle_device_info(eagle_ctx* ctx, char* arch_out, int arch_len, int* cu_count, int64_t* hbm_bytes) {
    if (!ctx) return EAGLE_ERR_ARG;
    if (arch_out && arch_len > 0) snprintf(arch_out, arch_len, "%s", ctx->arch);
    if (cu_count) *cu_count = ctx->cu_count;
    if (hbm_bytes) *hbm_bytes = ctx->hbm_bytes;
    return EAGLE_OK;
}
extern "C" int eagle_set_scan_mode(eagle_ctx* ctx, int mode) {
    if (!ctx || mode < 0 || mode > 1) return EAGLE_ERR_ARG;
    ctx->scan_mode = mode;
    for (eagle_ctx* p : ctx->peers) p->scan_mode = mode;
    return EAGLE_OK;
}
extern "C" int eagle_set_scan_rounding(eagle_ctx* ctx, int stochastic) {
    if (!ctx || stochastic < 0 || stochastic > 1) return EAGLE_ERR_ARG;
    ctx->scan_stochastic = stochastic;
    for (eagle_ctx* p : ctx->peers) p->scan_stochastic = stochastic;
    return EAGLE_OK;
}
extern "C" int eagle_set_scan_budget(eagle_ctx* ctx, double relative_budget) {
    if (ctx && relative_budget == 0.0) {   // the default policy: 1e-7 where the digits that run certify it, else 5e-7
        ctx->scan_budget = 5e-7; ctx->scan_budget_tight = 1e-7; ctx->spectral_off = false;
        for (eagle_ctx* p : ctx->peers) { p->scan_budget = 5e-7; p->scan_budget_tight = 1e-7; p->spectral_off = false; }
        return EAGLE_OK;
    }
    if (!ctx || !(relative_budget >= 1e-12 && relative_budget <= 5e-7)) return EAGLE_ERR_ARG;   // 1.8 x budget is enforced per marker: never above 0.9e-6
    // a budget asked for is THE budget: nothing tighter is tried first (the default context tries 1e-7, then 5e-7; relative_budget = 0 restores that)
    ctx->scan_budget = ctx->scan_budget_tight = relative_budget;
    ctx->spectral_off = false;
    for (eagle_ctx* p : ctx->peers) { p->scan_budget = p->scan_budget_tight = relative_budget; p->spectral_off = false; }
    return EAGLE_OK;
}
// on = 0: this context stops taking a digit off under the spectral bound (what eagle_calculate_a_and_vara does by itself after a
// certificate that overflowed under it); on = 1 re-arms.  For callers of the device-resident entry points, which see the certificate
// themselves (eagleeverything_amd/sharded.py).  Not part of the public ABI.
extern "C" void eagle_dev_set_spectral(eagle_ctx* ctx, int on) { if (ctx) ctx->spectral_off = !on; }
extern "C" int eagle_set_scan_slices(eagle_ctx* ctx, int nslices) {
    if (!ctx || nslices < 0 || nslices > 8) return EAGLE_ERR_ARG;
    ctx->scan_slices = nslices;
    for (eagle_ctx* p : ctx->peers) p->scan_slices = nslices;
    return EAGLE_OK;
}

// ------------------------------------------------------------------------------------------------
// selected_loci rule (calculateMMt_rcpp.cpp:88; calculate_a_and_vara_rcpp.cpp:79; calculate_reduced_a_rcpp.cpp:74):
// masking fires iff element 0 is not NA.  NA arrives as NaN.
// ------------------------------------------------------------------------------------------------
static int parse_selected(eagle_ctx* ctx, const double* sel, long nsel, long bound, std::vector<long>& out) {
    const char* msg = parse_selected_core(sel, nsel, bound, out);  // eagle_host.h
    return msg ? eagle_fail(ctx, EAGLE_ERR_ARG, msg) : EAGLE_OK;
}

// Rows (multiple of 256) of a streamed chunk whose padded row length is `row_bytes`.
static long stream_chunk_rows(long row_bytes, long total_rows_pad) {
    return stream_chunk_rows_core(eagle_resident_budget(), row_bytes, total_rows_pad);  // eagle_host.h
}

// Out-of-core streaming: chunk k+1 is read (pread -> pinned -> H2D -> decode, all on ctx->load_stream) while the kernels
// of chunk k run on ctx->stream.  Two chunk buffers; an event per buffer says when its kernels are done.
struct ChunkRing {
    int8_t* buf[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    std::vector<hipEvent_t> ev;  // start / end of every chunk's kernels (timed: eagle_last_stream_stats)
    long k = 0;
    double t_begin = 0;
    ~ChunkRing() {
        for (int b = 0; b < 2; b++) if (done[b]) (void)hipEventDestroy(done[b]);
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    int init(eagle_ctx* ctx) {
        for (int b = 0; b < 2; b++) HIPCHK(ctx, hipEventCreateWithFlags(&done[b], hipEventDisableTiming));
        ctx->st_chunks = ctx->st_file_bytes = 0;
        ctx->st_pread_s = ctx->st_load_wall_s = ctx->st_wait_s = ctx->st_compute_s = ctx->st_total_s = ctx->st_starved_s = ctx->st_load_first_s = 0;
        return EAGLE_OK;
    }
    // returns the buffer holding the freshly loaded tile (zero padded to clear_bytes); the caller launches its kernels on
    // ctx->stream and then calls computed()
    int load(eagle_ctx* ctx, const char* path, long row0, long nrows, long col0, long ncols, long ld, size_t clear_bytes, double mem_gb,
             int threads, int8_t** out) {
        const int b = (int)(k & 1);
        const double t0 = now_s();
        if (k == 0) t_begin = t0;
        if (k >= 2) HIPCHK(ctx, hipEventSynchronize(done[b]));  // the kernels that read this buffer two chunks ago
        const double t1 = now_s();
        hipStream_t main = ctx->stream;
        ctx->stream = ctx->load_stream;  // every loader below works on ctx->stream
        int rc = EAGLE_OK;
        hipError_t e = hipMemsetAsync(buf[b], 0, clear_bytes, ctx->stream);
        if (e != hipSuccess) rc = eagle_fail_hip(ctx, e, "chunk memset");
        if (!rc) rc = eagle_dev_load_ascii(ctx, path, row0, nrows, col0, ncols, buf[b], ld, mem_gb, threads);
        if (!rc && (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) rc = eagle_fail_hip(ctx, e, "chunk load sync");
        ctx->stream = main;
        *out = buf[b];
        ctx->st_wait_s += t1 - t0;
        ctx->st_load_wall_s += now_s() - t1;
        if (k == 0) ctx->st_load_first_s = now_s() - t1;
        if (timing_on() && getenv("EAGLE_HIP_TIMING")[0] == '2')
            fprintf(stderr, "[eaglehip]   chunk %ld: host waits %.1f..%.1f ms, loads ..%.1f ms\n", k, (t0 - t_begin) * 1e3, (t1 - t_begin) * 1e3, (now_s() - t_begin) * 1e3);
        hipEvent_t e0 = nullptr;  // the chunk's kernels start here on ctx->stream
        if (!rc && hipEventCreate(&e0) == hipSuccess) { ev.push_back(e0); (void)hipEventRecord(e0, ctx->stream); }
        return rc;
    }
    int computed(eagle_ctx* ctx) {
        hipEvent_t e1 = nullptr;
        if (ev.size() == (size_t)(2 * k + 1) && hipEventCreate(&e1) == hipSuccess) { ev.push_back(e1); (void)hipEventRecord(e1, ctx->stream); }
        HIPCHK(ctx, hipEventRecord(done[(int)(k & 1)], ctx->stream));
        if (timing_on() && getenv("EAGLE_HIP_TIMING")[0] == '2') fprintf(stderr, "[eaglehip]   chunk %ld: kernels launched at %.1f ms\n", k, (now_s() - t_begin) * 1e3);
        k++;
        return EAGLE_OK;
    }
    // after the last chunk: waits for its kernels and closes the books
    void finish(eagle_ctx* ctx) {
        (void)hipStreamSynchronize(ctx->stream);
        double ms = 0, starved = 0;
        for (size_t i = 0; i + 1 < ev.size(); i += 2) {
            float t = 0;
            if (hipEventElapsedTime(&t, ev[i], ev[i + 1]) == hipSuccess) ms += t;
            // the compute stream sat idle between the end of chunk k's kernels and the moment chunk k+1 was loaded
            if (i + 2 < ev.size() && hipEventElapsedTime(&t, ev[i + 1], ev[i + 2]) == hipSuccess) starved += t;
        }
        ctx->st_chunks = k;
        ctx->st_compute_s = ms / 1e3;
        ctx->st_starved_s = starved / 1e3;
        ctx->st_total_s = now_s() - t_begin;
        if (timing_on()) {
            const double later = ctx->st_load_wall_s - ctx->st_load_first_s;  // loads that had kernels to hide under
            fprintf(stderr, "[eaglehip] streamed: %ld chunks, %.3f GB read in %.3f s (%.2f GB/s while reading), loads %.3f s (first %.3f s), "
                            "kernels %.3f s, compute stream starved for %.3f s (%.0f %% of the later loads hidden), wall %.3f s\n",
                    k, ctx->st_file_bytes / 1e9, ctx->st_pread_s, ctx->st_pread_s > 0 ? ctx->st_file_bytes / 1e9 / ctx->st_pread_s : 0.0,
                    ctx->st_load_wall_s, ctx->st_load_first_s, ctx->st_compute_s, ctx->st_starved_s,
                    later > 0 ? 100.0 * std::max(0.0, 1.0 - ctx->st_starved_s / later) : 100.0, ctx->st_total_s);
        }
    }
};

// One pass over the Lr markers of a shard that starts at marker m0 of the file: ONE block of the resident image g (ring NULL; Lc is
// then the shard's padded length), or blocks of Lc markers read back from the file through `ring`, whose two buffers hold Lc rows of
// np bytes each.  load() yields the block; the caller launches its kernels on ctx->stream -- on as many padded rows as IT works (the
// scan's main pass: full chunks of Lc; everybody else: eagle_pad(nr)) -- and calls computed(); finish() after the last block of a
// pass that went through.
struct MarkerBlock { const int8_t* image; long ld, r0, nr; };
struct MarkerBlocks {
    const char* path; long m0, Lr, n, np, Lc; double mem_gb;
    const GenoEntry* g;
    ChunkRing* ring;
    bool full_chunks;     // streamed: a buffer is cleared as a full chunk of Lc rows before its load (else eagle_pad(nr) rows)
    long r0 = 0;
    bool more() const { return r0 < Lr; }
    int slot() const { return ring ? (int)(ring->k & 1) : 0; }   // of the two ring buffers, the one the block loaded last lies in
    int load(eagle_ctx* ctx, MarkerBlock* b) {
        const long nr = std::min(Lc, Lr - r0);
        if (!ring) { *b = {g->dev, g->ld, r0, nr}; return EAGLE_OK; }
        int8_t* tile = nullptr;
        const int rc = ring->load(ctx, path, m0 + r0, nr, 0, n, np, (size_t)(full_chunks ? Lc : eagle_pad(nr)) * np, mem_gb, host_threads(), &tile);
        *b = {tile, np, r0, nr};
        return rc;
    }
    int computed(eagle_ctx* ctx) { r0 += Lc; return ring ? ring->computed(ctx) : EAGLE_OK; }
    void finish(eagle_ctx* ctx) { if (ring) ring->finish(ctx); }
};

// Phase clock of one scan call: HIP events on the compute stream, read after the call's final synchronisation
// (eagle_last_scan_timing).  The interval that ENDS at an event is booked under the event's tag.
enum { PH_START = 0, PH_UPLOAD, PH_W, PH_LOADWAIT, PH_PREPARE, PH_VARA, PH_CERT, PH_D2H, PH_COUNT };
struct PhaseEvents {
    std::vector<hipEvent_t> ev;
    std::vector<int> tag;
    ~PhaseEvents() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    void mark(hipStream_t st, int t) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return;
        if (hipEventRecord(e, st) != hipSuccess) { (void)hipEventDestroy(e); return; }
        ev.push_back(e); tag.push_back(t);
    }
    void sum(double* ms) const {  // ms[PH_COUNT]; the stream has been synchronised
        for (int i = 0; i < PH_COUNT; i++) ms[i] = 0.0;
        for (size_t i = 1; i < ev.size(); i++) {
            float t = 0;
            if (hipEventElapsedTime(&t, ev[i - 1], ev[i]) == hipSuccess) ms[tag[i]] += t;
        }
    }
};

static int upload_square_on(eagle_ctx* ctx, const double* host, long n, long np, double* dev, hipStream_t st) {
    HIPCHK(ctx, hipMemsetAsync(dev, 0, sizeof(double) * np * np, st));
    HIPCHK(ctx, hipMemcpy2DAsync(dev, sizeof(double) * np, host, sizeof(double) * n, sizeof(double) * n, n, hipMemcpyHostToDevice, st));
    return EAGLE_OK;
}
// column-major n x n host matrix -> zero padded np x np device image (row-major image of the transpose)
static int upload_square(eagle_ctx* ctx, const double* host, long n, long np, double* dev) { return upload_square_on(ctx, host, n, np, dev, ctx->stream); }
// The same upload through the context's two pinned staging buffers: host threads copy piece k + 1 of the caller's pageable matrix into
// one while the DMA of piece k runs out of the other (the runtime's own pageable path stages single-threaded: 25-27 GB/s on the GPU
// boxes against 50+ this way).  Synchronous for the caller's memory: nothing of `host` is in flight when it returns.
// block_rows / on_block: after every block of `block_rows` rows of the image (the last one runs to n_pad: padding rows are zero) an event is
// recorded on `st` and on_block(r0, r1, event) is called -- the caller makes its compute stream wait for the event and works on the rows.
static int upload_square_staged(eagle_ctx* ctx, const double* host, long n, long np, double* dev, hipStream_t st, long block_rows = 0,
                                const std::function<int(long, long, hipEvent_t)>& on_block = nullptr) {
    const size_t piece = (size_t)64 << 20, rowb = sizeof(double) * (size_t)n;
    if (!on_block && (rowb * (size_t)n < 4 * piece || rowb > piece)) return upload_square_on(ctx, host, n, np, dev, st);
    if (rowb > piece) return eagle_fail(ctx, EAGLE_ERR_ARG, "staged upload: a row does not fit a staging buffer");
    int rc = eagle_stage_ensure(ctx, piece);
    if (rc) return rc;
    HIPCHK(ctx, hipMemsetAsync(dev, 0, sizeof(double) * np * np, st));
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (int b = 0; b < 2; b++) HIPCHK(ctx, hipEventCreateWithFlags(&ev[b], hipEventDisableTiming));
    const long rows_per = (long)(piece / rowb);
    const int threads = std::max(1, std::min(host_threads(), 16));
    hipError_t e = hipSuccess;
    std::vector<hipEvent_t> block_events;
    int rcb = EAGLE_OK;
    long k = 0, block0 = 0;
    double t_wait = 0, t_copy = 0, t_issue = 0, t_cb = 0;   // (EAGLE_HIP_TIMING: where the host side of the upload spends its time)
    const bool timed = timing_on();
    const double t_begin = timed ? now_s() : 0.0;
    for (long r0 = 0; r0 < n && e == hipSuccess && !rcb; k++) {
        long nr = std::min(rows_per, n - r0);
        if (on_block && block_rows > 0) nr = std::min(nr, block0 + block_rows - r0);   // pieces end at block boundaries
        double tq = timed ? now_s() : 0.0;
        if (k >= 2) e = hipEventSynchronize(ev[k & 1]);   // the DMA that last read this buffer
        if (e != hipSuccess) break;
        if (timed) { const double t = now_s(); t_wait += t - tq; tq = t; }
        char* dst = (char*)ctx->stage_pin[k & 1];
        const char* src = (const char*)(host + r0 * n);
        parallel_for((long)(rowb * (size_t)nr), threads, [&](long a, long b, int) { memcpy(dst + a, src + a, (size_t)(b - a)); });
        if (timed) { const double t = now_s(); t_copy += t - tq; tq = t; }
        e = hipMemcpy2DAsync(dev + r0 * np, sizeof(double) * np, dst, rowb, rowb, (size_t)nr, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(ev[k & 1], st);
        if (timed) { const double t = now_s(); t_issue += t - tq; tq = t; }
        r0 += nr;
        if (on_block && e == hipSuccess && (r0 == block0 + block_rows || r0 == n)) {
            // the block [block0, r0) is on its way; the last one takes the zero padding rows n .. n_pad along (block_rows is a multiple
            // of 256, so a block that ends exactly at n leaves no padding rows behind)
            const long end = (r0 == n) ? np : r0;
            hipEvent_t be = nullptr;
            e = hipEventCreateWithFlags(&be, hipEventDisableTiming);
            if (e == hipSuccess) { block_events.push_back(be); e = hipEventRecord(be, st); }
            if (e == hipSuccess) rcb = on_block(block0, end, be);
            block0 = end;
            if (timed) t_cb += now_s() - tq;
        }
    }
    if (timed) {
        const double t_loop = now_s() - t_begin;
        (void)hipStreamSynchronize(st);
        fprintf(stderr, "[eaglehip] staged upload %ld x %ld (%d threads, %ld pieces): host loop %.1f ms = waiting for a buffer %.1f + memcpy %.1f (%.1f GB/s) + "
                "issue %.1f + block callbacks %.1f; all landed after %.1f ms (%.1f GB/s)\n", n, n, threads, k, t_loop * 1e3, t_wait * 1e3, t_copy * 1e3,
                rowb * (double)n / 1e9 / std::max(t_copy, 1e-9), t_issue * 1e3, t_cb * 1e3, (now_s() - t_begin) * 1e3, rowb * (double)n / 1e9 / (now_s() - t_begin));
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // (the staging buffers serve other loaders after this call)
    for (int b = 0; b < 2; b++) (void)hipEventDestroy(ev[b]);
    for (hipEvent_t be : block_events) (void)hipEventDestroy(be);
    if (rcb) { (void)hipStreamSynchronize(st); return rcb; }
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return eagle_fail_hip(ctx, e, "staged upload"); }
    return EAGLE_OK;
}
static int upload_vec(eagle_ctx* ctx, const double* host, long n, long np, double* dev) {
    HIPCHK(ctx, hipMemsetAsync(dev, 0, sizeof(double) * np, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dev, host, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    return EAGLE_OK;
}

// ------------------------------------------------------------------------------------------------
extern "C" int eagle_read_block(eagle_ctx* ctx, const char* asciifname, long start_row, long numcols, long numrows,
                                double* out) {
    if (!ctx) return EAGLE_ERR_ARG;
    if (start_row < 0 || numcols < 0 || numrows < 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "negative dimension");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (numcols == 0 || numrows == 0) return eagle_dev_load_ascii(ctx, asciifname, start_row, 0, 0, 0, nullptr, 0, 1.0, 4);  // the file must open
    const long ld = eagle_pad(numcols);
    DevBuf tile, dbl;
    HIPCHK(ctx, tile.alloc((size_t)numrows * ld));
    HIPCHK(ctx, dbl.alloc(sizeof(double) * (size_t)numrows * numcols));
    int rc = eagle_dev_load_ascii(ctx, asciifname, start_row, numrows, 0, numcols, tile.as<int8_t>(), ld, 1.0, 4);
    if (rc) return rc;
    rc = eagle_dev_i8_to_f64_colmajor(ctx, tile.as<int8_t>(), numrows, numcols, ld, dbl.as<double>(), ctx->stream);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out, dbl.p, sizeof(double) * (size_t)numrows * numcols, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

// grow-only ctx-owned device buffer
template <class T> static int ensure_buf(eagle_ctx* ctx, T** buf, size_t* cap, size_t bytes, const char* what) {
    if (bytes <= *cap) { HIPCHK(ctx, dev_scratch_handout(*buf, bytes)); return EAGLE_OK; }
    if (*buf) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(*buf); *buf = nullptr; *cap = 0; }
    hipError_t e = dev_alloc(buf, bytes);
    if (e != hipSuccess) return eagle_fail_hip(ctx, e, what);
    *cap = bytes;
    return EAGLE_OK;
}

// Exact int32 partial  sum_{c in [c0, c1)} m_c m_c^T  into ctx->d_c32 (zeroed here; upper 256-tiles live), with the columns of
// `sel` that fall into the range masked (calculateMMt_rcpp.cpp:88-92 as an exact rank-k downdate).  The window of M.ascii is
// kept resident if it fits, else streamed through HBM in marker windows.
static int mmt_range(eagle_ctx* ctx, const char* path, long n, long L, long c0, long c1, const std::vector<long>& sel, double mem_gb,
                     int threads, int quiet) {
    const long np = eagle_pad(n);
    int rc = ensure_buf(ctx, &ctx->d_c32, &ctx->c32_cap, sizeof(int32_t) * (size_t)np * np, "MM^T accumulator hipMalloc");
    if (rc) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->d_c32, 0, sizeof(int32_t) * (size_t)np * np, ctx->stream));
    const long Lw_all = c1 - c0;
    if (Lw_all <= 0) return EAGLE_OK;
    GenoEntry* g = nullptr;
    rc = get_resident(ctx, path, 0, n, c0, Lw_all, mem_gb, threads, &g, sizeof(int32_t) * (size_t)np * np);
    if (rc < 0) return rc;
    std::vector<long> in_range;
    for (long c : sel) if (c >= c0 && c < c1) in_range.push_back(c - c0);
    DevBuf dsel, win;
    if (rc == EAGLE_OK) {
        // the fp4 operand image stays with the resident file: a later calculateMMt on it (SummaryAM re-calls .calcMMt,
        // E/R/summary_am.R:140) is the SYRK + finish only
        const long Lwp = eagle_pad(Lw_all);
        if (!g->dev_f4) {
            hipError_t e = dev_alloc(&g->dev_f4, (size_t)np * (size_t)(Lwp / 2));
            if (e != hipSuccess) { g->dev_f4 = nullptr; (void)hipGetLastError(); }
            else if ((rc = eagle_dev_pack_fp4(ctx, g->dev, np, Lwp, g->ld, g->dev_f4, ctx->stream))) { (void)hipFree(g->dev_f4); g->dev_f4 = nullptr; return rc; }
        }
        rc = g->dev_f4 ? eagle_dev_mmt_accumulate_f4(ctx, g->dev_f4, np, Lwp, Lwp / 2, ctx->d_c32, ctx->stream)
                       : eagle_dev_mmt_accumulate(ctx, g->dev, np, Lwp, g->ld, ctx->d_c32, ctx->stream);  // no room: pack into the ctx buffer per call
        if (rc) return rc;
        if (!in_range.empty()) {
            HIPCHK(ctx, dsel.alloc(sizeof(long) * in_range.size()));
            HIPCHK(ctx, hipMemcpyAsync(dsel.p, in_range.data(), sizeof(long) * in_range.size(), hipMemcpyHostToDevice, ctx->stream));
            rc = eagle_dev_mmt_downdate(ctx, g->dev, np, g->ld, dsel.as<long>(), (long)in_range.size(), ctx->d_c32, ctx->stream);
            if (rc) return rc;
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        return EAGLE_OK;
    }
    // the window does not fit (or may not stay) in HBM: stream column windows of every line (= marker chunks) and accumulate
    // the exact integer partial products, MMt = sum_w M_w M_w^T.
    const long Lw = stream_chunk_rows(np, eagle_pad(Lw_all));  // window width in markers; rows of the window = np
    HIPCHK(ctx, win.alloc((size_t)2 * np * Lw));
    ChunkRing ring;
    if ((rc = ring.init(ctx))) return rc;
    ring.buf[0] = win.as<int8_t>();
    ring.buf[1] = win.as<int8_t>() + (size_t)np * Lw;
    if (!quiet) say(ctx, " M.ascii streamed through HBM in windows of %ld markers", Lw);
    for (long w0 = 0; w0 < Lw_all; w0 += Lw) {
        const long nc = std::min(Lw, Lw_all - w0);
        int8_t* wtile = nullptr;
        rc = ring.load(ctx, path, 0, n, c0 + w0, nc, Lw, (size_t)np * Lw, mem_gb, threads, &wtile);
        if (rc) return rc;
        rc = eagle_dev_mmt_accumulate(ctx, wtile, np, Lw, Lw, ctx->d_c32, ctx->stream);
        if (rc) return rc;
        std::vector<long> in_win;
        for (long c : in_range) if (c >= w0 && c < w0 + nc) in_win.push_back(c - w0);
        if (!in_win.empty()) {
            DevBuf dw;
            HIPCHK(ctx, dw.alloc(sizeof(long) * in_win.size()));
            HIPCHK(ctx, hipMemcpyAsync(dw.p, in_win.data(), sizeof(long) * in_win.size(), hipMemcpyHostToDevice, ctx->stream));
            // duplicates of one column must be dropped across the whole list, which k_mmt_downdate does per call:
            // selected_loci entries are distinct columns in any sane call; duplicates inside one window are handled
            rc = eagle_dev_mmt_downdate(ctx, wtile, np, Lw, dw.as<long>(), (long)in_win.size(), ctx->d_c32, ctx->stream);
            if (rc) return rc;
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        if ((rc = ring.computed(ctx))) return rc;
    }
    ring.finish(ctx);
    return EAGLE_OK;
}

static int download_big(eagle_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);   // below, with the other result paths

// Sample QC (eagle_sample_ibs, eagle_ingest.cpp): the two exact Gram products over all L markers of M.ascii, D = M M^T into ctx->d_c32
// and Q = (M o M)(M o M)^T into an accumulator of its own, by mmt_range's rules -- the resident image and its cached fp4 operand when
// the file fits, marker windows through the ChunkRing when it does not -- then k_ibs_finish.  Q's operand is never the cached image:
// a resident file's fp4 image is copied, sign bits cleared, window by window into the ctx-owned fp4 buffer (at most 1 GiB of it); a
// streamed window is packed into that buffer, multiplied for D, cleared in place and multiplied again for Q.
int eagle_ibs_counts(eagle_ctx* ctx, const char* path, long n, long L, double mem_gb, int threads, int32_t* ibs0_out, int32_t* hethet_out) {
    const long np = eagle_pad(n), Lp = eagle_pad(L);
    const size_t accb = sizeof(int32_t) * (size_t)np * np;
    int rc = ensure_buf(ctx, &ctx->d_c32, &ctx->c32_cap, accb, "MM^T accumulator hipMalloc");
    if (rc) return rc;
    DevBuf q32;
    HIPCHK(ctx, q32.alloc(accb));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_c32, 0, accb, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(q32.p, 0, accb, ctx->stream));
    GenoEntry* g = nullptr;
    rc = get_resident(ctx, path, 0, n, 0, L, mem_gb, threads, &g, 2 * accb);
    if (rc < 0) return rc;
    if (rc == EAGLE_OK) {
        if (!g->dev_f4) {   // as mmt_range makes it: a later calculateMMt on the file finds the image it would have made itself
            hipError_t e = dev_alloc(&g->dev_f4, (size_t)np * (size_t)(Lp / 2));
            if (e != hipSuccess) { g->dev_f4 = nullptr; (void)hipGetLastError(); }
            else if ((rc = eagle_dev_pack_fp4(ctx, g->dev, np, Lp, g->ld, g->dev_f4, ctx->stream))) { (void)hipFree(g->dev_f4); g->dev_f4 = nullptr; return rc; }
        }
        if (g->dev_f4 && (rc = eagle_dev_mmt_accumulate_f4(ctx, g->dev_f4, np, Lp, Lp / 2, ctx->d_c32, ctx->stream))) return rc;
        const long Lq = std::min(Lp, std::max(256L, (long)(((size_t)2 << 30) / (size_t)np) / 256 * 256));   // markers per window of Q's operand
        void* buf = eagle_ctx_f4_buffer(ctx, (size_t)np * (size_t)(Lq / 2));
        if (!buf) return EAGLE_ERR_HIP;
        for (long w0 = 0; w0 < Lp; w0 += Lq) {
            const long nc = std::min(Lq, Lp - w0);
            if (g->dev_f4) {
                rc = eagle_dev_f4_abs(ctx, (const uint8_t*)g->dev_f4 + w0 / 2, Lp / 2, np, nc / 2, buf, nc / 2, ctx->stream);
            } else {            // no room for the cached image: pack the window, use it for D, then clear the signs where it lies
                rc = eagle_dev_pack_fp4(ctx, g->dev + w0, np, nc, g->ld, buf, ctx->stream);
                if (!rc) rc = eagle_dev_mmt_accumulate_f4(ctx, buf, np, nc, nc / 2, ctx->d_c32, ctx->stream);
                if (!rc) rc = eagle_dev_f4_abs(ctx, buf, nc / 2, np, nc / 2, buf, nc / 2, ctx->stream);
            }
            if (!rc) rc = eagle_dev_mmt_accumulate_f4(ctx, buf, np, nc, nc / 2, q32.as<int32_t>(), ctx->stream);
            if (rc) return rc;
        }
    } else {
        const long Lw = stream_chunk_rows(np, Lp);  // window width in markers; rows of the window = np
        DevBuf win;
        HIPCHK(ctx, win.alloc((size_t)2 * np * Lw));
        void* buf = eagle_ctx_f4_buffer(ctx, (size_t)np * (size_t)(Lw / 2));
        if (!buf) return EAGLE_ERR_HIP;
        ChunkRing ring;
        if ((rc = ring.init(ctx))) return rc;
        ring.buf[0] = win.as<int8_t>();
        ring.buf[1] = win.as<int8_t>() + (size_t)np * Lw;
        for (long w0 = 0; w0 < L; w0 += Lw) {
            const long nc = std::min(Lw, L - w0);
            int8_t* wtile = nullptr;
            rc = ring.load(ctx, path, 0, n, w0, nc, Lw, (size_t)np * Lw, mem_gb, threads, &wtile);
            if (!rc) rc = eagle_dev_pack_fp4(ctx, wtile, np, Lw, Lw, buf, ctx->stream);
            if (!rc) rc = eagle_dev_mmt_accumulate_f4(ctx, buf, np, Lw, Lw / 2, ctx->d_c32, ctx->stream);
            if (!rc) rc = eagle_dev_f4_abs(ctx, buf, Lw / 2, np, Lw / 2, buf, Lw / 2, ctx->stream);
            if (!rc) rc = eagle_dev_mmt_accumulate_f4(ctx, buf, np, Lw, Lw / 2, q32.as<int32_t>(), ctx->stream);
            if (!rc) rc = ring.computed(ctx);
            if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        }
        ring.finish(ctx);
    }
    DevBuf out;
    const size_t outb = sizeof(int32_t) * (size_t)n * n;
    HIPCHK(ctx, out.alloc(2 * outb));
    rc = eagle_dev_ibs_finish(ctx, ctx->d_c32, q32.as<int32_t>(), n, np, L, out.as<int32_t>(), out.as<int32_t>() + (size_t)n * n, ctx->stream);
    if (rc) return rc;
    rc = download_big(ctx, ibs0_out, out.p, outb);
    if (rc) return rc;
    return download_big(ctx, hethet_out, (const char*)out.p + outb, outb);
}

// The tail of eagle_bed_sample_ibs (eagle_ingest.cpp, which runs the windows): k_bed_ibs_finish on the four accumulators and the
// results' way to the host, by eagle_ibs_counts' path.
int eagle_bed_ibs_results(eagle_ctx* ctx, const int32_t* acc4, long n, long linc, int min_overlap, int32_t* ncalled_out, int32_t* ibs0_out,
                          int32_t* hethet_out, int32_t* hetsum_out, uint32_t* dist_out) {
    const long np = eagle_pad(n);
    const size_t acc = (size_t)np * np, outn = (size_t)n * n, outb = sizeof(int32_t) * outn;
    DevBuf out;
    HIPCHK(ctx, out.alloc((dist_out ? 5 : 4) * outb));
    int32_t* o = out.as<int32_t>();
    int rc = eagle_dev_bed_ibs_finish(ctx, acc4, acc4 + acc, acc4 + 2 * acc, acc4 + 3 * acc, n, np, linc, min_overlap, o, o + outn, o + 2 * outn,
                                      o + 3 * outn, dist_out ? (uint32_t*)(o + 4 * outn) : nullptr, ctx->stream);
    if (rc) return rc;
    void* host[5] = {ncalled_out, ibs0_out, hethet_out, hetsum_out, dist_out};
    for (int k = 0; k < (dist_out ? 5 : 4); k++)
        if ((rc = download_big(ctx, host[k], o + (size_t)k * outn, outb))) return rc;
    return EAGLE_OK;
}

// GRM (eagle_weighted_gram, eagle_ingest.cpp): Q = sum_m q_m g_m g_m^T over all L markers of M.ascii by eagle_ibs_counts' rules -- the
// resident image when the file fits, marker windows through the ChunkRing when it does not.  q is cut into three base-128 digit planes
// on the host; per window of at most about 1 GiB and per plane that is not zero there, k_scale_cols_i8 writes digit x genotype into the
// ctx-owned operand buffer and k_gram_i8ab multiplies the window with it into that plane's int32 accumulator; k_wgram_finish sums the
// planes.  The genotype image is only ever read.
struct WgramPlanes {
    std::vector<uint8_t> h[3];     // digit planes, zero beyond L
    DevBuf d[3], c32;              // their device copies; the accumulators of the live planes, side by side
    int32_t* acc[3] = {nullptr, nullptr, nullptr};
    bool live(int p, long c0, long c1) const {
        const uint8_t* b = h[p].data();
        for (long c = c0; c < c1; c++) if (b[c]) return true;
        return false;
    }
};
// the columns [c0, c0 + cols) of the markers (cols % 256 == 0) lie at A (np rows, leading dimension ldA): every live plane's product
static int wgram_window(eagle_ctx* ctx, WgramPlanes& P, const int8_t* A, long ldA, long n, long np, long c0, long cols, long L) {
    const long Lq = std::min(cols, std::max(256L, (long)(((size_t)1 << 30) / (size_t)np) / 256 * 256));   // markers per operand window
    const bool wide = (double)ldA * 256.0 >= 2147483648.0;   // a line too long for the tile engine's 32-bit offsets: copy the window out first
    int8_t* buf = (int8_t*)eagle_ctx_f4_buffer(ctx, (size_t)np * (size_t)Lq * (wide ? 2 : 1));
    if (!buf) return EAGLE_ERR_HIP;
    for (long w0 = 0; w0 < cols; w0 += Lq) {
        const long nc = std::min(Lq, cols - w0), m0 = c0 + w0, m1 = std::min(m0 + nc, L);
        const int8_t* Aw = A + w0;
        long ldw = ldA;
        bool copied = false;
        for (int p = 0; p < 3; p++) {
            if (!P.acc[p] || m0 >= m1 || !P.live(p, m0, m1)) continue;
            if (wide && !copied) {
                int8_t* a2 = buf + (size_t)np * (size_t)Lq;
                HIPCHK(ctx, hipMemcpy2DAsync(a2, (size_t)nc, A + w0, (size_t)ldA, (size_t)nc, (size_t)np, hipMemcpyDeviceToDevice, ctx->stream));
                Aw = a2; ldw = nc; copied = true;
            }
            int rc = eagle_dev_scale_cols_i8(ctx, Aw, ldw, n, np, nc, P.d[p].as<uint8_t>() + m0, buf, nc, ctx->stream);
            if (!rc) rc = eagle_dev_gram_i8ab(ctx, Aw, ldw, buf, nc, np, nc, P.acc[p], ctx->stream);
            if (rc) return rc;
        }
    }
    return EAGLE_OK;
}
int eagle_wgram(eagle_ctx* ctx, const char* path, long n, long L, const uint32_t* q, double mem_gb, int threads, int64_t* Q_out) {
    const long np = eagle_pad(n), Lp = eagle_pad(L);
    const size_t accb = sizeof(int32_t) * (size_t)np * np, outb = sizeof(int64_t) * (size_t)n * n;
    GenoEntry* g = nullptr;
    int rc = get_resident(ctx, path, 0, n, 0, L, mem_gb, threads, &g, 3 * accb + outb + ((size_t)1 << 30));
    if (rc < 0) return rc;
    const bool resident = rc == EAGLE_OK;
    const long Lw = resident ? Lp : stream_chunk_rows(np, Lp);   // window width in markers; rows of the window = np
    const long Ld = (Lp + Lw - 1) / Lw * Lw;                     // the digit planes cover every window in full
    WgramPlanes P;
    int nlive = 0;
    for (int p = 0; p < 3; p++) {
        P.h[p].assign((size_t)Ld, 0);
        for (long m = 0; m < L; m++) P.h[p][(size_t)m] = (uint8_t)((q[m] >> (7 * p)) & 127u);
        if (P.live(p, 0, L)) nlive++; else P.h[p].clear();
    }
    HIPCHK(ctx, P.c32.alloc(accb * (size_t)std::max(nlive, 1)));
    if (nlive) HIPCHK(ctx, hipMemsetAsync(P.c32.p, 0, accb * (size_t)nlive, ctx->stream));
    for (int p = 0, k = 0; p < 3; p++) {
        if (P.h[p].empty()) continue;
        P.acc[p] = (int32_t*)((char*)P.c32.p + accb * (size_t)k++);
        HIPCHK(ctx, P.d[p].alloc((size_t)Ld));
        HIPCHK(ctx, hipMemcpyAsync(P.d[p].p, P.h[p].data(), (size_t)Ld, hipMemcpyHostToDevice, ctx->stream));
    }
    if (nlive && resident) {   // (q = 0 everywhere: no product)
        if ((rc = wgram_window(ctx, P, g->dev, g->ld, n, np, 0, Lp, L))) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    } else if (nlive) {
        DevBuf win;
        HIPCHK(ctx, win.alloc((size_t)2 * np * Lw));
        ChunkRing ring;
        if ((rc = ring.init(ctx))) return rc;
        ring.buf[0] = win.as<int8_t>();
        ring.buf[1] = win.as<int8_t>() + (size_t)np * Lw;
        for (long w0 = 0; w0 < L; w0 += Lw) {
            const long nc = std::min(Lw, L - w0);
            int8_t* wtile = nullptr;
            rc = ring.load(ctx, path, 0, n, w0, nc, Lw, (size_t)np * Lw, mem_gb, threads, &wtile);
            if (!rc) rc = wgram_window(ctx, P, wtile, Lw, n, np, w0, Lw, L);
            if (!rc) rc = ring.computed(ctx);
            if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        }
        ring.finish(ctx);
    }
    DevBuf out;
    HIPCHK(ctx, out.alloc(outb));
    rc = eagle_dev_wgram_finish(ctx, P.acc[0], P.acc[1], P.acc[2], n, np, out.as<int64_t>(), ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    return download_big(ctx, Q_out, out.p, outb);
}

extern "C" int eagle_calculateMMt(eagle_ctx* ctx, const char* f_name_ascii, double max_memory_in_Gbytes, int num_cores,
                                  const double* selected_loci, long n_selected, const long dims[2], int quiet,
                                  double* MMt_out) {
    if (!ctx) return EAGLE_ERR_ARG;
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "bad dims");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<long> sel;
    int rc = parse_selected(ctx, selected_loci, n_selected, L, sel);
    if (rc) return rc;
    say(ctx, " Number of cores being used for calculation is .. %d", num_cores);  // calculateMMt_rcpp.cpp:36
    // calculateMMt_rcpp.cpp:75-76,84,103-106: the reference chooses between one DGEMM and row blocks; a block
    // size of zero rows makes it divide by zero.  The device path needs no such split, but the failure is kept.
    double need = (double)((unsigned long)n * n * sizeof(double) + 2 * ((unsigned long)n * L * sizeof(double))) / 1e9;
    if (!(max_memory_in_Gbytes > need)) {
        double p2 = sqrt(4.0 * (double)L * (double)L + 4.0 * max_memory_in_Gbytes * 1e9 / sizeof(double));
        long rows_in_block = (long)((-2.0 * (double)L + p2) / 2.2);
        if (rows_in_block <= 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "availmemGb too small: zero rows per block");
        say(ctx, "number of rows in block is %ld", rows_in_block);  // :107-112, said whatever `quiet` is
        say(ctx, " 1 ");
    }
    const int threads = num_cores > 0 ? num_cores : 1;
    const long np = eagle_pad(n);
    const int nd = ndev_of(ctx);
    std::vector<long> edge;
    split_markers(L, nd, edge);
    const long packed = eagle_upper_tiles_count(np);
    RcclState* rccl = (RcclState*)ctx->rccl;
    if (rccl && rccl->dead) rccl = nullptr;   // aborted in an earlier call: host-staged sums from now on
    Rendezvous rv;
    rv.n = nd;
    rc = run_on_devices(ctx, [&](int k, eagle_ctx* c) -> int {
        hipError_t e = hipSetDevice(c->device);
        int r = e == hipSuccess ? mmt_range(c, f_name_ascii, n, L, edge[k], edge[k + 1], sel, max_memory_in_Gbytes, threads, quiet)
                                : eagle_fail_hip(c, e, "hipSetDevice");
        if (nd == 1 && !rccl) return r;
        // ONE sum of the partials: the upper 256-tiles of every device's accumulator, packed, to the lead
        if (!r) r = ensure_buf(c, &c->d_pack, &c->pack_cap, sizeof(int32_t) * (size_t)packed, "packed MM^T hipMalloc");
        if (!r) r = eagle_dev_tiles_pack(c, c->d_c32, np, c->d_pack, 0, c->stream);
        if (!r && (e = hipStreamSynchronize(c->stream)) != hipSuccess) r = eagle_fail_hip(c, e, "MM^T partial");
        if (!rv.arrive(r == 0)) return r ? r : eagle_fail(c, EAGLE_ERR_HIP, "another device failed before the MM^T sum");
        if (rccl) {
            const ncclComm_t comm = rccl_comm(rccl, k);
            ncclResult_t nr = (rccl_fault("reduce", k) || !comm) ? ncclSystemError
                                                   : rccl->Reduce(c->d_pack, c->d_pack, (size_t)packed, ncclInt32, ncclSum, 0, comm, c->stream);
            if (nr != ncclSuccess) { r = failf(c, EAGLE_ERR_HIP, "ncclReduce: %s", rccl->GetErrorString(nr)); rccl_abort_all(rccl); }
            else if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) r = eagle_fail_hip(c, e, "ncclReduce sync");
        } else if (k == 0) {  // host-staged stand-in: the peers' packed tiles are copied to the lead and added, one by one
            r = ensure_buf(c, &c->d_pack2, &c->pack2_cap, sizeof(int32_t) * (size_t)packed, "packed MM^T landing buffer");
            for (int p = 1; p < nd && !r; p++) {
                eagle_ctx* pc = dev_ctx(ctx, p);
                e = pc->device == c->device ? hipMemcpyAsync(c->d_pack2, pc->d_pack, sizeof(int32_t) * (size_t)packed, hipMemcpyDeviceToDevice, c->stream)
                                            : hipMemcpyPeerAsync(c->d_pack2, c->device, pc->d_pack, pc->device, sizeof(int32_t) * (size_t)packed, c->stream);
                if (e != hipSuccess) { r = eagle_fail_hip(c, e, "peer copy of a partial MM^T"); break; }
                r = eagle_dev_add_i32(c, c->d_pack, c->d_pack2, packed, c->stream);
            }
            if (!r && (e = hipStreamSynchronize(c->stream)) != hipSuccess) r = eagle_fail_hip(c, e, "staged MM^T sum");
        }
        rv.arrive(r == 0);  // the peers keep their buffers until the lead has read them
        return r;
    });
    if (rc) return rc;
    if ((nd > 1 || rccl) && (rc = eagle_dev_tiles_pack(ctx, ctx->d_c32, np, ctx->d_pack, 1, ctx->stream))) return rc;
    if (ctx->mmt_n != n) {
        if (ctx->d_mmt) { (void)hipFree(ctx->d_mmt); ctx->d_mmt = nullptr; }
        ctx->mmt_n = 0;
        HIPCHK(ctx, dev_alloc(&ctx->d_mmt, sizeof(double) * (size_t)n * n));
        ctx->mmt_n = n;
    }
    if (!ctx->d_mmt_max) HIPCHK(ctx, dev_alloc(&ctx->d_mmt_max, sizeof(double)));
    rc = eagle_dev_mmt_finish(ctx, ctx->d_c32, n, np, ctx->d_mmt, n, ctx->d_mmt_max, ctx->stream);
    if (rc) return rc;
    // AM() calls this once, then works on the host for seconds (eigen, REML) before its first find_qtl: the arena of that scan is
    // reserved meanwhile, on a background thread (a no-op below 4 GB)
    (void)prepare_scan(ctx, n, L, true);
    return download_big(ctx, MMt_out, ctx->d_mmt, sizeof(double) * (size_t)n * n);
}

// A large result back into the caller's (pageable) memory: the runtime's own pageable copy moves ~10 GB/s (80 ms for the 800 MB
// of MM^T at n = 10,000, most of a warm eagle_calculateMMt call).  Through the ctx's two pinned staging buffers instead: the DMA of
// piece k+1 (57 GB/s) runs under the host threads' copy of piece k into the destination.  Synchronises ctx->stream.
static int download_big(eagle_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes) {
    const size_t piece = (size_t)64 << 20;
    if (bytes < 4 * piece) {
        HIPCHK(ctx, hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return EAGLE_OK;
    }
    int rc = eagle_stage_ensure(ctx, piece);
    if (rc) return rc;
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (int b = 0; b < 2; b++) HIPCHK(ctx, hipEventCreateWithFlags(&ev[b], hipEventDisableTiming));
    const int threads = std::max(1, std::min(host_threads(), 16));
    const size_t np_ = (bytes + piece - 1) / piece;
    hipError_t e = hipSuccess;
    for (size_t k = 0; k <= np_ && e == hipSuccess; k++) {
        if (k < np_) {   // piece k into buffer k & 1 (its previous content, piece k - 2, was copied out in iteration k - 1)
            const size_t off = k * piece, len = std::min(piece, bytes - off);
            e = hipMemcpyAsync(ctx->stage_pin[k & 1], (const char*)dev_src + off, len, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipEventRecord(ev[k & 1], ctx->stream);
        }
        if (k > 0 && e == hipSuccess) {   // piece k - 1 out of its buffer, under the DMA of piece k
            const size_t off = (k - 1) * piece, len = std::min(piece, bytes - off);
            e = hipEventSynchronize(ev[(k - 1) & 1]);
            if (e == hipSuccess) {
                const char* src = (const char*)ctx->stage_pin[(k - 1) & 1];
                char* dst = (char*)host_dst + off;
                parallel_for((long)len, threads, [&](long a, long b, int) { memcpy(dst + a, src + a, (size_t)(b - a)); });
            }
        }
    }
    for (int b = 0; b < 2; b++) (void)hipEventDestroy(ev[b]);
    if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return eagle_fail_hip(ctx, e, "staged download"); }
    return EAGLE_OK;
}

extern "C" int eagle_last_mmt_normalised(eagle_ctx* ctx, double* MMt_norm_out, double* max_out) {
    if (!ctx || !ctx->d_mmt || ctx->mmt_n <= 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "no MMt result held");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long n = ctx->mmt_n;
    DevBuf tmp;
    HIPCHK(ctx, tmp.alloc(sizeof(double) * (size_t)n * n));
    HIPCHK(ctx, hipMemcpyAsync(tmp.p, ctx->d_mmt, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToDevice, ctx->stream));
    int rc = eagle_dev_mmt_normalise(ctx, tmp.as<double>(), n, n, ctx->d_mmt_max, ctx->stream);
    if (rc) return rc;
    if (max_out) HIPCHK(ctx, hipMemcpyAsync(max_out, ctx->d_mmt_max, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return download_big(ctx, MMt_norm_out, tmp.p, sizeof(double) * (size_t)n * n);
}

// ------------------------------------------------------------------------------------------------
// The cached S (SCache, eagle_ctx.h): every read and write of its state is in this section; the rule it follows is s_plan of eagle_host.h.
// S = inv_MMt_sqrt is MMt^-1/2, the same matrix in every call of an AM() run, but R builds it anew each time (no pointer identity, and
// hashing 800 MB costs what copying them costs): the copy of the last call stays on the device, this call computes on it at once, and
// the caller's matrix is compared with it bit for bit while the card works; a difference starts the work over.
// ------------------------------------------------------------------------------------------------
static SPolicy scache_policy() {
    SPolicy p;
    p.no_scache = getenv("EAGLE_HIP_NO_SCACHE") != nullptr;
    if (const char* m = getenv("EAGLE_HIP_SCACHE_MAX_NP")) p.max_np = atol(m);   // (tests force the large-n form at small sizes)
    p.no_host_verify = getenv("EAGLE_HIP_NO_HOST_SVERIFY") != nullptr;
    p.trust_s = getenv("EAGLE_HIP_EXPERIMENT_TRUST_S") != nullptr;
    return p;
}
// any bit of two device arrays different -> *flag != 0 (the cached S against the caller's)
__global__ __launch_bounds__(256) void k_bits_differ(const unsigned long long* __restrict__ a, const unsigned long long* __restrict__ b, long count,
                                                     int* __restrict__ flag) {
    int d = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) d |= a[i] != b[i];
    if (__any(d) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}
// The helper thread's pass over the caller's n x n matrix on the cores that idle while the card works: copied into the host copy (the
// device copy is, or is about to be, this caller's S), or compared with it (measured against the 800 MB upload + device comparison under
// the vara kernel: 3.4 ms of the call's 141.5 at the headline size).
static void scache_host_pass(SCache& c, const double* S_host, long n, bool copy) {
    c.pending = true;
    c.host_differs = 0;
    c.helper = std::thread([&c, S_host, n, copy] {
        std::atomic<int> differs{0};
        parallel_for((long)(sizeof(double) * (size_t)n * (size_t)n), std::max(1, std::min(host_threads(), 16)), [&](long a, long b, int) {
            if (copy) memcpy((char*)c.h_S + a, (const char*)S_host + a, (size_t)(b - a));
            else if (memcmp((const char*)c.h_S + a, (const char*)S_host + a, (size_t)(b - a)) != 0) differs.store(1);
        });
        c.host_differs = differs.load();
        if (copy) c.h_n = n;
    });
}
// The S this call computes on: *Sa stays slot_S, the call's slot at the head of the arena (taken AFTER arena_reserve: the slot record is
// judged at the generation the arena has now), or becomes the device copy.
int SCache::acquire(eagle_ctx* ctx, const SCall& call, const SPolicy& pol, const double* S_host, double* slot_S, double** Sa) {
    const long n = call.n, np = call.np;
    const size_t sq = sizeof(double) * (size_t)np * np, hb = sizeof(double) * (size_t)n * (size_t)n;
    const bool slot_held = s_slot_valid(slot, ctx->arena_gen, (size_t)((char*)slot_S - (char*)ctx->arena), n, np);
    slot = SSlot();   // (valid again only when this scan has gone through)
    helper_rc = EAGLE_OK;
    if (!call.w_direct && np <= pol.max_np && !pol.no_scache && dev_np != np) {
        if (d_S) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(d_S); d_S = nullptr; }
        if (d_scr) { (void)hipFree(d_scr); d_scr = nullptr; }
        dev_n = dev_np = 0;
        if (dev_alloc(&d_S, sq) == hipSuccess && dev_alloc(&d_scr, sq) == hipSuccess) dev_np = np;
        else { if (d_S) (void)hipFree(d_S); d_S = nullptr; (void)hipGetLastError(); }
    }
    plan = s_plan(call, pol, SHeld{dev_np, dev_n, h_S ? h_n : 0, slot_held});
    if (plan.source == S_NONE) return EAGLE_OK;
    const bool cached = plan.source != S_SLOT_VERIFY && plan.source != S_SLOT_UPLOAD;
    if (plan.source == S_CACHE_UPLOAD || plan.source == S_SLOT_UPLOAD) {
        int r = upload_square(ctx, S_host, n, np, cached ? d_S : slot_S);
        if (r) return r;
        h_n = 0;
        s_gen = ctx->w8_s_gen_next++;   // another content where this call's S lies: what the W engine kept with the last one is void
    }
    if (cached) { dev_n = n; *Sa = d_S; }
    if (!plan.refresh_host) return EAGLE_OK;
    // (20 GB at n = 50,000: only when the host has that to spare four times over -- an overcommitted malloc would succeed and the
    // copy then meet the OOM killer; without a host copy the small sizes verify on the device and the large ones upload S every call)
    const long pages = sysconf(_SC_AVPHYS_PAGES), psz = sysconf(_SC_PAGESIZE);
    if (hb > h_cap && pages > 0 && psz > 0 && (double)hb > 0.25 * (double)pages * (double)psz) return EAGLE_OK;
    if (hb > h_cap) { free(h_S); h_S = (double*)malloc(hb); h_cap = h_S ? hb : 0; }
    if (h_S) scache_host_pass(*this, S_host, n, true);   // off the critical path, joined before the call returns
    return EAGLE_OK;
}
// Under the scan: the comparison of the caller's S with the copy the products ran on.  The device form sends the caller's S to the scratch
// copy on the loader stream.  A copy out of PAGEABLE memory blocks the calling thread until the runtime has staged it (14 ms for 800 MB),
// and since the int8 W ends with a host read of its statistics nothing was queued behind it any more: the card sat idle for those 14 ms
// (rocprofv3 timeline of the call, tools/upload_probe.py).  The deferred form is therefore issued from the helper thread while the caller
// goes on queueing the genotype pass and the vara kernel (S's 800 MB at n = 10,000 then hide under the whole scan, not under W alone).
int SCache::begin_verify(eagle_ctx* ctx, const double* S_host, long n, long np) {
    if (plan.verify == SV_NONE) return EAGLE_OK;
    if (plan.verify == SV_HOST) { scache_host_pass(*this, S_host, n, false); return EAGLE_OK; }
    if (!h_flag) {
        const hipError_t e = pin_alloc(&h_flag, 64);
        if (e != hipSuccess) { plan.verify = SV_NONE; return eagle_fail_hip(ctx, e, "pinned flag"); }
    }
    auto compare = [this, ctx, S_host, n, np]() -> int {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        int* flag = (int*)scr_take(ctx, EAGLE_SCR_SCACHE_FLAG);
        HIPCHK(ctx, dev_scratch_handout(d_scr, sizeof(double) * (size_t)np * np));   // (the scratch copy the caller's S is compared in)
        pin_scratch_handout(h_flag, 64);
        *h_flag = 0;
        HIPCHK(ctx, hipMemsetAsync(flag, 0, sizeof(int), ctx->load_stream));
        const int r = upload_square_on(ctx, S_host, n, np, d_scr, ctx->load_stream);
        if (r) return r;
        hipLaunchKernelGGL(k_bits_differ, dim3(1024), dim3(256), 0, ctx->load_stream, (const unsigned long long*)d_scr, (const unsigned long long*)d_S,
                           np * np, flag);
        HIPCHK(ctx, hipMemcpyAsync(h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->load_stream));
        return EAGLE_OK;
    };
    pending = true;
    if (plan.verify == SV_DEVICE_INLINE) return compare();
    helper = std::thread([this, compare] { helper_rc = compare(); });
    return EAGLE_OK;
}
// Collects what acquire / begin_verify started (nothing of the caller's S may be in flight past here) and applies the outcome to the cache.
// rc: the caller's state so far; a failure is returned unchanged.
int SCache::settle(eagle_ctx* ctx, int rc, SOutcome* out) {
    *out = S_NOTHING;
    if (!pending) return rc;
    const SVerify how = plan.verify;
    leave();
    if (helper_rc && !rc) rc = helper_rc;
    hipError_t e = hipStreamSynchronize(ctx->load_stream);
    if (e != hipSuccess && !rc) rc = eagle_fail_hip(ctx, e, "verification of the cached S");
    if (rc || how == SV_NONE) return rc;
    const SOutcome o = s_outcome(how, how == SV_HOST ? host_differs != 0 : *h_flag != 0);
    if (o == S_SAME) hits++;
    else {   // the work so far ran on another S than the caller's
        if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return eagle_fail_hip(ctx, e, "scan on a stale S");
        if (o == S_OTHER_ON_DEVICE) std::swap(d_S, d_scr);
        else dev_n = 0;
        s_gen = ctx->w8_s_gen_next++;
        h_n = 0;
        misses++;
    }
    *out = o;
    return EAGLE_OK;
}
// A scan that went through on S in its arena slot, verified or uploaded by this call: the next scan may find it there.
void SCache::commit(const eagle_ctx* ctx, const double* slot_S, long n, long np) {
    if (plan.source != S_SLOT_VERIFY && plan.source != S_SLOT_UPLOAD) return;
    slot.gen = ctx->arena_gen; slot.off = (size_t)((const char*)slot_S - (const char*)ctx->arena); slot.n = n; slot.np = np;
}
// Every way out of a scan: the helper thread is joined, nothing stays pending.
void SCache::leave() {
    if (helper.joinable()) helper.join();
    pending = false;
    plan.verify = SV_NONE;
}
void SCache::forget_host() { free(h_S); h_S = nullptr; h_n = 0; h_cap = 0; }   // (eagle_drop_cache: 8 n^2 bytes of host memory)
void SCache::release() {   // (eagle_close)
    leave();
    forget_host();
    (void)hipFree(d_S); (void)hipFree(d_scr);   // (null: nothing to free)
    if (h_flag) (void)hipHostFree(h_flag);
}

// what scan_setup reserves for a resident scan of Lr markers on n individuals (the same terms)
static size_t scan_arena_bytes(eagle_ctx* ctx, long n, long Lr) {
    const long np = eagle_pad(n), Lp = eagle_pad(Lr > 0 ? Lr : 1);
    const size_t sq = sizeof(double) * (size_t)np * np;
    const bool use_i8 = scan_use_i8(ctx->scan_mode, np);
    const int nslices = ctx->scan_slices | (ctx->scan_stochastic ? EAGLE_SLICES_STOCHASTIC : 0);
    const size_t wsb = use_i8 ? (size_t)eagle_vara_i8_workspace_bytes(np, Lp, nslices) : 0;
    const size_t certb = use_i8 ? (size_t)eagle_scan_certify_workspace_bytes(np) : 0;
    return 4 * arena_round(sq) + 2 * arena_round(sizeof(double) * np) + arena_round(wsb) + arena_round(certb);
}
static int prepare_scan(eagle_ctx* ctx, long n, long L, bool only_if_roomy) {
    if (!ctx || n <= 0 || L <= 0) return EAGLE_ERR_ARG;
    const int nd = ndev_of(ctx);
    std::vector<long> edge;
    split_markers(L, nd, edge);
    (void)hipSetDevice(ctx->device);
    arena_prefetch(ctx, scan_arena_bytes(ctx, n, edge[1] - edge[0]), only_if_roomy);
    for (size_t k = 0; k < ctx->peers.size(); k++) {
        (void)hipSetDevice(ctx->peers[k]->device);
        arena_prefetch(ctx->peers[k], scan_arena_bytes(ctx->peers[k], n, edge[k + 2] - edge[k + 1]), only_if_roomy);
    }
    (void)hipSetDevice(ctx->device);
    return EAGLE_OK;
}
extern "C" int eagle_prepare_scan(eagle_ctx* ctx, long n, long L) { return prepare_scan(ctx, n, L, false); }

static int ensure_scan_out(eagle_ctx* ctx, long L_pad) {
    if (ctx->scan_cap >= L_pad) return EAGLE_OK;
    if (ctx->d_a) { (void)hipFree(ctx->d_a); ctx->d_a = nullptr; }
    if (ctx->d_vara) { (void)hipFree(ctx->d_vara); ctx->d_vara = nullptr; }
    if (ctx->d_bound) { (void)hipFree(ctx->d_bound); ctx->d_bound = nullptr; }
    ctx->scan_cap = 0;
    HIPCHK(ctx, dev_alloc(&ctx->d_a, sizeof(double) * (size_t)L_pad));
    HIPCHK(ctx, dev_alloc(&ctx->d_vara, sizeof(double) * (size_t)L_pad));
    HIPCHK(ctx, dev_alloc(&ctx->d_bound, sizeof(double) * (size_t)L_pad));
    ctx->scan_cap = L_pad;
    return EAGLE_OK;
}

// ------------------------------------------------------------------------------------------------
// The scan driver.  scan_range makes at most two attempts; an attempt (scan_once) is the sequence of its stages, which stand below in
// the order they run.  Three structs: what the caller passed, this device's share of the call, and what the stages hand on.  The
// modes of an attempt are decided once (scan_plan, eagle_host.h); the stages only read the plan.
// ------------------------------------------------------------------------------------------------
struct ScanArgs {   // what the caller passed: built once in each entry point
    const char* file; long L, n; const std::vector<long>& sel;
    const double *inv_MMt_sqrt, *dim_reduced_vara, *a;   // w_direct (eagle_scan_with_W): W itself, unused, v = S a_hat
    double mem_gb; int quiet; double *a_out, *vara_out; bool w_direct;
};
// this device's share: the markers [m0, m1), device k of nd; rv / rccl: the meeting point and the communicators of a multi-device call (NULL for one device)
struct ScanShare { long m0, m1; int k, nd; Rendezvous* rv; RcclState* rccl; };
struct ScanState {
    long Lr, np, Lp; size_t sq; int nslices;   // markers of the shard; padded individuals, markers (at least a tile); bytes of an np x np operand
    ScanPlan plan;
    GenoEntry* g = nullptr;   // residency: the shard's image (NULL: streamed, or no markers)
    // setup: the carve-up of the arena
    long Lc = 0;              // marker rows per pass
    double *Sa = nullptr, *Va = nullptr, *tmp = nullptr, *Wu = nullptr, *ah = nullptr, *v = nullptr;
    void *ws = nullptr, *cert = nullptr;
    long* cert_totals = nullptr;   // {re-evaluated, flagged, fell back, over the tight threshold}, summed over marker blocks
    ChunkRing ring;
    int8_t *shifted[2] = {}, *cs[2] = {}; int32_t* l1s[2] = {};
    PhaseEvents ph;
    double t0 = 0, t_setup = 0;
    long over_tight_all = 0;  // markers of the whole scan over the tight threshold (CERT_TIGHT_MAX)
};

// One rendezvous round of a multi-device call (rv; NULL: one device, no round).  true: every device is well so far, the attempt goes
// on.  false: leave now with *rc -- this device's failure, or the news that another device failed.  A failed device arrives too: the
// others are waiting for it.
static bool scan_arrive(eagle_ctx* ctx, Rendezvous* rv, int* rc, double v, long add = 0) {
    if (!rv) return *rc == EAGLE_OK;
    if (rv->arrive(*rc == EAGLE_OK, v, add)) return true;
    if (!*rc) *rc = eagle_fail(ctx, EAGLE_ERR_HIP, "another device of the scan failed");
    return false;
}

// Residency: the shard's image in HBM -- there already, or loaded if it fits beside what the scan itself needs -- else *streamed.
static int scan_residency(eagle_ctx* ctx, const ScanArgs& A, const ScanShare& D, ScanState& st, bool* streamed) {
    // operands, digit + certification workspaces (the arena: what this context already holds of it -- from an earlier call or from
    // the background reservation -- is not free memory any more and must not be counted against the file a second time), the
    // re-centred image of the shard
    arena_collect(ctx);
    const bool i8 = scan_use_i8(ctx->scan_mode, st.np);   // (the plan waits for this stage's answer)
    const size_t arena_need = 4 * st.sq + (i8 ? (size_t)eagle_vara_i8_workspace_bytes(st.np, st.Lp, st.nslices) + (size_t)eagle_scan_certify_workspace_bytes(st.np) : 0);
    const int r = get_resident(ctx, A.file, D.m0, st.Lr, 0, A.n, A.mem_gb, host_threads(), &st.g,
                               (arena_need > ctx->arena_cap ? arena_need - ctx->arena_cap : 0) + (i8 ? (size_t)st.Lp * st.np + 9 * (size_t)st.Lp : 0) +
                                   ((size_t)1 << 30));
    *streamed = (r == EAGLE_STREAM);
    return r < 0 ? r : EAGLE_OK;
}

// Setup: the arena carved up, the operands on their way, the S to compute on, room for the results.
static int scan_setup(eagle_ctx* ctx, const ScanArgs& A, const ScanShare& D, ScanState& st, bool s_trusted, const SPolicy& pol) {
    const ScanPlan& P = st.plan;
    const long n = A.n, np = st.np;
    const size_t sq = st.sq;
    const long Lc = st.Lc = P.streamed ? stream_chunk_rows(np, st.Lp) : st.Lp;
    const size_t wsb = P.use_i8 ? (size_t)eagle_vara_i8_workspace_bytes(np, Lc, st.nslices) : 0;
    const size_t certb = P.use_i8 ? (size_t)eagle_scan_certify_workspace_bytes(np) : 0;
    st.cert_totals = (long*)scr_take(ctx, EAGLE_SCR_CERT_TOTALS);
    int r = arena_reserve(ctx, 4 * arena_round(sq) + 2 * arena_round(sizeof(double) * np) + arena_round(wsb) + arena_round(certb) +
                                   (P.streamed ? (P.use_i8 ? 4 : 2) * arena_round((size_t)Lc * np) + 2 * arena_round((size_t)Lc) +
                                                     2 * arena_round(2 * sizeof(int32_t) * (size_t)Lc) : 0));
    if (r) return r;
    st.Sa = arena_take<double>(ctx, sq, s_slot_valid(ctx->scache.slot, ctx->arena_gen, ctx->arena_off, n, np));
    st.Va = arena_take<double>(ctx, sq);
    st.tmp = arena_take<double>(ctx, sq);
    st.Wu = arena_take<double>(ctx, sq);
    st.ah = arena_take<double>(ctx, sizeof(double) * np);
    st.v = arena_take<double>(ctx, sizeof(double) * np);
    st.ws = arena_take<char>(ctx, wsb);
    st.cert = arena_take<char>(ctx, certb);
    st.ph.mark(ctx->stream, PH_START);
    if (P.streamed) {
        if ((r = st.ring.init(ctx))) return r;
        st.ring.buf[0] = arena_take<int8_t>(ctx, (size_t)Lc * np);
        st.ring.buf[1] = arena_take<int8_t>(ctx, (size_t)Lc * np);
        for (int b = 0; b < 2 && P.use_i8; b++) {
            st.shifted[b] = arena_take<int8_t>(ctx, (size_t)Lc * np);
            st.cs[b] = arena_take<int8_t>(ctx, (size_t)Lc);
            st.l1s[b] = arena_take<int32_t>(ctx, 2 * sizeof(int32_t) * (size_t)Lc);
        }
    }
    if (P.w == W_READY) {  // W and v arrive ready: no n^3 work, W goes straight into the buffer the fold works on
        if ((r = upload_square(ctx, A.inv_MMt_sqrt, n, np, st.Wu))) return r;
        if ((r = upload_vec(ctx, A.a, n, np, st.v))) return r;
    } else {
        // V changes with every call; it arrives in row blocks on the loader stream UNDER the first product, which works on the rows
        // that have landed (the W routes) -- unless the rows of W are shared between devices (the row-block product there needs all
        // of V at once).
        if (P.w == W_SHARED && (r = upload_square_staged(ctx, A.dim_reduced_vara, n, np, st.Va, ctx->stream))) return r;
        if ((r = upload_vec(ctx, A.a, n, np, st.ah))) return r;
    }
    // the S to compute on: the cached copy when there is one (the caller's matrix is verified under the products: scan_verify_s), else uploaded
    if ((r = ctx->scache.acquire(ctx, SCall{A.w_direct, s_trusted, n, np, D.rv != nullptr, P.streamed, P.bounds_flow}, pol, A.inv_MMt_sqrt, st.Sa, &st.Sa)))
        return r;
    // streamed: every block is worked as a full chunk of Lc rows (one workspace layout for all of them; the rows beyond a short
    // last block are zero and land in the slack behind the shard's results)
    if ((r = ensure_scan_out(ctx, P.streamed ? (st.Lr + Lc - 1) / Lc * Lc : st.Lp))) return r;
    HIPCHK(ctx, hipMemsetAsync(st.cert_totals, 0, 4 * sizeof(long), ctx->stream));
    st.ph.mark(ctx->stream, PH_UPLOAD);
    return EAGLE_OK;
}

// W = S (V S) and v = S a_hat, one function per route of the plan.
// W_READY: only the fold.
static int scan_w_ready(eagle_ctx* ctx, ScanState& st) { return eagle_dev_fold_upper(ctx, st.Wu, st.np, ctx->stream); }
// W_SHARED: each device computes 1/nd of the rows of W's image (the n^3 part would otherwise not scale) ...
static int scan_w_shared_rows(eagle_ctx* ctx, const ScanArgs& A, const ScanShare& D, ScanState& st) {
    const long rows = st.np / D.nd, r0 = D.k * rows;
    int rc = eagle_dev_scan_operands_rows(ctx, st.Sa, st.Va, st.ah, A.n, st.np, r0, r0 + rows, st.v, st.Wu, st.tmp, ctx->stream);
    hipError_t e;
    if (!rc && (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) rc = eagle_fail_hip(ctx, e, "rows of W");
    return rc;
}
// ... and, once every device has its rows (scan_once's arrival between the two), ONE all-gather completes it everywhere.
static int scan_w_shared_gather(eagle_ctx* ctx, const ScanShare& D, ScanState& st) {
    const long np = st.np, rows = np / D.nd, r0 = D.k * rows;
    const ncclComm_t comm = rccl_comm(D.rccl, D.k);
    ncclResult_t nr = (rccl_fault("allgather", D.k) || !comm) ? ncclSystemError
                                                    : D.rccl->AllGather(st.Wu + r0 * np, st.Wu, (size_t)(rows * np), ncclDouble, comm, ctx->stream);
    if (nr == ncclSuccess) return eagle_dev_fold_upper(ctx, st.Wu, np, ctx->stream);
    const int rc = failf(ctx, EAGLE_ERR_HIP, "ncclAllGather: %s", D.rccl->GetErrorString(nr));
    rccl_abort_all(D.rccl);
    return rc;
}
// W_INT8: W on the int8 engine (csrc/eagle_w8.hip).  Its configuration is chosen from statistics of ALL of V, so V is uploaded whole
// (loader stream; S's statistics and slices do not wait for it); a call that declines runs the fp64 products on the resident operands.
// The upload is pipelined when this context has a configuration to guess (its last call's): V goes up in blocks of 1,536 rows through
// the pinned staging buffers (16 host threads), and each block's statistics, digit slices and columns of the first product run on the
// compute stream as soon as its rows have landed; the finish step keeps that product only if the rule, on the statistics of ALL of V,
// chooses the guessed configuration.  (the cache's verdict on S goes with it: the same verified content as the last call's -- no upload,
// no refresh -- lets the engine keep what it made from S alone; EAGLE_HIP_NO_SCACHE: nobody vouches for S)
static int scan_w_int8(eagle_ctx* ctx, const ScanArgs& A, ScanState& st, const SPolicy& pol) {
    const long n = A.n, np = st.np;
    int rc = EAGLE_OK;
    hipError_t e;
    int r8 = eagle_w8_begin(ctx, st.Sa, st.Va, st.ah, n, np, st.v, st.Wu, st.tmp, 1, pol.no_scache ? 0 : ctx->scache.s_gen, ctx->stream);
    if (r8 < 0) rc = r8;
    if (!rc) {
        const long vb = eagle_w8_vrows_block();
        rc = upload_square_staged(ctx, A.dim_reduced_vara, n, np, st.Va, ctx->load_stream, vb, [&](long r0, long r1, hipEvent_t landed) -> int {
            if (r8) return EAGLE_OK;   // declined at the start (no workspace): only the upload
            hipError_t ew = hipStreamWaitEvent(ctx->stream, landed, 0);
            if (ew != hipSuccess) return eagle_fail_hip(ctx, ew, "row block event");
            const int rv8 = eagle_w8_vrows(ctx, r0, r1, ctx->stream);
            if (rv8 < 0) return rv8;
            if (rv8) r8 = 1;
            return EAGLE_OK;
        });
    }
    if (!rc && !r8) {
        r8 = eagle_w8_finish(ctx, ctx->stream);
        if (r8 < 0) rc = r8;
    }
    if (!rc && r8 == 1) {   // declined: the fp64 products on the operands that are resident now (v is made already)
        hipEvent_t ev = nullptr;
        if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) rc = eagle_fail_hip(ctx, e, "hipEventCreate");
        if (!rc && ((e = hipEventRecord(ev, ctx->load_stream)) != hipSuccess || (e = hipStreamWaitEvent(ctx->stream, ev, 0)) != hipSuccess))
            rc = eagle_fail_hip(ctx, e, "V upload event");
        ctx->w8_active = false;
        if (!rc) rc = eagle_dev_scan_operands_w_f64(ctx, st.Sa, st.Va, np, st.Wu, st.tmp, ctx->stream);
        if (ev) (void)hipEventDestroy(ev);
    }
    if (rc) (void)hipStreamSynchronize(ctx->load_stream);
    return rc;
}
// W_FP64: v = S a_hat at once; then V in blocks of 1024 rows of its image: copy on the loader stream, event, the rows X = V S of
// that block on the compute stream.  PCIe (57 GB/s) delivers a block in half the time its product takes, so all of
// V's upload but the first block hides under the first n^3 product.
static int scan_w_fp64(eagle_ctx* ctx, const ScanArgs& A, ScanState& st) {
    const long n = A.n, np = st.np;
    hipError_t e;
    int rc = eagle_dev_scan_operands_begin(ctx, st.Sa, st.ah, n, np, st.v, st.tmp, ctx->stream);
    if (!rc && (e = hipMemsetAsync(st.Va, 0, st.sq, ctx->load_stream)) != hipSuccess) rc = eagle_fail_hip(ctx, e, "V memset");
    std::vector<hipEvent_t> landed;
    for (long b0 = 0; b0 < np && !rc; b0 += EAGLE_VROWS_BLOCK) {
        const long b1 = std::min(np, b0 + EAGLE_VROWS_BLOCK), hr = std::min(n, b1) - b0;  // rows of the image = columns of the R matrix
        if (hr > 0) {
            e = hipMemcpy2DAsync(st.Va + b0 * np, sizeof(double) * np, A.dim_reduced_vara + b0 * n, sizeof(double) * n, sizeof(double) * n, (size_t)hr,
                                 hipMemcpyHostToDevice, ctx->load_stream);
            if (e != hipSuccess) { rc = eagle_fail_hip(ctx, e, "upload of a row block of V"); break; }
        }
        hipEvent_t ev = nullptr;
        if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) { rc = eagle_fail_hip(ctx, e, "hipEventCreate"); break; }
        landed.push_back(ev);
        if ((e = hipEventRecord(ev, ctx->load_stream)) != hipSuccess || (e = hipStreamWaitEvent(ctx->stream, ev, 0)) != hipSuccess) {
            rc = eagle_fail_hip(ctx, e, "row block event"); break;
        }
        rc = eagle_dev_scan_operands_vrows(ctx, st.Sa, st.Va, np, b0, b1, st.tmp, ctx->stream);
    }
    if (!rc) rc = eagle_dev_scan_operands_finish(ctx, st.Sa, st.Va, np, st.Wu, st.tmp, ctx->stream);
    if (rc) (void)hipStreamSynchronize(ctx->load_stream);  // nothing of the caller's V may still be in flight when we return
    for (hipEvent_t ev : landed) (void)hipEventDestroy(ev);
    return rc;
}

// Verification of S right behind W: the comparison of the caller's matrix with the cached copy the products ran on starts here, and
// where the plan of the cache says so it is settled here too.
static int scan_verify_s(eagle_ctx* ctx, const ScanArgs& A, ScanState& st) {
    SCache& sc = ctx->scache;
    if (sc.plan.verify == SV_NONE) return EAGLE_OK;
    int rc = sc.begin_verify(ctx, A.inv_MMt_sqrt, A.n, st.np);
    // (rv: a device of a multi-device call must not defer -- a peer that streams or holds no cached S settles a changed S inline,
    // and a second attempt of this one would pass every rendezvous of the call a second time)
    if (sc.plan.verify == SV_DEVICE_INLINE) {
        SOutcome o;
        rc = sc.settle(ctx, rc, &o);
        if (!rc && o == S_OTHER_ON_DEVICE) {   // another S, on the device already: the products start over with it
            st.Sa = sc.d_S;
            rc = eagle_dev_scan_operands(ctx, st.Sa, st.Va, st.ah, A.n, st.np, st.v, st.Wu, st.tmp, ctx->stream);
        }
    }
    return rc;
}

// The re-centred image of a resident file for the int8 scan, made by the first such scan of the file and kept with it.
static int ensure_shifted_image(eagle_ctx* ctx, GenoEntry* g, long n, long np) {
    if (g->dev_s) return EAGLE_OK;
    hipError_t e = dev_alloc(&g->dev_s, (size_t)g->rows_pad * g->ld);
    if (e != hipSuccess && eagle_drop_f4_images(ctx) > 0) { (void)hipGetLastError(); e = dev_alloc(&g->dev_s, (size_t)g->rows_pad * g->ld); }
    if (e == hipSuccess) e = dev_alloc(&g->cshift, (size_t)g->rows_pad);
    if (e == hipSuccess) e = dev_alloc(&g->l1, 2 * sizeof(int32_t) * (size_t)g->rows_pad);
    const int rc = e == hipSuccess ? eagle_dev_marker_shift(ctx, g->dev, g->rows_pad, n, np, g->ld, g->dev_s, g->cshift, g->l1, ctx->stream)
                                   : eagle_fail_hip(ctx, e, "re-centred image hipMalloc");
    if (rc) {  // never leave a half-made image behind: the next call would scan garbage
        if (g->dev_s) (void)hipFree(g->dev_s);
        if (g->cshift) (void)hipFree(g->cshift);
        if (g->l1) (void)hipFree(g->l1);
        g->dev_s = nullptr; g->cshift = nullptr; g->l1 = nullptr;
    }
    return rc;
}

// One marker block on the int8 MFMA: b worked as nrp padded rows; slot: which of the two streamed sets of re-centring buffers is free.
static int scan_block_i8(eagle_ctx* ctx, long n, ScanState& st, const MarkerBlock& b, long nrp, int slot) {
    const bool streamed = st.plan.streamed;
    const long np = st.np, r0 = b.r0;
    // re-centred image of the markers (kept with a resident file, rebuilt per chunk when streaming)
    const int8_t *Ms, *cv;
    const int32_t* l1;
    int rc;
    if (streamed) {
        rc = eagle_dev_marker_shift(ctx, b.image, nrp, n, np, b.ld, st.shifted[slot], st.cs[slot], st.l1s[slot], ctx->stream);
        if (rc) return rc;
        Ms = st.shifted[slot]; cv = st.cs[slot]; l1 = st.l1s[slot];
    } else {
        if ((rc = ensure_shifted_image(ctx, st.g, n, np))) return rc;
        Ms = st.g->dev_s; cv = st.g->cshift; l1 = st.g->l1;
    }
    // one pass over the genotypes gives a = Mt v and the diagonal term of vara; then the int8 MFMA kernel
    // (the W-dependent part -- digits of W, rho -- once per scan; per block of a streamed file only the genotype pass)
    rc = eagle_dev_vara_i8_prepare_part(ctx, b.image, nrp, np, b.ld, st.Wu, st.nslices, st.ws, st.v, ctx->d_a + r0, ctx->stream, !streamed ? 0 : (r0 == 0 ? 0 : 2));
    if (rc) return rc;
    st.ph.mark(ctx->stream, PH_PREPARE);
    rc = eagle_dev_vara_i8_mfma_shifted(ctx, Ms, cv, nrp, np, b.ld, st.nslices, st.ws, ctx->d_vara + r0, nullptr, ctx->stream);
    if (rc) return rc;
    // markers that fail their budget under the spectral bound get the dropped digit back (a per-marker decision: the same
    // whatever the blocking; dropped on the device when nobody qualifies)
    rc = eagle_dev_vara_i8_extend(ctx, Ms, cv, l1, b.nr, nrp, np, b.ld, st.nslices, st.ws, ctx->d_vara + r0, ctx->stream);
    if (rc) return rc;
    st.ph.mark(ctx->stream, PH_VARA);
    // a-posteriori certificate: markers the digit bounds cannot settle are re-evaluated by the fp64 kernel, so that
    // which(tsq == max(tsq))[1] on the returned arrays is the marker the fp64 scan selects (find_qtl.R:71-83).  One resident
    // block on one device: bound, selection and re-evaluation right here.  Marker blocks / device shards: only the
    // per-marker bounds now; selection against the global lower bound after the last block (scan_certify_global).
    if (st.plan.bounds_flow)
        return eagle_dev_cert_bounds(ctx, b.nr, nrp, np, cv, l1, st.nslices, st.ws, ctx->d_vara + r0, ctx->d_bound + r0, ctx->stream);
    rc = eagle_dev_scan_certify(ctx, b.image, b.nr, nrp, np, b.ld, cv, l1, st.nslices, st.ws, st.Wu, ctx->d_a + r0, ctx->d_vara + r0, st.cert, ctx->stream);
    if (!rc) rc = eagle_dev_cert_accumulate(ctx, st.cert, st.cert_totals, ctx->stream);
    return rc;
}
// ... and in fp64.
static int scan_block_f64(eagle_ctx* ctx, ScanState& st, const MarkerBlock& b, long nrp) {
    int rc = eagle_dev_gemv_i8(ctx, b.image, nrp, st.np, b.ld, st.v, 1.0, ctx->d_a + b.r0, ctx->stream);
    if (rc) return rc;
    st.ph.mark(ctx->stream, PH_PREPARE);
    rc = eagle_dev_vara_f64(ctx, b.image, nrp, st.np, b.ld, st.Wu, ctx->d_vara + b.r0, ctx->stream);
    if (!rc) st.ph.mark(ctx->stream, PH_VARA);
    return rc;
}
static MarkerBlocks scan_marker_blocks(const ScanArgs& A, const ScanShare& D, const ScanState& st, ChunkRing* ring, bool full_chunks) {
    return MarkerBlocks{A.file, D.m0, st.Lr, A.n, st.np, st.Lc, A.mem_gb, st.g, st.plan.streamed ? ring : nullptr, full_chunks};
}
// The block loop: one pass per marker block -- the whole shard when it is resident, else full chunks of Lc rows read back from the file.
static int scan_blocks(eagle_ctx* ctx, const ScanArgs& A, const ScanShare& D, ScanState& st) {
    const bool streamed = st.plan.streamed;
    if (streamed && !A.quiet) say(ctx, " Mt.ascii streamed through HBM in blocks of %ld markers", st.Lc);
    MarkerBlocks w = scan_marker_blocks(A, D, st, &st.ring, true);
    while (w.more()) {
        MarkerBlock b;
        int rc = w.load(ctx, &b);
        if (rc) return rc;
        if (streamed) st.ph.mark(ctx->stream, PH_LOADWAIT);
        const long nrp = streamed ? st.Lc : eagle_pad(b.nr);
        rc = st.plan.use_i8 ? scan_block_i8(ctx, A.n, st, b, nrp, w.slot()) : scan_block_f64(ctx, st, b, nrp);
        if (rc) return rc;
        if (st.plan.use_i8) st.ph.mark(ctx->stream, PH_CERT);
        if ((rc = w.computed(ctx))) return rc;
    }
    w.finish(ctx);
    return EAGLE_OK;
}

// The global certification of a scan whose bounds flow (plan.bounds_flow): such a scan is certified against ONE lower bound of the
// maximum over every block of every device, so that the candidates, and with them every returned bit, are those of the one-block
// scan of the whole file (the per-marker bounds of all blocks stay: 8 bytes per marker).
// First this shard's lower bound of the maximum tsq and its markers over the tight threshold: the maximum / the sum over the devices
// (scan_once's arrival) decide for all of them.
static int scan_shard_bound(eagle_ctx* ctx, ScanState& st, eagle_cert_info* mine) {
    int rc = eagle_dev_cert_lb_b(ctx, st.Lr, ctx->d_a, ctx->d_vara, ctx->d_bound, st.cert, st.ws, ctx->stream);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(mine, st.cert, sizeof *mine, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e != hipSuccess ? eagle_fail_hip(ctx, e, "lower bound of the shard's maximum") : EAGLE_OK;
}
// More candidates than the re-evaluation buffer holds (degenerate operands): all of the shard in fp64 (on the fp64 products, should W
// have come from the int8 engine).  A streamed shard is read once more, through a second ring that borrows the first one's buffers.
static int scan_redo_f64(eagle_ctx* ctx, const ScanArgs& A, const ScanShare& D, ScanState& st) {
    int rc = eagle_w8_redo_f64(ctx, st.np, ctx->stream);
    if (rc) return rc;
    ChunkRing again;
    if (st.plan.streamed) {
        if ((rc = again.init(ctx))) return rc;
        again.buf[0] = st.ring.buf[0]; again.buf[1] = st.ring.buf[1];
    }
    MarkerBlocks w = scan_marker_blocks(A, D, st, &again, false);
    while (w.more()) {
        MarkerBlock b;
        if ((rc = w.load(ctx, &b))) return rc;
        if ((rc = eagle_dev_vara_f64(ctx, b.image, eagle_pad(b.nr), st.np, b.ld, st.Wu, ctx->d_vara + b.r0, ctx->stream))) return rc;
        if ((rc = w.computed(ctx))) return rc;
    }
    w.finish(ctx);
    return EAGLE_OK;
}
// The fp64 re-evaluation of the cnt candidates.  Streamed: only the candidates' rows are read back from the file (its 2-bit sidecar
// when there is one): typically one or two.
static int scan_reevaluate(eagle_ctx* ctx, const ScanArgs& A, const ScanShare& D, ScanState& st, long cnt) {
    const long np = st.np;
    if (!st.plan.streamed) return eagle_dev_cert_reevaluate(ctx, st.g->dev, st.g->ld, np, st.Wu, ctx->d_vara, st.cert, ctx->stream);
    int rc = EAGLE_OK;
    std::vector<long> idx((size_t)cnt);
    int8_t* rows = eagle_cert_rows(st.cert);
    hipError_t e = hipMemcpyAsync(idx.data(), eagle_cert_indices(st.cert), sizeof(long) * (size_t)cnt, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(rows, 0, (size_t)((cnt + 127) / 128 * 128) * (size_t)np, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = eagle_fail_hip(ctx, e, "candidate list");
    std::vector<RowRun> runs((size_t)cnt);
    for (long c = 0; c < cnt; c++) runs[(size_t)c] = {D.m0 + idx[(size_t)c], 1};
    if (!rc) rc = eagle_load_rows(ctx, A.file, runs, 0, A.n, rows, np, A.mem_gb, 1);
    if (!rc) rc = eagle_dev_cert_reevaluate(ctx, nullptr, np, np, st.Wu, ctx->d_vara, st.cert, ctx->stream);
    return rc;
}
// Then, against the global lower bound glb: selection of this shard's candidates, their re-evaluation (or the redo), the counters.
static int scan_certify_global(eagle_ctx* ctx, const ScanArgs& A, const ScanShare& D, ScanState& st, double glb) {
    eagle_cert_info hd;
    int rc = eagle_dev_cert_select_b(ctx, st.Lr, ctx->d_a, ctx->d_vara, ctx->d_bound, st.cert, glb, st.over_tight_all, st.ws, ctx->stream);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(&hd, st.cert, sizeof hd, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return eagle_fail_hip(ctx, e, "candidate count");
    if (hd.overflow) rc = scan_redo_f64(ctx, A, D, st);
    else if (hd.reevaluated > 0) rc = scan_reevaluate(ctx, A, D, st, hd.reevaluated);
    if (!rc) rc = eagle_dev_cert_accumulate(ctx, st.cert, st.cert_totals, ctx->stream);
    if (!rc) st.ph.mark(ctx->stream, PH_CERT);
    return rc;
}

// Publish: the selected markers zeroed, the results on the host, the figures of the eagle_last_* getters, the arena slot of S.
static int scan_publish(eagle_ctx* ctx, const ScanArgs& A, const ScanShare& D, ScanState& st) {
    const long Lr = st.Lr, m0 = D.m0;
    DevBuf dsel;
    std::vector<long> in_range;
    for (long r : A.sel) if (r >= m0 && r < D.m1) in_range.push_back(r - m0);
    if (!in_range.empty()) {  // :79-84: a zeroed marker row gives a = 0 and vara = 0 exactly
        HIPCHK(ctx, dsel.alloc(sizeof(long) * in_range.size()));
        HIPCHK(ctx, hipMemcpyAsync(dsel.p, in_range.data(), sizeof(long) * in_range.size(), hipMemcpyHostToDevice, ctx->stream));
        const int rc = eagle_dev_zero_rows(ctx, ctx->d_a, ctx->d_vara, Lr, dsel.as<long>(), (long)in_range.size(), 0, ctx->stream);
        if (rc) return rc;
    }
    ctx->scan_L = Lr;
    ctx->scan_first = m0;
    long totals[4] = {0, 0, 0, 0};
    if (Lr > 0) {
        HIPCHK(ctx, hipMemcpyAsync(A.a_out + m0, ctx->d_a, sizeof(double) * (size_t)Lr, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(A.vara_out + m0, ctx->d_vara, sizeof(double) * (size_t)Lr, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(totals, st.cert_totals, sizeof totals, hipMemcpyDeviceToHost, ctx->stream));
    VaraHdr vh = {};   // head of the digit workspace
    if (st.plan.use_i8 && Lr > 0) HIPCHK(ctx, hipMemcpyAsync(&vh, st.ws, sizeof vh, hipMemcpyDeviceToHost, ctx->stream));
    st.ph.mark(ctx->stream, PH_D2H);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->cert_reevaluated = totals[0]; ctx->cert_flagged = totals[1]; ctx->cert_fell_back = totals[2] != 0;
    ctx->scan_digits_used = vh.S; ctx->scan_digits_cut = vh.S_sliced; ctx->scan_specH = vh.specH;
    ctx->scan_budget_used = vh.budget; ctx->scan_bound_level = vh.level; ctx->scan_w_err = vh.wErr;
    // (one resident block counted on the device; blocks / shards: the sum the devices exchanged)
    ctx->cert_over_tight = st.plan.bounds_flow ? st.over_tight_all : totals[3];
    ctx->scan_budget_enforced = ctx->cert_over_tight > eagle_cert_tight_max() ? vh.budget_loose : vh.budget;
    // a scan that took a digit off under the spectral bound and then had to redo a block in fp64: markers of this data set sit
    // outside what the bound covers -- this context keeps the worst-case digit count from now on (eagle_set_scan_budget re-arms)
    if (ctx->cert_fell_back && vh.specH > 0.0) ctx->spectral_off = true;
    st.ph.sum(ctx->scan_phase_ms);
    ctx->scan_blocks = st.plan.streamed ? st.ring.k : 1;
    ctx->scan_host_setup_s = st.t_setup - st.t0;
    ctx->scan_range_wall_s = now_s() - st.t0;
    if (Lr > 0) ctx->scache.commit(ctx, st.Sa, A.n, st.np);
    return EAGLE_OK;
}

// The scan of the markers [m0, m1) of Mt.ascii on ctx's device: a, vara into ctx->d_a / d_vara (and the host ranges
// a_out[m0..m1), vara_out[m0..m1)).  Every device passes the same rendezvous in the same order, failed or not: every arrival of the
// call stands in this function (plan.arrivals of them), and a stage never meets anybody.
// This is ONE attempt (scan_range, below, makes at most two).  pol: the switches of the cached S as read for this call; *redo: S_NOTHING,
// or how the verification settled at the END of the scan found another S than the one it ran on.
// s_trusted: the device copy of S was uploaded from this very caller matrix a moment ago (the second attempt after a deferred
// verification found another S): no verification this time
static int scan_once(eagle_ctx* ctx, const ScanArgs& A, const ScanShare& D, bool s_trusted, const SPolicy& pol, SOutcome* redo) {
    ScanState st;
    st.Lr = D.m1 - D.m0;
    st.np = eagle_pad(A.n);
    st.Lp = eagle_pad(st.Lr > 0 ? st.Lr : 1);
    st.sq = sizeof(double) * (size_t)st.np * st.np;
    st.nslices = ctx->scan_slices | (ctx->scan_stochastic ? EAGLE_SLICES_STOCHASTIC : 0);
    int rc = EAGLE_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) rc = eagle_fail_hip(ctx, e, "hipSetDevice");
    bool streamed = false;
    if (!rc && st.Lr > 0) rc = scan_residency(ctx, A, D, st, &streamed);
    st.plan = scan_plan(ctx->scan_mode, st.np, D.nd, D.rccl != nullptr, D.rv != nullptr, A.w_direct, eagle_w8_wanted(ctx, st.np), streamed);
    const ScanPlan& P = st.plan;
    if (!scan_arrive(ctx, D.rv, &rc, streamed ? 1.0 : 0.0)) return rc;

    SCache& sc = ctx->scache;   // the S of the last call, kept for this one
    struct Left { SCache& c; ~Left() { c.leave(); } } left{sc};   // (its helper thread is joined on every way out)
    st.t0 = now_s();
    rc = scan_setup(ctx, A, D, st, s_trusted, pol);
    st.t_setup = now_s();
    double t1 = 0;
    if (timing_on() && !rc) { (void)hipStreamSynchronize(ctx->stream); t1 = now_s(); }

    if (P.w != W_INT8) { ctx->w8_active = false; ctx->w8_info = W8Info(); ctx->w8_info.declined = 7; }   // (only that route reports on the engine)
    if (P.w == W_SHARED) {
        if (!rc) rc = scan_w_shared_rows(ctx, A, D, st);
        if (!scan_arrive(ctx, D.rv, &rc, 0.0)) return rc;
        rc = scan_w_shared_gather(ctx, D, st);
    } else if (!rc) {
        rc = P.w == W_READY ? scan_w_ready(ctx, st) : P.w == W_INT8 ? scan_w_int8(ctx, A, st, pol) : scan_w_fp64(ctx, A, st);
    }
    if (!rc) rc = scan_verify_s(ctx, A, st);
    if (!rc) st.ph.mark(ctx->stream, PH_W);

    if (!rc) rc = scan_blocks(ctx, A, D, st);

    if (P.bounds_flow) {
        eagle_cert_info mine = {};   // (an empty shard: lower bound 0, nothing over the tight threshold)
        if (!rc && st.Lr > 0) rc = scan_shard_bound(ctx, st, &mine);
        if (!scan_arrive(ctx, D.rv, &rc, mine.lower_bound, (long)mine.over_tight)) return rc;
        const double glb = D.rv ? D.rv->vmax : mine.lower_bound;
        st.over_tight_all = D.rv ? D.rv->vsum : (long)mine.over_tight;
        if (st.Lr > 0) rc = scan_certify_global(ctx, A, D, st, glb);
    }

    SOutcome settled;
    rc = sc.settle(ctx, rc, &settled);   // the deferred outcome of the verification of the cached S
    if (!rc && (settled == S_OTHER_ON_DEVICE || settled == S_OTHER_FORGOTTEN)) { *redo = settled; return EAGLE_OK; }   // ran on the wrong operand: once more (scan_range)
    if (timing_on() && !rc) {
        (void)hipStreamSynchronize(ctx->stream);
        fprintf(stderr, "[eaglehip] scan n=%ld markers [%ld, %ld) of %ld on device %d%s: alloc+upload %.1f ms, device compute %.1f ms\n", A.n, D.m0, D.m1, A.L,
                ctx->device, streamed ? " (streamed)" : "", (t1 - st.t0) * 1e3, (now_s() - t1) * 1e3);
    }
    return rc ? rc : scan_publish(ctx, A, D, st);
}
// The scan, and when its deferred verification finds that the cached S it ran on was not the caller's, a second time on the caller's:
// s_trusted when that S is on the device already (the scratch copy has become the cached one), else with an upload.  The second attempt
// verifies nothing (s_plan), so there is no third.
static int scan_range(eagle_ctx* ctx, const ScanArgs& A, const ScanShare& D) {
    const SPolicy pol = scache_policy();
    SOutcome redo = S_NOTHING;
    const int rc = scan_once(ctx, A, D, false, pol, &redo);
    return !rc && redo != S_NOTHING ? scan_once(ctx, A, D, redo == S_OTHER_ON_DEVICE, pol, &redo) : rc;
}

// After a scan on several devices: the lead reports the certificate counters of all of them, and the spectral_off latch of any is everybody's.
static void merge_peer_scans(eagle_ctx* ctx) {
    for (eagle_ctx* p : ctx->peers) {
        ctx->cert_reevaluated += p->cert_reevaluated; ctx->cert_flagged += p->cert_flagged; ctx->cert_fell_back |= p->cert_fell_back;
        ctx->spectral_off |= p->spectral_off;
        if (!ctx->scan_digits_cut) { ctx->scan_digits_used = p->scan_digits_used; ctx->scan_digits_cut = p->scan_digits_cut; ctx->scan_specH = p->scan_specH; }
    }
    for (eagle_ctx* p : ctx->peers) p->spectral_off = ctx->spectral_off;   // every device of the next scan decides alike
}

extern "C" int eagle_calculate_a_and_vara(eagle_ctx* ctx, const char* f_name_ascii, const double* selected_loci,
                                          long n_selected, const double* inv_MMt_sqrt, const double* dim_reduced_vara,
                                          double max_memory_in_Gbytes, const long dims[2], const double* a, int quiet,
                                          double* a_out, double* vara_out) {
    if (!ctx) return EAGLE_ERR_ARG;
    const long L = dims[0], n = dims[1];
    if (n <= 0 || L <= 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "bad dims");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<long> sel;
    int rc = parse_selected(ctx, selected_loci, n_selected, L, sel);
    if (rc) return rc;
    // calculate_a_and_vara_rcpp.cpp:65 (integer division), :74, :129-144
    double mem_needed = (double)((4UL * (unsigned long)n * (unsigned long)L * sizeof(double)) / 1000000000UL);
    if (!quiet) say(ctx, "Inside internal function calculate_a_and_vara_rcpp: Need memory (gigabytes)  %g", mem_needed);
    if (!(mem_needed < max_memory_in_Gbytes)) {
        say(ctx, " Increasing maxmemGb would improve performance... \n");
        long rows_in_block = (long)(max_memory_in_Gbytes * 1e9 / (double)(4UL * (unsigned long)n * sizeof(double)));
        if (rows_in_block < 0) {
            say(ctx, "\n");  // calculate_a_and_vara_rcpp.cpp:134-139, line for line
            say(ctx, "Error:  availmemGb is set to %g", max_memory_in_Gbytes);
            say(ctx, "        Cannot even read in a single row of data into memory.");
            say(ctx, "        Please increase availmemGb for this data set.");
            say(ctx, "\n");
            say(ctx, " multiple_locus_am has terminated with errors\n");
            a_out[0] = 0.0;
            vara_out[0] = 0.0;
            eagle_fail(ctx, EAGLE_SOFT_SENTINEL, "availmemGb: cannot even read in a single row of data into memory");
            return EAGLE_SOFT_SENTINEL;
        }
        if (rows_in_block == 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "availmemGb too small: zero rows per block");
    }
    const int nd = ndev_of(ctx);
    std::vector<long> edge;
    split_markers(L, nd, edge);
    Rendezvous rv;
    rv.n = nd;
    RcclState* rccl = (RcclState*)ctx->rccl;
    if (rccl && rccl->dead) rccl = nullptr;   // aborted in an earlier call: W on every device, host-staged exchange
    const double t_call = now_s();
    const ScanArgs args = {f_name_ascii, L, n, sel, inv_MMt_sqrt, dim_reduced_vara, a, max_memory_in_Gbytes, quiet, a_out, vara_out, false};
    rc = run_on_devices(ctx, [&](int k, eagle_ctx* c) -> int {
        return scan_range(c, args, ScanShare{edge[k], edge[k + 1], k, nd, nd > 1 || rccl ? &rv : nullptr, rccl});
    });
    ctx->scan_call_wall_s = now_s() - t_call;
    if (rc) return rc;
    merge_peer_scans(ctx);
    return EAGLE_OK;
}

// Optional shortcut for the R side (not one of the reference's .Call symbols): the same scan with W = S V S and v = S a_hat
// handed over ready-made.  Inside AM() they need no n^3 product at all: dim_reduced_vara is Henderson's varG I - C22 =
// varG^2 Ze P Ze with Ze = MMt^1/2 (E/R/calculate_reduced_vara.R:21-35) and inv_MMt_sqrt = Ze^-1, so W = varG^2 P and
// v = S (varG Ze P y) = varG P y (E/R/calculate_reduced_a.R:31) -- and .find_qtl holds P (find_qtl.R:9).  The reference-shaped
// entry point cannot know that (it receives opaque matrices) and spends 24 % of a scan at n = 10,000 on S (V S).
extern "C" int eagle_scan_with_W(eagle_ctx* ctx, const char* f_name_ascii, const double* selected_loci, long n_selected, const double* W,
                                 const double* v, double max_memory_in_Gbytes, const long dims[2], int quiet, double* a_out, double* vara_out) {
    if (!ctx) return EAGLE_ERR_ARG;
    const long L = dims[0], n = dims[1];
    if (n <= 0 || L <= 0 || !W || !v) return eagle_fail(ctx, EAGLE_ERR_ARG, "bad dims / null operand");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<long> sel;
    int rc = parse_selected(ctx, selected_loci, n_selected, L, sel);
    if (rc) return rc;
    const int nd = ndev_of(ctx);
    std::vector<long> edge;
    split_markers(L, nd, edge);
    Rendezvous rv;
    rv.n = nd;
    const ScanArgs args = {f_name_ascii, L, n, sel, W, nullptr, v, max_memory_in_Gbytes, quiet, a_out, vara_out, true};
    rc = run_on_devices(ctx, [&](int k, eagle_ctx* c) -> int {
        return scan_range(c, args, ScanShare{edge[k], edge[k + 1], k, nd, nd > 1 ? &rv : nullptr, nullptr});
    });
    if (rc) return rc;
    merge_peer_scans(ctx);
    return EAGLE_OK;
}

extern "C" int eagle_scan_operand_cache_stats(eagle_ctx* ctx, long* hits, long* misses) {
    if (!ctx) return EAGLE_ERR_ARG;
    long h = ctx->scache.hits, m = ctx->scache.misses;
    for (eagle_ctx* p : ctx->peers) { h += p->scache.hits; m += p->scache.misses; }
    if (hits) *hits = h;
    if (misses) *misses = m;
    return EAGLE_OK;
}
extern "C" int eagle_last_stream_stats(eagle_ctx* ctx, eagle_stream_stats* out) {
    if (!ctx || !out) return EAGLE_ERR_ARG;
    out->chunks = ctx->st_chunks; out->file_bytes = ctx->st_file_bytes;
    out->pread_s = ctx->st_pread_s; out->load_s = ctx->st_load_wall_s; out->wait_s = ctx->st_wait_s;
    out->kernel_s = ctx->st_compute_s; out->wall_s = ctx->st_total_s;
    out->load_first_s = ctx->st_load_first_s; out->starved_s = ctx->st_starved_s;
    return EAGLE_OK;
}
// Where the last eagle_calculate_a_and_vara / eagle_scan_with_W call spent its time on device `device_index` of the context
// (0 = the lead): host seconds until the operand uploads were enqueued, then the phases on that device's compute stream.
extern "C" int eagle_last_scan_timing(eagle_ctx* ctx, int device_index, eagle_scan_timing* out) {
    if (!ctx || !out || device_index < 0 || device_index >= ndev_of(ctx)) return EAGLE_ERR_ARG;
    const eagle_ctx* c = dev_ctx(ctx, device_index);
    out->call_wall_s = ctx->scan_call_wall_s;
    out->device_wall_s = c->scan_range_wall_s;
    out->host_setup_s = c->scan_host_setup_s;
    out->upload_ms = c->scan_phase_ms[PH_UPLOAD];
    out->w_ms = c->scan_phase_ms[PH_W];
    out->load_wait_ms = c->scan_phase_ms[PH_LOADWAIT];
    out->prepare_ms = c->scan_phase_ms[PH_PREPARE];
    out->vara_ms = c->scan_phase_ms[PH_VARA];
    out->certify_ms = c->scan_phase_ms[PH_CERT];
    out->d2h_ms = c->scan_phase_ms[PH_D2H];
    out->blocks = c->scan_blocks;
    out->markers = c->scan_L;
    return EAGLE_OK;
}
extern "C" int eagle_last_scan_certificate(eagle_ctx* ctx, long* n_reevaluated, long* n_flagged, int* fell_back) {
    if (!ctx) return EAGLE_ERR_ARG;
    if (n_reevaluated) *n_reevaluated = ctx->cert_reevaluated;
    if (n_flagged) *n_flagged = ctx->cert_flagged;
    if (fell_back) *fell_back = ctx->cert_fell_back;
    return EAGLE_OK;
}

extern "C" int eagle_last_scan_budget(eagle_ctx* ctx, double* budget_used, int* bound_level, double* w_error_bound) {
    if (!ctx) return EAGLE_ERR_ARG;
    if (budget_used) *budget_used = ctx->scan_budget_used;
    if (bound_level) *bound_level = ctx->scan_bound_level;
    if (w_error_bound) *w_error_bound = ctx->scan_w_err;
    return EAGLE_OK;
}
extern "C" int eagle_last_scan_enforced(eagle_ctx* ctx, double* budget_enforced, long* n_over_tight) {
    if (!ctx) return EAGLE_ERR_ARG;
    if (budget_enforced) *budget_enforced = ctx->scan_budget_enforced;
    if (n_over_tight) *n_over_tight = ctx->cert_over_tight;
    return EAGLE_OK;
}
extern "C" int eagle_set_w_mode(eagle_ctx* ctx, int mode) {
    if (!ctx || mode < 0 || mode > 2) return EAGLE_ERR_ARG;
    ctx->w_mode = mode;
    for (eagle_ctx* p : ctx->peers) p->w_mode = mode;
    return EAGLE_OK;
}
extern "C" int eagle_last_w_info(eagle_ctx* ctx, eagle_w_info* out) {
    if (!ctx || !out) return EAGLE_ERR_ARG;
    const W8Info& i = ctx->w8_info;
    out->int8 = ctx->w8_active ? 1 : 0;
    out->declined = i.declined;
    out->k1 = i.k1; out->T1 = i.T1; out->pairs1 = i.pairs1;
    out->k2 = i.k2; out->T2 = i.T2; out->pairs2 = i.pairs2;
    out->eta = i.eta; out->eta_x = i.eta_x; out->target = i.target; out->mean_diag = i.mean_diag; out->asym_term = i.asym_term;
    out->pipelined = i.pipelined ? 1 : 0; out->pad = 0;
    return EAGLE_OK;
}
extern "C" int eagle_last_scan_digits(eagle_ctx* ctx, int* digits_used, int* digits_cut, double* spectral_bound) {
    if (!ctx) return EAGLE_ERR_ARG;
    if (digits_used) *digits_used = ctx->scan_digits_used;
    if (digits_cut) *digits_cut = ctx->scan_digits_cut;
    if (spectral_bound) *spectral_bound = ctx->scan_specH;
    return EAGLE_OK;
}

extern "C" int eagle_extract_geno(eagle_ctx* ctx, const char* f_name_ascii, double max_memory_in_Gbytes, long selected_locus,
                                  const long dims[2], int* column_out) {
    if (!ctx) return EAGLE_ERR_ARG;
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0 || selected_locus < 0 || selected_locus >= L) return eagle_fail(ctx, EAGLE_ERR_ARG, "bad dims / locus");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    off_t fsize; long mt;
    int rk = eagle_file_key(ctx, f_name_ascii, &fsize, &mt);
    if (rk) return rk;
    for (int k = 0; k < ndev_of(ctx); k++) {  // whichever device holds the marker's column of M.ascii (a shard is a column window)
        eagle_ctx* c = dev_ctx(ctx, k);
        for (auto& g : c->cache)
            if (g.path == f_name_ascii && g.size == fsize && g.mtime_ns == mt && g.row0 == 0 && g.rows == n && selected_locus >= g.col0 &&
                selected_locus < g.col0 + g.cols) {
                HIPCHK(ctx, hipSetDevice(c->device));
                DevBuf col;
                HIPCHK(ctx, col.alloc(sizeof(int) * (size_t)n));
                int rc = eagle_dev_extract_col(c, g.dev, n, g.ld, selected_locus - g.col0, col.as<int>(), c->stream);
                if (rc) return rc;
                HIPCHK(ctx, hipMemcpyAsync(column_out, col.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(ctx, hipStreamSynchronize(c->stream));
                (void)hipSetDevice(ctx->device);
                return EAGLE_OK;
            }
    }
    // not resident: the column through the loader (the file's sidecar, fixed-width text or the line scanner; a view's source)
    DevBuf col;
    HIPCHK(ctx, col.alloc((size_t)n * 16));
    int rc = eagle_dev_load_ascii(ctx, f_name_ascii, 0, n, selected_locus, 1, col.as<int8_t>(), 16, max_memory_in_Gbytes, host_threads());
    if (rc) return rc;
    std::vector<int8_t> h((size_t)n * 16);
    HIPCHK(ctx, hipMemcpyAsync(h.data(), col.p, h.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (long r = 0; r < n; r++) column_out[r] = h[(size_t)r * 16];
    return EAGLE_OK;
}

static int local_scan_argmax(eagle_ctx* ctx, eagle_best* h) {
    h->tsqmax = 0.0; h->index0 = -1; h->near_ties = 0;
    if (!ctx->d_a || ctx->scan_L <= 0) return EAGLE_OK;  // an empty shard
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // ctx-owned workspace: a hipMalloc / hipFree pair per call costs milliseconds in a process that has 100+ GB mapped (measured:
    // 13 ms per find_qtl-shaped call inside bench.py), and hipFree synchronises the device
    if (!ctx->argmax_ws) HIPCHK(ctx, dev_alloc(&ctx->argmax_ws, sizeof(double) * 3 * 1024 + 256));
    else HIPCHK(ctx, dev_scratch_handout(ctx->argmax_ws, sizeof(double) * 3 * 1024 + 256));
    double* scratch = (double*)ctx->argmax_ws;
    eagle_best* best = (eagle_best*)((char*)ctx->argmax_ws + sizeof(double) * 3 * 1024);
    int rc = eagle_dev_tsq_argmax(ctx, ctx->d_a, ctx->d_vara, ctx->scan_L, nullptr, best, scratch, ctx->stream);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(h, best, sizeof *h, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (h->index0 >= 0) h->index0 += ctx->scan_first;  // global marker index
    return EAGLE_OK;
}
extern "C" int eagle_last_scan_argmax(eagle_ctx* ctx, long* index_out, double* tsqmax_out, long* n_near_ties) {
    if (!ctx || !ctx->d_a || (ctx->scan_L <= 0 && ctx->peers.empty())) return eagle_fail(ctx, EAGLE_ERR_ARG, "no scan result held");
    // per-device (max tsq, first index) of the shards, merged on the host: the largest tsq, ties -> the smallest global
    // index = which(tsq == max)[1] (find_qtl.R:76-80)
    eagle_best h;
    int rc = local_scan_argmax(ctx, &h);
    if (rc) return rc;
    for (eagle_ctx* p : ctx->peers) {
        eagle_best o;
        if ((rc = local_scan_argmax(p, &o))) { snprintf(ctx->err, sizeof ctx->err, "%s", p->err); return rc; }
        if (o.index0 < 0) continue;
        const double thr = h.index0 >= 0 ? std::max(h.tsqmax, o.tsqmax) * (1.0 - 1e-9) : 0.0;
        const long near = (h.index0 >= 0 && h.tsqmax >= thr ? h.near_ties : 0) + (o.tsqmax >= thr ? o.near_ties : 0);
        if (h.index0 < 0 || o.tsqmax > h.tsqmax || (o.tsqmax == h.tsqmax && o.index0 < h.index0)) { h.tsqmax = o.tsqmax; h.index0 = o.index0; }
        h.near_ties = near;
    }
    (void)hipSetDevice(ctx->device);
    if (h.index0 < 0) h.tsqmax = __builtin_nan("");
    if (index_out) *index_out = h.index0 + 1;  // R is 1-based; 0 = every tsq was NaN
    if (tsqmax_out) *tsqmax_out = h.tsqmax;
    if (n_near_ties) *n_near_ties = h.near_ties;
    return EAGLE_OK;
}

// ar[m0..m1) = varG * Mt[m0..m1) (P y) on ctx's device (calculate_reduced_a_rcpp.cpp:82-84)
static int reduced_a_range(eagle_ctx* ctx, const char* f_name_ascii, long n, long L, long m0, long m1, const std::vector<long>& sel, double varG,
                           const double* P, const double* y, double max_memory_in_Gbytes, double* ar_out) {
    const long Lr = m1 - m0;
    if (Lr <= 0) return EAGLE_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long np = eagle_pad(n), Lp = eagle_pad(Lr);
    GenoEntry* g = nullptr;
    int rc = get_resident(ctx, f_name_ascii, m0, Lr, 0, n, max_memory_in_Gbytes, host_threads(), &g,
                          sizeof(double) * (size_t)np * np + ((size_t)1 << 30));
    if (rc < 0) return rc;
    const bool streamed = (rc == EAGLE_STREAM);
    const long Lc = streamed ? stream_chunk_rows(np, Lp) : Lp;
    DevBuf Pa, yv, py, out, dsel, chunk;
    HIPCHK(ctx, Pa.alloc(sizeof(double) * (size_t)np * np));
    HIPCHK(ctx, yv.alloc(sizeof(double) * np)); HIPCHK(ctx, py.alloc(sizeof(double) * np));
    HIPCHK(ctx, out.alloc(sizeof(double) * Lp));
    ChunkRing ring;
    if (streamed) {
        HIPCHK(ctx, chunk.alloc((size_t)2 * Lc * np));
        if ((rc = ring.init(ctx))) return rc;
        ring.buf[0] = chunk.as<int8_t>();
        ring.buf[1] = chunk.as<int8_t>() + (size_t)Lc * np;
    }
    if ((rc = upload_square(ctx, P, n, np, Pa.as<double>()))) return rc;
    if ((rc = upload_vec(ctx, y, n, np, yv.as<double>()))) return rc;
    rc = eagle_dev_colgemv(ctx, Pa.as<double>(), n, np, yv.as<double>(), py.as<double>(), ctx->stream);  // :82
    if (rc) return rc;
    MarkerBlocks w{f_name_ascii, m0, Lr, n, np, Lc, max_memory_in_Gbytes, g, streamed ? &ring : nullptr, false};
    while (w.more()) {  // :83-84, one pass per marker block (the whole shard when resident)
        MarkerBlock b;
        if ((rc = w.load(ctx, &b))) return rc;
        rc = eagle_dev_gemv_i8(ctx, b.image, eagle_pad(b.nr), np, b.ld, py.as<double>(), varG, out.as<double>() + b.r0, ctx->stream);
        if (rc) return rc;
        if ((rc = w.computed(ctx))) return rc;
    }
    w.finish(ctx);
    std::vector<long> in_range;
    for (long r : sel) if (r >= m0 && r < m1) in_range.push_back(r - m0);
    if (!in_range.empty()) {  // :74-78
        HIPCHK(ctx, dsel.alloc(sizeof(long) * in_range.size()));
        HIPCHK(ctx, hipMemcpyAsync(dsel.p, in_range.data(), sizeof(long) * in_range.size(), hipMemcpyHostToDevice, ctx->stream));
        rc = eagle_dev_zero_rows(ctx, out.as<double>(), nullptr, Lr, dsel.as<long>(), (long)in_range.size(), 0, ctx->stream);
        if (rc) return rc;
    }
    HIPCHK(ctx, hipMemcpyAsync(ar_out + m0, out.p, sizeof(double) * (size_t)Lr, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

extern "C" int eagle_calculate_reduced_a(eagle_ctx* ctx, const char* f_name_ascii, double varG, const double* P,
                                         const double* y, double max_memory_in_Gbytes, const long dims[2],
                                         const double* selected_loci, long n_selected, int quiet, double* ar_out) {
    if (!ctx) return EAGLE_ERR_ARG;
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "bad dims");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<long> sel;
    int rc = parse_selected(ctx, selected_loci, n_selected, L, sel);
    if (rc) return rc;
    // calculate_reduced_a_rcpp.cpp:56: sizeof(double)/1000000000 is integer 0, so "memory needed" is 0 and the
    // in-memory branch runs iff 0 < availmemGb; otherwise the block size comes out negative (:92-103).
    if (!quiet) {
        say(ctx, "Inside internal function calculate_reduced_a_rcpp. Memory needed (gigabytes): 0");
        say(ctx, "Inside internal function calculate_reduced_a_rcpp. Memory available (gigabytes): %g", max_memory_in_Gbytes);
    }
    if (!(0.0 < max_memory_in_Gbytes)) {
        say(ctx, " Note:  Increasing availmemGb would improve performance... ");
        say(ctx, "\n");  // calculate_reduced_a_rcpp.cpp:95-100, line for line
        say(ctx, "Error:  availmemGb is set to %g", max_memory_in_Gbytes);
        say(ctx, "        Cannot even read in a single row of data into memory.");
        say(ctx, "        Please increase availmemGb for this data set.");
        say(ctx, "\n");
        say(ctx, "AM has terminated with errors\n");
        ar_out[0] = 0.0;
        eagle_fail(ctx, EAGLE_SOFT_SENTINEL, "availmemGb: cannot even read in a single row of data into memory");
        return EAGLE_SOFT_SENTINEL;
    }
    const int nd = ndev_of(ctx);
    std::vector<long> edge;
    split_markers(L, nd, edge);
    return run_on_devices(ctx, [&](int k, eagle_ctx* c) -> int {
        return reduced_a_range(c, f_name_ascii, n, L, edge[k], edge[k + 1], sel, varG, P, y, max_memory_in_Gbytes, ar_out);
    });
}

// ------------------------------------------------------------------------------------------------
// The scan in the eigenbasis of MM^T (include/eagle_hip.h section 1d; kernels and per-device work in eagle_spectral.hip): the
// markers -- and with them Z = Mt U -- split over the devices of the context like everywhere else; no exchange step at all.
// ------------------------------------------------------------------------------------------------
extern "C" int eagle_spectral_prepare(eagle_ctx* ctx, const char* f_name_ascii, const long dims[2], const double* U, double max_memory_in_Gbytes) {
    if (!ctx || !f_name_ascii || !U) return EAGLE_ERR_ARG;
    const long L = dims[0], n = dims[1];
    if (L <= 0 || n <= 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "bad dims");
    const int nd = ndev_of(ctx);
    std::vector<long> edge;
    split_markers(L, nd, edge);
    int rc = run_on_devices(ctx, [&](int k, eagle_ctx* c) -> int {
        return eagle_spectral_prepare_range(c, f_name_ascii, L, n, edge[k], edge[k + 1], U, max_memory_in_Gbytes);
    });
    ctx->spectral_L = rc ? 0 : L;
    return rc;
}
// The one pass / finish / masking sequence behind eagle_spectral_scan and eagle_spectral_scan_weights: d (n_pad, zero padded), G = [Gy | GX]
// (n_pad x NC row-major, zero padded), C (p x p), c1 (p) ready on the host, every device over its shard of Z.
static int spectral_scan_operands(eagle_ctx* ctx, const double* d, const double* G, int NC, const double* Cm, const double* c1, long p, double varG,
                                  const double* selected_loci, long n_selected, double* a_out, double* vara_out) {
    std::vector<long> sel;
    int rc = parse_selected(ctx, selected_loci, n_selected, ctx->spectral_L, sel);
    if (rc) return rc;
    return run_on_devices(ctx, [&](int, eagle_ctx* c) -> int {
        return eagle_spectral_scan_range(c, d, G, NC, Cm, c1, p, varG, sel.data(), (long)sel.size(), a_out, vara_out);
    });
}
extern "C" int eagle_spectral_scan(eagle_ctx* ctx, const double* lambda, const double* UtX, const double* Uty, long p, double varE, double varG,
                                   const double* selected_loci, long n_selected, double* a_out, double* vara_out) {
    if (!ctx || !lambda || !UtX || !Uty || !a_out || !vara_out) return EAGLE_ERR_ARG;
    if (ctx->spectral_L <= 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "spectral_scan: eagle_spectral_prepare has not run");
    if (p < 1 || p > 31) return eagle_fail(ctx, EAGLE_ERR_ARG, "spectral_scan: 1 <= p <= 31 fixed-effect columns");
    const long n = ctx->z_n, np = eagle_pad(n);
    const int NC = p + 1 <= 16 ? 16 : 32;
    std::vector<double> d(np), G((size_t)np * NC), Cm((size_t)p * p), c1(p);
    int rc = eagle_spectral_host_operands(ctx, n, lambda, UtX, Uty, p, varE, varG, NC, d.data(), G.data(), Cm.data(), c1.data());
    if (rc) return rc;
    return spectral_scan_operands(ctx, d.data(), G.data(), NC, Cm.data(), c1.data(), p, varG, selected_loci, n_selected, a_out, vara_out);
}
// The same scan with the operands made by the caller (a model whose C and c1 hold terms lambda and UtX alone do not give).
extern "C" int eagle_spectral_scan_weights(eagle_ctx* ctx, const double* d, const double* Gy, const double* GX, long p, const double* C, const double* c1,
                                           double varG, const double* selected_loci, long n_selected, double* a_out, double* vara_out) {
    if (!ctx || !d || !Gy || !GX || !C || !c1 || !a_out || !vara_out) return EAGLE_ERR_ARG;
    if (ctx->spectral_L <= 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "spectral_scan_weights: eagle_spectral_prepare has not run");
    if (p < 1 || p > 31) return eagle_fail(ctx, EAGLE_ERR_ARG, "spectral_scan_weights: 1 <= p <= 31 fixed-effect columns");
    const long n = ctx->z_n, np = eagle_pad(n);
    const int NC = p + 1 <= 16 ? 16 : 32;
    std::vector<double> dp(np, 0.0), G((size_t)np * NC, 0.0);
    for (long k = 0; k < n; k++) {
        dp[k] = d[k];
        G[(size_t)k * NC] = Gy[k];
        for (long j = 0; j < p; j++) G[(size_t)k * NC + 1 + j] = GX[j * n + k];
    }
    return spectral_scan_operands(ctx, dp.data(), G.data(), NC, C, c1, p, varG, selected_loci, n_selected, a_out, vara_out);
}

// Many traits over one Z (section 1d).  The per-trait host operands (eagle_spectral_host_operands: d_t, G_t, C_t, c1_t; the
// long-double p^2 n loops) run on up to 16 host threads, one trait at a time each; the traits are then packed into column groups
// (spectral_trait_groups, eagle_host.h), each group's columns built once for every device.
extern "C" int eagle_spectral_traits_passes(long T, const long* p) {
    if (T < 1 || !p) return EAGLE_ERR_ARG;
    for (long t = 0; t < T; t++) if (p[t] < 1 || p[t] > 31) return EAGLE_ERR_ARG;
    std::vector<SpectralGroup> groups;
    spectral_trait_groups(T, p, SPT_MAX_TILES, groups);
    return (int)groups.size();
}
extern "C" int eagle_spectral_scan_traits(eagle_ctx* ctx, long T, const double* lambda, const double* const* UtX, const long* p, const double* Uty,
                                          const double* varE, const double* varG, double* a_out, double* vara_out, long* index_out,
                                          double* tsqmax_out) {
    if (!ctx) return EAGLE_ERR_ARG;
    if (ctx->spectral_L <= 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "spectral_scan_traits: eagle_spectral_prepare has not run");
    if (T < 1) return eagle_fail(ctx, EAGLE_ERR_ARG, "spectral_scan_traits: T >= 1 traits");
    if (!lambda || !UtX || !p || !Uty || !varE || !varG || !index_out || (!a_out) != (!vara_out))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "spectral_scan_traits: NULL argument (a_out and vara_out: both or neither)");
    char msg[256];
    for (long t = 0; t < T; t++) {
        if (p[t] < 1 || p[t] > 31) {
            snprintf(msg, sizeof msg, "spectral_scan_traits: trait %ld: 1 <= p <= 31 fixed-effect columns (got %ld)", t + 1, p[t]);
            return eagle_fail(ctx, EAGLE_ERR_ARG, msg);
        }
        if (!UtX[t]) return eagle_fail(ctx, EAGLE_ERR_ARG, "spectral_scan_traits: NULL UtX[t]");
    }
    const long L = ctx->spectral_L, n = ctx->z_n, np = eagle_pad(n);
    std::vector<std::vector<double>> d(T), Gt(T), Cm(T), c1(T);
    std::vector<int> rct(T, 0);
    std::atomic<long> next(0);
    auto work = [&] {
        for (long t; (t = next++) < T;) {
            d[t].resize(np); Gt[t].resize((size_t)np * (p[t] + 1)); Cm[t].resize((size_t)p[t] * p[t]); c1[t].resize(p[t]);
            rct[t] = eagle_spectral_host_operands(nullptr, n, lambda, UtX[t], Uty + t * n, p[t], varE[t], varG[t], (int)(p[t] + 1), d[t].data(),
                                                  Gt[t].data(), Cm[t].data(), c1[t].data());
        }
    };
    {
        std::vector<std::thread> pool;
        for (long w = 1; w < std::min<long>(host_threads(), T); w++) pool.emplace_back(work);
        work();
        for (auto& th : pool) th.join();
    }
    for (long t = 0; t < T; t++)
        if (rct[t]) {  // again on this thread, for the message
            std::vector<double> dd(np), gg((size_t)np * (p[t] + 1)), cc((size_t)p[t] * p[t]), c(p[t]);
            eagle_spectral_host_operands(ctx, n, lambda, UtX[t], Uty + t * n, p[t], varE[t], varG[t], (int)(p[t] + 1), dd.data(), gg.data(), cc.data(), c.data());
            snprintf(msg, sizeof msg, "trait %ld: %s", t + 1, ctx->err);
            return eagle_fail(ctx, rct[t], msg);
        }
    std::vector<SpectralGroup> groups;
    spectral_trait_groups(T, p, SPT_MAX_TILES, groups);
    std::vector<SpectralTraitDesc> desc(T);
    std::vector<double> par;
    std::vector<std::vector<double>> G(groups.size());
    for (size_t k = 0; k < groups.size(); k++) {
        const SpectralGroup& gr = groups[k];
        const long NC = 16L * gr.nt;
        G[k].assign((size_t)np * NC, 0.0);
        int off = 0;
        for (long t = gr.t0; t < gr.t1; t++) {
            const int pt = (int)p[t], qcol = gr.ntl * 16 + (int)(t - gr.t0);
            desc[t] = {off, pt, qcol, (int)t, (long)par.size(), varG[t]};
            par.insert(par.end(), Cm[t].begin(), Cm[t].end());
            par.insert(par.end(), c1[t].begin(), c1[t].end());
            double* Gk = G[k].data();
            for (long r = 0; r < n; r++) {
                memcpy(Gk + r * NC + off, Gt[t].data() + r * (pt + 1), sizeof(double) * (pt + 1));
                Gk[r * NC + qcol] = d[t][r];
            }
            off += pt + 1;
        }
    }
    const int nd = ndev_of(ctx);
    std::vector<std::vector<eagle_best>> best((size_t)nd, std::vector<eagle_best>(T));
    int rc = run_on_devices(ctx, [&](int k, eagle_ctx* c) -> int {
        return eagle_spectral_traits_range(c, T, groups, G, desc.data(), par.data(), (long)par.size(), L, a_out, vara_out, best[k].data());
    });
    if (rc) return rc;
    // the devices' maxima merged: the largest tsq, ties -> the smallest global index (which(tsq == max(tsq))[1], find_qtl.R:76-80)
    for (long t = 0; t < T; t++) {
        double bv = 0.0;
        long bi = -1;
        for (int k = 0; k < nd; k++) {
            const eagle_best& b = best[k][t];
            if (b.index0 >= 0 && (bi < 0 || b.tsqmax > bv || (b.tsqmax == bv && b.index0 < bi))) { bv = b.tsqmax; bi = b.index0; }
        }
        index_out[t] = bi + 1;
        if (tsqmax_out) tsqmax_out[t] = bi >= 0 ? bv : NAN;
    }
    return EAGLE_OK;
}
extern "C" int eagle_spectral_rows(eagle_ctx* ctx, const long* idx, long k, double* out) {
    if (!ctx) return EAGLE_ERR_ARG;
    if (ctx->spectral_L <= 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "spectral_rows: eagle_spectral_prepare has not run");
    if (k < 0 || (k > 0 && (!idx || !out))) return eagle_fail(ctx, EAGLE_ERR_ARG, "spectral_rows: bad arguments");
    for (long j = 0; j < k; j++)
        if (idx[j] < 0 || idx[j] >= ctx->spectral_L) return eagle_fail(ctx, EAGLE_ERR_ARG, "spectral_rows: marker index out of range");
    if (k == 0) return EAGLE_OK;
    return run_on_devices(ctx, [&](int, eagle_ctx* c) -> int { return eagle_spectral_rows_range(c, idx, k, out); });
}
