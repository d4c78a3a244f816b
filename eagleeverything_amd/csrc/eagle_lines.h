// eagle_lines.h -- the one walker of every pass over the lines of an ingested genotype image (M.ascii, Mt.ascii, their sidecar or a
// VIEW alias), and the gather of a few chosen lines.  The image side's counterpart of BedRing / BedPanel (eagle_ingest.cpp).
#ifndef EAGLE_LINES_H
#define EAGLE_LINES_H
#include <algorithm>
#include <vector>

#include "eagle_ctx.h"

// The `rows` lines of `cols` characters of a genotype file, where they lie when the image is (or can be made) resident, else window by
// window through one buffer.  open() decides the route; the caller then cuts the pass into windows (eagle_host.h's RowWindows: the
// whole image when resident(), else with the capacity of its site, for which stream_rows() is the streamed scans' rule), sizes its
// per-window scratch from their `cap`, and each() runs body(img, lo, nr, c0, c1) per window: img = the rows [lo, lo + nr) at leading
// dimension ld(), the body launches on ctx->stream.  A streamed window is the buffer zeroed, then eagle_dev_load_ascii, so every byte
// beyond the rows and characters loaded is zero.  THE two rules of a window loop live here and nowhere else: a failed load or body
// drains the stream before each() returns (kernels may be queued on buffers of the caller's frame), and the last streamed window has
// finished before the buffer is freed.
struct ImageLines {
    eagle_ctx* ctx = nullptr;
    const char* path = nullptr;
    long rows = 0, cols = 0;
    double mem_gb = 0;
    int threads = 1;
    const GenoEntry* src = nullptr;
    long ld_ = 0;
    // stream_only: never resident; ld_streamed: the leading dimension of a streamed window (0: the 256-padding of a resident image)
    int open(eagle_ctx* c, const char* path_, long rows_, long cols_, double max_mem_gb, bool stream_only = false, long ld_streamed = 0) {
        ctx = c; path = path_; rows = rows_; cols = cols_; mem_gb = max_mem_gb; threads = host_threads();
        const int rc = stream_only ? EAGLE_STREAM : eagle_get_resident(ctx, path, rows, cols, mem_gb, threads, &src);
        if (rc != EAGLE_OK && rc != EAGLE_STREAM) return rc;
        if (rc == EAGLE_STREAM) src = nullptr;
        ld_ = src ? src->ld : (ld_streamed ? ld_streamed : eagle_pad(cols));
        return EAGLE_OK;
    }
    bool resident() const { return src != nullptr; }
    long ld() const { return ld_; }
    long stream_rows() const { return stream_chunk_rows_core(eagle_resident_budget(), ld_, eagle_pad(rows)); }
    // a resident image is one window; else disjoint windows of cap_streamed rows
    RowWindows disjoint(long cap_streamed) const { return row_windows_disjoint(rows, src ? rows : cap_streamed); }
    // buf_rows: the rows of the streamed buffer where they are more than the windows' cap (0: cap)
    template <class Body>
    int each(RowWindows ws, Body body, long buf_rows = 0) {
        const size_t bytes = (size_t)(buf_rows ? buf_rows : ws.cap) * (size_t)ld_;
        DevBuf win;
        if (!src) HIPCHK(ctx, win.alloc(bytes));
        int rc = EAGLE_OK;
        RowWindow w;
        while (!rc && ws.next(w)) {
            const int8_t* img = src ? src->dev + w.lo * ld_ : win.as<int8_t>();
            if (!src) {
                const hipError_t e = hipMemsetAsync(win.p, 0, bytes, ctx->stream);
                rc = e != hipSuccess ? eagle_fail_hip(ctx, e, "hipMemsetAsync")
                                     : eagle_dev_load_ascii(ctx, path, w.lo, w.nr, 0, cols, win.as<int8_t>(), ld_, mem_gb, threads);
            }
            if (!rc) rc = body(img, w.lo, w.nr, w.c0, w.c1);
        }
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        if (!src) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // `win` is freed on return: its last kernel has finished
        return EAGLE_OK;
    }
};

// The k <= 64 chosen lines loci[0 .. k) of an image (repeats allowed) as a 64-row int8 image of its leading dimension, the rows from k
// on zero: k_gather_rows_i8 from the resident image, else from the distinct lines, each read once through eagle_load_rows.  The
// buffers and the host map stay with the caller's frame, which ends with a synchronisation of ctx->stream.
struct LociRows {
    std::vector<int32_t> map;
    DevBuf d_map, B8, uniq_img;
    const int8_t* rows() const { return (const int8_t*)B8.p; }
    int gather(ImageLines& img, const long* loci, long k) {
        eagle_ctx* ctx = img.ctx;
        const long ld = img.ld();
        map.resize((size_t)k);
        HIPCHK(ctx, d_map.alloc(sizeof(int32_t) * 64));
        HIPCHK(ctx, B8.alloc((size_t)64 * ld));
        const int8_t* from = img.resident() ? img.src->dev : nullptr;
        int rc = EAGLE_OK;
        if (from) {
            for (long i = 0; i < k; i++) map[(size_t)i] = (int32_t)loci[i];
        } else {
            std::vector<int32_t> u(loci, loci + k);
            std::sort(u.begin(), u.end());
            u.erase(std::unique(u.begin(), u.end()), u.end());
            for (long i = 0; i < k; i++) map[(size_t)i] = (int32_t)(std::lower_bound(u.begin(), u.end(), (int32_t)loci[i]) - u.begin());
            HIPCHK(ctx, uniq_img.alloc((size_t)64 * ld));
            HIPCHK(ctx, hipMemsetAsync(uniq_img.p, 0, (size_t)64 * ld, ctx->stream));
            std::vector<RowRun> runs;
            append_keep_runs(u.data(), (long)u.size(), runs);
            rc = eagle_load_rows(ctx, img.path, runs, 0, img.cols, uniq_img.as<int8_t>(), ld, img.mem_gb, img.threads);
            from = uniq_img.as<int8_t>();
        }
        if (!rc) {
            const hipError_t e = hipMemcpyAsync(d_map.p, map.data(), sizeof(int32_t) * (size_t)k, hipMemcpyHostToDevice, ctx->stream);
            rc = e != hipSuccess ? eagle_fail_hip(ctx, e, "hipMemcpyAsync")
                                 : eagle_dev_gather_rows_i8(ctx, from, ld, d_map.as<int32_t>(), k, 64, B8.as<int8_t>(), ld, ctx->stream);
        }
        if (rc) (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
};
#endif
