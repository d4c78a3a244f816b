// eagle_load.cpp -- the genotype file loader of libeaglehip.so: the tile streamer (pread -> pinned -> H2D -> decode), the
// resident genotype cache, and the VIEW aliases of eagle_reshape_m.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "eagle_ctx.h"
#include "eagle_reshape.h"

// ------------------------------------------------------------------------------------------------
// Loader: lines of a no-space ASCII genotype file (or of a VIEW alias of one) -> int8 {-1,0,1} at dst[r*ld + c] in HBM
// (padding untouched; callers zero it).  One ladder of sources (load_plan): the resident image of a view's source, the
// 2-bit sidecar, fixed-width text (every line `width` characters + '\n', pread() straight into pinned memory by `threads`
// workers, double-buffered against the H2D copy + decode kernel: stream_rows), and the host line scanner (scan_lines) for
// text that is not fixed-width after all.
// ------------------------------------------------------------------------------------------------
struct FileInfo {
    int fd = -1;
    off_t size = 0;
    long mtime_ns = 0;
    long width = -1;   // characters per line if fixed-width, else -1
    long nlines = -1;
    ~FileInfo() { if (fd >= 0) close(fd); }
};

static int open_file(eagle_ctx* ctx, const char* path, FileInfo& fi) {
    fi.fd = open(path, O_RDONLY);
    if (fi.fd < 0) return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", path);  // ReadBlock.cpp:42-45
    struct stat st;
    if (fstat(fi.fd, &st) != 0) return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not stat  %s", path);
    fi.size = st.st_size;
    fi.mtime_ns = (long)st.st_mtim.tv_sec * 1000000000L + st.st_mtim.tv_nsec;
    // probe the first line
    char buf[1 << 16];
    long pos = 0, width = -1;
    while (pos < fi.size && width < 0) {
        ssize_t got = pread(fi.fd, buf, sizeof buf, pos);
        if (got <= 0) break;
        void* nl = memchr(buf, '\n', (size_t)got);
        if (nl) width = pos + ((char*)nl - buf);
        pos += got;
    }
    if (width >= 0 && fi.size % (width + 1) == 0) {
        fi.width = width;
        fi.nlines = fi.size / (width + 1);
    } else if (width >= 0 && (fi.size + 1) % (width + 1) == 0) {  // last line without '\n'
        fi.width = width;
        fi.nlines = (fi.size + 1) / (width + 1);
    }
    return EAGLE_OK;
}

static void parallel_pread(int fd, uint8_t* dst, long dst_stride, long nrows, long nbytes, off_t off0, long src_stride,
                           int threads, volatile int* io_err) {
    auto work = [&](long r0, long r1) {
        if (src_stride == dst_stride && nbytes == src_stride) {  // contiguous range
            long total = (r1 - r0) * src_stride, done = 0;
            while (done < total) {
                ssize_t got = pread(fd, dst + r0 * dst_stride + done, (size_t)(total - done), off0 + r0 * src_stride + done);
                if (got <= 0) {  // reading past EOF by the missing final '\n' is fine
                    if (got == 0 && total - done <= 1) { dst[r0 * dst_stride + done] = '\n'; break; }
                    *io_err = 1;
                    return;
                }
                done += got;
            }
            return;
        }
        for (long r = r0; r < r1; r++) {
            long done = 0;
            while (done < nbytes) {
                ssize_t got = pread(fd, dst + r * dst_stride + done, (size_t)(nbytes - done), off0 + r * src_stride + done);
                if (got <= 0) {
                    if (got == 0 && nbytes - done <= 1) { dst[r * dst_stride + done] = '\n'; break; }
                    *io_err = 1;
                    return;
                }
                done += got;
            }
        }
    };
    // a thread per >= 2 MiB of the read, 32 at most: num_cores comes from the caller (R hands detectCores()), and spawning
    // hundreds of threads per 64 MiB staging buffer costs more than the reads
    const long by_size = (nrows * nbytes) >> 21;
    if (threads > 32) threads = 32;
    if (threads > by_size) threads = (int)by_size;
    if (threads <= 1 || nrows < 2 * threads) { work(0, nrows); return; }
    std::vector<std::thread> pool;
    long per = (nrows + threads - 1) / threads;
    for (int t = 0; t < threads; t++) {
        long r0 = t * per, r1 = std::min(nrows, r0 + per);
        if (r0 >= r1) break;
        pool.emplace_back(work, r0, r1);
    }
    for (auto& th : pool) th.join();
}

// Two pinned host buffers + two device buffers of at least `need` bytes each, owned by the ctx (grow-only).
int eagle_stage_ensure(eagle_ctx* ctx, size_t need) {
    if (need <= ctx->stage_cap) {   // handed out again: every caller asks before it stages the first byte of its pass
        for (int b = 0; b < 2; b++) { HIPCHK(ctx, dev_scratch_handout(ctx->stage_raw[b], need)); pin_scratch_handout(ctx->stage_pin[b], need); }
        return EAGLE_OK;
    }
    (void)hipStreamSynchronize(ctx->stream);
    for (int b = 0; b < 2; b++) {
        if (ctx->stage_pin[b]) { (void)hipHostFree(ctx->stage_pin[b]); ctx->stage_pin[b] = nullptr; }
        if (ctx->stage_raw[b]) { (void)hipFree(ctx->stage_raw[b]); ctx->stage_raw[b] = nullptr; }
    }
    ctx->stage_cap = 0;
    for (int b = 0; b < 2; b++) {
        HIPCHK(ctx, pin_alloc(&ctx->stage_pin[b], need));
        HIPCHK(ctx, dev_alloc(&ctx->stage_raw[b], need));
    }
    ctx->stage_cap = need;
    return EAGLE_OK;
}


// The staged reader: rows of nb bytes each, pread into the staging ring at `stride` bytes per row (double-buffered against the H2D
// copy), at most cap_bytes per chunk, and handed to launch(raw, first_row, rows, bad) on ctx->stream.  The rows are the runs
// {source row, count} in order: source row q starts at file offset off0 + q * src_stride, and one run is one pread of consecutive
// rows (split across workers when large).  Returns EAGLE_OK with the number of bad bytes the kernels counted in *nbad,
// LOAD_SHORT_READ when the file ended early, or an error.
enum { LOAD_SHORT_READ = 1 };
template <class Launch>
static int stream_rows(eagle_ctx* ctx, int fd, off_t off0, long src_stride, const std::vector<RowRun>& runs, long nb, long stride, long cap_bytes,
                       int threads, int* nbad, Launch launch) {
    long nrows = 0;
    for (const RowRun& q : runs) nrows += q.count;
    const long chunk_rows = std::max(1L, std::min(nrows, cap_bytes / stride));
    int rc = eagle_stage_ensure(ctx, (size_t)chunk_rows * stride);
    if (rc) return rc;
    // the bad-byte counter lives in the ctx scratch page: a hipMalloc / hipFree per tile would synchronise the device,
    // i.e. wait for the kernels of the previous chunk when the tile is a chunk of a streamed file
    int* const bad = (int*)scr_take(ctx, EAGLE_SCR_LOADER_BAD);
    HIPCHK(ctx, hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
    EventPair done;
    HIPCHK(ctx, done.create());
    volatile int io_err = 0;
    size_t ri = 0;
    long pos = 0, k = 0;  // next row: runs[ri].src_row + pos
    for (long r = 0; r < nrows; r += chunk_rows, k++) {
        const int b = (int)(k & 1);
        const long nr = std::min(chunk_rows, nrows - r);
        if (k >= 2) HIPCHK(ctx, hipEventSynchronize(done.e[b]));  // the copy out of pin[b] two chunks ago has finished
        const double tp = now_s();
        for (long filled = 0; filled < nr && !io_err;) {
            while (runs[ri].count == 0) ri++;
            const long m = std::min(runs[ri].count - pos, nr - filled);
            parallel_pread(fd, (uint8_t*)ctx->stage_pin[b] + filled * stride, stride, m, nb, off0 + (off_t)(runs[ri].src_row + pos) * src_stride,
                           src_stride, threads, &io_err);
            filled += m;
            pos += m;
            if (pos == runs[ri].count) { ri++; pos = 0; }
        }
        ctx->st_pread_s += now_s() - tp;
        ctx->st_file_bytes += nr * nb;
        if (io_err) { (void)hipStreamSynchronize(ctx->stream); return LOAD_SHORT_READ; }
        HIPCHK(ctx, hipMemcpyAsync(ctx->stage_raw[b], ctx->stage_pin[b], (size_t)nr * stride, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipEventRecord(done.e[b], ctx->stream));
        rc = launch((const uint8_t*)ctx->stage_raw[b], r, nr, bad);
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    }
    HIPCHK(ctx, hipMemcpyAsync(nbad, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

// The 2-bit sidecar "<path>.e2b" when there is a valid one for the text file `fi` (made from this very file: same size and mtime)
// that holds `rows` x `cols`: its open file descriptor, header in *h.  Else -1: the caller reads the text.
static int open_sidecar(const char* path, const FileInfo& fi, long rows, long cols, E2bHeader* h) {
    if (!eagle_sidecar_enabled()) return -1;
    const int fd = open((std::string(path) + ".e2b").c_str(), O_RDONLY);
    if (fd < 0) return -1;
    struct stat st;
    if (pread(fd, h, sizeof *h, 0) == (ssize_t)sizeof *h && memcmp(h->magic, "EAGLE2B", 8) == 0 && h->version == 1 && (off_t)h->src_size == fi.size &&
        h->src_mtime_ns == fi.mtime_ns && (uint64_t)rows <= h->rows && (uint64_t)cols <= h->cols && fstat(fd, &st) == 0 &&
        (uint64_t)st.st_size >= sizeof *h + h->rows * h->row_bytes)
        return fd;
    close(fd);
    return -1;
}

// What one load takes: the source lines of `runs` (disjoint, in any order) to consecutive destination rows, and of every line the
// characters [col0, col0 + ncols) or, with a keep-map (an Mt view), the characters keep[col0], ..., keep[col0 + ncols - 1].
struct LoadPlan {
    std::vector<RowRun> runs;
    long nrows = 0, src_rows = 0;                  // rows loaded; lines the source must have
    long col0 = 0, ncols = 0;
    const std::vector<int32_t>* keep = nullptr;    // host keep-map, or nullptr: contiguous characters
    const int32_t* d_keep = nullptr;               // the keep-map in HBM
    long first() const { return keep ? (long)(*keep)[(size_t)col0] : col0; }
    long last() const { return keep ? (long)(*keep)[(size_t)(col0 + ncols - 1)] : col0 + ncols - 1; }
};

// The line scanner, for text that is not fixed-width: one forward getline pass over the file.  The wanted characters of every
// wanted line are gathered on the host into pinned memory and decoded on the device (k_decode_ascii), one staging buffer at a time;
// a line goes to the destination row of its run, so the runs may come in any order.  The first col0 + ncols (keep-map: last() + 1)
// characters of each wanted line are required to exist (the reference indexes past the end of a short line: undefined).
static int scan_lines(eagle_ctx* ctx, int fd, const LoadPlan& p, int8_t* dst, long ld) {
    struct Span { long src, count, dst; };
    std::vector<Span> spans;
    long d = 0;
    for (const RowRun& q : p.runs) { if (q.count) spans.push_back({q.src_row, q.count, d}); d += q.count; }
    std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.src < b.src; });
    FILE* f = fdopen(dup(fd), "r");
    if (!f) return eagle_fail(ctx, EAGLE_ERR_OPEN, "fdopen failed");
    struct FCloser { FILE* f; ~FCloser() { fclose(f); } } fcloser{f};
    rewind(f);
    const long ncols = p.ncols, need = p.last() + 1;
    const long chunk_rows = std::max(1L, std::min(p.nrows, (long)(67108864 / std::max(1L, ncols))));
    int rc = eagle_stage_ensure(ctx, (size_t)chunk_rows * ncols);
    if (rc) return rc;
    char* const pin = (char*)ctx->stage_pin[0];
    uint8_t* const raw = (uint8_t*)ctx->stage_raw[0];
    int* const bad = (int*)scr_take(ctx, EAGLE_SCR_LOADER_BAD);
    HIPCHK(ctx, hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
    long filled = 0, out_row = 0;  // staged rows, destination of the first
    auto flush = [&]() -> int {
        if (filled == 0) return EAGLE_OK;
        HIPCHK(ctx, hipMemcpyAsync(raw, pin, (size_t)filled * ncols, hipMemcpyHostToDevice, ctx->stream));
        int r = eagle_dev_decode_ascii(ctx, raw, filled, ncols, ncols, dst + out_row * ld, ld, bad, ctx->stream);
        if (r) return r;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // single staging buffer
        filled = 0;
        return EAGLE_OK;
    };
    char* line = nullptr;
    size_t cap = 0;
    struct Freer { char** p; ~Freer() { free(*p); } } freer{&line};
    long ln = 0;
    for (const Span& s : spans) {
        for (; ln < s.src + s.count; ln++) {
            ssize_t len = getline(&line, &cap, f);
            if (len < 0) return eagle_fail(ctx, EAGLE_ERR_FORMAT, "file has fewer lines than requested");
            if (ln < s.src) continue;
            while (len > 0 && (line[len - 1] == '\n' || line[len - 1] == '\r')) len--;
            if (len < need) return eagle_fail(ctx, EAGLE_ERR_FORMAT, "line shorter than the requested columns");
            const long to = s.dst + ln - s.src;
            if (filled == chunk_rows || (filled > 0 && to != out_row + filled)) { if ((rc = flush())) return rc; }
            if (filled == 0) out_row = to;
            char* o = pin + filled * ncols;
            if (p.keep) for (long j = 0; j < ncols; j++) o[j] = line[(*p.keep)[(size_t)(p.col0 + j)]];
            else memcpy(o, line + p.col0, (size_t)ncols);
            filled++;
        }
    }
    if ((rc = flush())) return rc;
    int nbad = 0;
    HIPCHK(ctx, hipMemcpyAsync(&nbad, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (nbad) return failf(ctx, EAGLE_ERR_FORMAT, "%d characters outside '0'..'2' in the requested tile", nbad);
    return EAGLE_OK;
}

// How many bytes of genotypes may stay resident per file: EAGLE_HIP_MAX_RESIDENT_GB (tests force the streamed path
// with it), otherwise whatever HBM has free.  Files above it are streamed through HBM in marker chunks.
static size_t resident_budget() {
    const char* e = getenv("EAGLE_HIP_MAX_RESIDENT_GB");
    if (e && *e) return (size_t)(atof(e) * 1e9);
    return (size_t)-1;
}

// Resident genotype tile of a whole file: `rows` lines x first `cols` characters, zero padded to
// [pad128(rows)][pad128(cols)].
// Returns EAGLE_OK (*out set), EAGLE_STREAM (too large: the caller streams marker chunks) or an error.
// reserve_bytes: HBM the caller still needs for operands and workspaces.
static bool file_key(const char* path, off_t* size, long* mtime_ns) {
    struct stat st;
    if (stat(path, &st) != 0) return false;
    *size = st.st_size;
    *mtime_ns = (long)st.st_mtim.tv_sec * 1000000000L + st.st_mtim.tv_nsec;
    return true;
}
// A VIEW alias is keyed by its name and its source's size and mtime; a source that changed since registration fails every
// call on the alias (never stale bits).
static int view_check(eagle_ctx* ctx, const ViewAlias& v) {
    off_t size; long mt;
    if (!file_key(v.src.c_str(), &size, &mt)) return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s (the source of %s)", v.src.c_str(), v.alias.c_str());
    if (size != v.src_size || mt != v.src_mtime_ns)
        return failf(ctx, EAGLE_ERR_FORMAT, "%s changed after the view %s was registered (call eagle_reshape_m again)", v.src.c_str(), v.alias.c_str());
    return EAGLE_OK;
}
int eagle_file_key(eagle_ctx* ctx, const char* path, off_t* size, long* mtime_ns) {
    if (const ViewAlias* v = eagle_view_find(ctx, path)) {
        int rc = view_check(ctx, *v);
        if (rc) return rc;
        *size = v->src_size; *mtime_ns = v->src_mtime_ns;
        return EAGLE_OK;
    }
    return file_key(path, size, mtime_ns) ? EAGLE_OK : failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", path);
}
static void free_entry(GenoEntry& g) {
    if (g.dev) (void)hipFree(g.dev);
    if (g.dev_s) (void)hipFree(g.dev_s);
    if (g.cshift) (void)hipFree(g.cshift);
    if (g.l1) (void)hipFree(g.l1);
    if (g.dev_f4) (void)hipFree(g.dev_f4);
    g.dev = g.dev_s = g.cshift = nullptr; g.l1 = nullptr; g.dev_f4 = nullptr;
}
// Whole-file resident copy (rows lines x cols characters from the origin), current size and mtime.
const GenoEntry* eagle_cache_find(eagle_ctx* ctx, const char* path, long rows, long cols) {
    off_t size; long mt;
    if (eagle_file_key(ctx, path, &size, &mt)) return nullptr;
    for (auto& g : ctx->cache)
        if (g.path == path && g.size == size && g.mtime_ns == mt && g.row0 == 0 && g.col0 == 0 && g.rows == rows && g.cols == cols) return &g;
    return nullptr;
}
// An entry that can serve the window [row0, row0+rows) x [col0, col0+cols): the same window, or an image from the origin that
// holds it as a prefix (all columns and the first `rows` lines, or all lines and the first `cols` characters): what the lead of
// a multi-device context finds when the converters left the whole file resident.
static GenoEntry* cache_find_window(eagle_ctx* ctx, const char* path, off_t size, long mt, long row0, long rows, long col0, long cols) {
    for (auto& g : ctx->cache) {
        if (!(g.path == path && g.size == size && g.mtime_ns == mt)) continue;
        if (g.row0 == row0 && g.col0 == col0 && g.rows == rows && g.cols == cols) return &g;
        if (row0 == 0 && col0 == 0 && g.row0 == 0 && g.col0 == 0 &&
            ((g.cols == cols && g.rows >= rows && rows % 256 == 0) || (g.rows == rows && g.cols >= cols && cols % 256 == 0)))
            return &g;
    }
    return nullptr;
}
static void cache_drop_path(eagle_ctx* ctx, const char* path) {
    for (size_t i = 0; i < ctx->cache.size();)
        if (ctx->cache[i].path == path) {
            free_entry(ctx->cache[i]);
            ctx->cache.erase(ctx->cache.begin() + i);
        } else i++;
}
int eagle_cache_adopt(eagle_ctx* ctx, const char* path, long rows, long cols, long rows_pad, long ld, int8_t* dev) {
    cache_drop_path(ctx, path);
    GenoEntry g;
    int rk = eagle_file_key(ctx, path, &g.size, &g.mtime_ns);
    if (rk) { (void)hipFree(dev); return rk; }
    g.path = path; g.rows = rows; g.cols = cols; g.rows_pad = rows_pad; g.ld = ld; g.dev = dev;
    ctx->cache.push_back(g);
    return EAGLE_OK;
}

// Resident int8 image of the window [row0, row0+rows) x [col0, col0+cols) of a genotype text file, zero padded to
// [pad256(rows)][pad256(cols)] (the whole file: row0 = col0 = 0).
// Returns EAGLE_OK (*out set), EAGLE_STREAM (too large: the caller streams marker chunks) or an error.
// reserve_bytes: HBM the caller still needs for operands and workspaces.
int get_resident(eagle_ctx* ctx, const char* path, long row0, long rows, long col0, long cols, double max_mem_gb, int threads,
                 GenoEntry** out, size_t reserve_bytes) {
    off_t fsize; long mt;
    int rk = eagle_file_key(ctx, path, &fsize, &mt);
    if (rk) return rk;
    if (GenoEntry* hit = cache_find_window(ctx, path, fsize, mt, row0, rows, col0, cols)) { *out = hit; return EAGLE_OK; }
    for (size_t i = 0; i < ctx->cache.size();)  // stale entries of the same path (the file changed) and other windows of it
        if (ctx->cache[i].path == path) { free_entry(ctx->cache[i]); ctx->cache.erase(ctx->cache.begin() + i); } else i++;
    GenoEntry g;
    g.path = path; g.size = fsize; g.mtime_ns = mt; g.rows = rows; g.cols = cols; g.row0 = row0; g.col0 = col0;
    g.rows_pad = eagle_pad(rows); g.ld = eagle_pad(cols);
    size_t bytes = (size_t)g.rows_pad * (size_t)g.ld;
    if (bytes > resident_budget()) return EAGLE_STREAM;
    size_t freeb = 0, totalb = 0;
    HIPCHK(ctx, hipMemGetInfo(&freeb, &totalb));
    if (bytes + reserve_bytes > freeb) {
        drop_cache_local(ctx);
        HIPCHK(ctx, hipMemGetInfo(&freeb, &totalb));
        if (bytes + reserve_bytes > freeb) return EAGLE_STREAM;  // does not fit beside the operands: stream it
    }
    HIPCHK(ctx, dev_alloc(&g.dev, bytes));
    hipError_t e = hipMemsetAsync(g.dev, 0, bytes, ctx->stream);
    if (e != hipSuccess) { (void)hipFree(g.dev); return eagle_fail_hip(ctx, e, "memset"); }
    int rc = eagle_dev_load_ascii(ctx, path, row0, rows, col0, cols, g.dev, g.ld, max_mem_gb, threads);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(g.dev); return rc; }
    ctx->cache.push_back(g);
    *out = &ctx->cache.back();
    return EAGLE_OK;
}

int eagle_get_resident(eagle_ctx* ctx, const char* path, long rows, long cols, double max_mem_gb, int threads, const GenoEntry** out) {
    GenoEntry* g = nullptr;
    int rc = get_resident(ctx, path, 0, rows, 0, cols, max_mem_gb, threads, &g);
    *out = g;
    return rc;
}
int eagle_get_resident_window(eagle_ctx* ctx, const char* path, long row0, long rows, long col0, long cols, double max_mem_gb, int threads,
                              const GenoEntry** out) {
    GenoEntry* g = nullptr;
    int rc = get_resident(ctx, path, row0, rows, col0, cols, max_mem_gb, threads, &g);
    *out = g;
    return rc;
}
size_t eagle_resident_budget() { return resident_budget(); }

// ------------------------------------------------------------------------------------------------
// VIEW aliases of eagle_reshape_m (E/src/ReshapeM_rcpp.cpp): the window [row0, row0+nrows) x [col0, col0+ncols) of the file
// ReshapeM_rcpp would write, made from the source -- the same int8 image, zero padding included, that loading the rewritten
// file gives.  An M view (axis 0) drops lines: its rows become runs of consecutive kept source lines.  An Mt view (axis 1) drops
// characters: a keep-map, with which the kept columns are gathered on the device from the resident image (k_gather_cols_i8), the
// rows of the 2-bit sidecar (k_unpack2b_cols) or fixed-width text (k_decode_ascii_cols), or on the host by the line scanner.
// ------------------------------------------------------------------------------------------------
extern "C" int eagle_dev_decode_ascii_cols(eagle_ctx* ctx, const uint8_t* raw, long stride, const int32_t* map, long base, long rows, long ncols,
                                           long eol, int8_t* out, long ld_out, int* bad_dev, void* stream);
extern "C" int eagle_dev_unpack2b_cols(eagle_ctx* ctx, const uint8_t* raw, long stride, const int32_t* map, long base, long rows, long ncols,
                                       int8_t* out, long ld_out, int* bad_dev, void* stream);

static const GenoEntry* resident_source(eagle_ctx* ctx, const ViewAlias& v, long rows, long cols) {
    for (auto& g : ctx->cache)
        if (g.path == v.src && g.size == v.src_size && g.mtime_ns == v.src_mtime_ns && g.row0 == 0 && g.col0 == 0 && g.dev && g.rows >= rows &&
            g.cols >= cols)
            return &g;
    return nullptr;
}

// The source ladder of every load: the resident image (views only: a plain load must not consult the cache, get_resident builds
// its images through here), the 2-bit sidecar, fixed-width text, the line scanner.  `v`: the view the plan was made for, or
// nullptr; a view window is counted under the source that served it (eagle_view_load_counts).
static int load_plan(eagle_ctx* ctx, const char* src, const LoadPlan& p, const ViewAlias* v, int8_t* dst, long ld, double max_mem_gb,
                     int threads) {
    const long c_first = p.first(), c_last = p.last();
    if (v) {
        if (const GenoEntry* g = resident_source(ctx, *v, p.src_rows, c_last + 1)) {
            long i = 0;
            for (const RowRun& q : p.runs) {
                const int8_t* s = g->dev + q.src_row * g->ld;
                if (p.keep) {
                    int rc = eagle_dev_gather_cols_i8(ctx, s, g->ld, p.d_keep + p.col0, 0, q.count, p.ncols, dst + i * ld, ld, ctx->stream);
                    if (rc) return rc;
                } else {
                    HIPCHK(ctx, hipMemcpy2DAsync(dst + i * ld, (size_t)ld, s + p.col0, (size_t)g->ld, (size_t)p.ncols, (size_t)q.count,
                                                 hipMemcpyDeviceToDevice, ctx->stream));
                }
                i += q.count;
            }
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            ctx->view_loads[EAGLE_VIEW_RESIDENT]++;
            return EAGLE_OK;
        }
    }
    FileInfo fi;
    int rc = open_file(ctx, src, fi);
    if (rc) return rc;
    if (p.nrows == 0 || p.ncols == 0) return EAGLE_OK;
    int nbad = 0;
    E2bHeader h;
    const int sfd = open_sidecar(src, fi, p.src_rows, c_last + 1, &h);
    if (sfd >= 0) {
        struct Closer { int fd; ~Closer() { close(fd); } } closer{sfd};
        const SidecarWindow w = sidecar_window(c_first, c_last, (long)h.cols, (long)h.row_bytes);
        const long stride = (w.nb + 15) / 16 * 16;
        rc = stream_rows(ctx, sfd, (off_t)sizeof h + w.b0, (long)h.row_bytes, p.runs, w.nb, stride, 67108864, threads, &nbad,
                         [&](const uint8_t* raw, long r, long nr, int* bad) {
                             if (p.keep)
                                 return eagle_dev_unpack2b_cols(ctx, raw, stride, p.d_keep + p.col0, 4 * w.b0, nr, p.ncols, dst + r * ld, ld, bad, ctx->stream);
                             return eagle_dev_unpack2b(ctx, raw, nr, p.ncols, stride, w.shift, dst + r * ld, ld, bad, ctx->stream);
                         });
        if (rc == LOAD_SHORT_READ) return eagle_fail(ctx, EAGLE_ERR_FORMAT, "short read from the 2-bit sidecar");
        if (rc) return rc;
        if (nbad) return failf(ctx, EAGLE_ERR_FORMAT, "%d invalid genotype codes in %s.e2b", nbad, src);
        if (v) ctx->view_loads[EAGLE_VIEW_SIDECAR]++;
        return EAGLE_OK;
    }
    if (fi.width >= 0) {
        if (p.src_rows > fi.nlines) return eagle_fail(ctx, EAGLE_ERR_FORMAT, "file has fewer lines than requested");
        if (c_last >= fi.width) return eagle_fail(ctx, EAGLE_ERR_FORMAT, "line shorter than the requested columns");
        // the line end goes along when the window reaches the end of the line (of a view's line: its keep-map spans the whole line)
        const bool at_end = p.keep ? p.col0 + p.ncols == (long)p.keep->size() : c_last + 1 == fi.width;
        const long nb = text_window_bytes(c_first, c_last, fi.width, at_end);
        // staging budget: a quarter of availmemGb per buffer, within [one row, 64 MiB]; the two pinned / device staging
        // buffers live in the ctx (page-locking 100s of MB per call costs more than the copy it feeds).  k_decode_ascii checks
        // the line end only when the stride exceeds the columns: the stride is nb exactly.
        const double budget = max_mem_gb > 0 ? max_mem_gb * 1e9 / 4.0 : 64e6;
        rc = stream_rows(ctx, fi.fd, (off_t)c_first, fi.width + 1, p.runs, nb, nb, (long)std::min(budget, 67108864.0), threads, &nbad,
                         [&](const uint8_t* raw, long r, long nr, int* bad) {
                             if (p.keep)
                                 return eagle_dev_decode_ascii_cols(ctx, raw, nb, p.d_keep + p.col0, c_first, nr, p.ncols, at_end ? fi.width - c_first : -1,
                                                                    dst + r * ld, ld, bad, ctx->stream);
                             return eagle_dev_decode_ascii(ctx, raw, nr, p.ncols, nb, dst + r * ld, ld, bad, ctx->stream);
                         });
        if (rc != EAGLE_OK && rc != LOAD_SHORT_READ) return rc;
        if (rc == EAGLE_OK && nbad == 0) {
            if (v) ctx->view_loads[EAGLE_VIEW_TEXT]++;
            return EAGLE_OK;
        }
        // a short read, a bad character or a misplaced line end: not fixed-width after all (or not a genotype file): the scanner decides
    }
    if (v) ctx->view_loads[EAGLE_VIEW_SCANNER]++;
    return scan_lines(ctx, fi.fd, p, dst, ld);
}

// The lines `runs` (disjoint) of the genotype file or VIEW alias `path`, characters [col0, col0 + ncols), to consecutive rows of dst.
int eagle_load_rows(eagle_ctx* ctx, const char* path, const std::vector<RowRun>& runs, long col0, long ncols, int8_t* dst, long ld,
                    double max_mem_gb, int threads) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LoadPlan p;
    p.col0 = col0; p.ncols = ncols;
    long lines = 0;  // lines of `path` the runs need
    for (const RowRun& q : runs) { p.nrows += q.count; if (q.count) lines = std::max(lines, q.src_row + q.count); }
    const ViewAlias* v = eagle_view_find(ctx, path);
    if (!v) {
        p.runs = runs;
        p.src_rows = lines;
        return load_plan(ctx, path, p, nullptr, dst, ld, max_mem_gb, threads);
    }
    int rc = view_check(ctx, *v);
    if (rc) return rc;
    if (p.nrows == 0 || ncols == 0) return EAGLE_OK;
    if (v->axis == 1) {
        if (lines > v->lines) return eagle_fail(ctx, EAGLE_ERR_FORMAT, "file has fewer lines than requested");
        if (col0 + ncols > (long)v->keep.size()) return eagle_fail(ctx, EAGLE_ERR_FORMAT, "line shorter than the requested columns");
        if (!v->d_keep) {   // made on first use
            HIPCHK(ctx, dev_alloc(&v->d_keep, sizeof(int32_t) * std::max((size_t)1, v->keep.size())));
            HIPCHK(ctx, hipMemcpy(v->d_keep, v->keep.data(), sizeof(int32_t) * v->keep.size(), hipMemcpyHostToDevice));
        }
        p.runs = runs;
        p.src_rows = lines;
        p.keep = &v->keep;
        p.d_keep = v->d_keep;
    } else {
        if (lines > (long)v->keep.size()) return eagle_fail(ctx, EAGLE_ERR_FORMAT, "file has fewer lines than requested");
        for (const RowRun& q : runs) append_keep_runs(v->keep.data() + q.src_row, q.count, p.runs);
        for (const RowRun& q : p.runs) p.src_rows = std::max(p.src_rows, q.src_row + q.count);
    }
    return load_plan(ctx, v->src.c_str(), p, v, dst, ld, max_mem_gb, threads);
}

// public: load a window of a genotype text file into a caller-owned HBM int8 buffer
extern "C" int eagle_dev_load_ascii(eagle_ctx* ctx, const char* path, long row0, long nrows, long col0, long ncols,
                                    int8_t* dst, long ld, double max_mem_gb, int threads) {
    if (!ctx) return EAGLE_ERR_ARG;
    if (row0 < 0 || nrows < 0 || col0 < 0 || ncols < 0 || ld % 4 || ncols > ld) return eagle_fail(ctx, EAGLE_ERR_ARG, "load_ascii: bad window");
    return eagle_load_rows(ctx, path, {{row0, nrows}}, col0, ncols, dst, ld, max_mem_gb, threads);
}

// Lines and the lengths of the first and last line of a text file: from the first line and the size when the file is fixed-width
// (what the loaders assume and verify), else from a line index.
static bool text_shape(const char* path, long* nlines, long* first_len, long* last_len) {
    FileInfo fi;
    if (open_file(nullptr, path, fi)) return false;
    if (fi.width >= 0) { *nlines = fi.nlines; *first_len = *last_len = fi.width; return true; }
    ReshapeMap m;
    if (!m.open_ro(path)) return false;
    LineIndex ix;
    index_lines_buf(m.p, m.size, host_threads(), ix);
    *nlines = ix.nlines();
    *first_len = *nlines > 0 ? (long)(ix.end(0) - ix.begin(0)) : 0;
    *last_len = *nlines > 0 ? (long)(ix.end(*nlines - 1) - ix.begin(*nlines - 1)) : 0;
    return true;
}

static void view_drop(eagle_ctx* c, const std::string& alias) {
    for (size_t i = 0; i < c->views.size();)
        if (c->views[i].alias == alias) {
            if (c->views[i].d_keep) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); (void)hipFree(c->views[i].d_keep); }
            c->views.erase(c->views.begin() + (long)i);
        } else i++;
    if (!c->cache.empty()) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); cache_drop_path(c, alias.c_str()); }
}

extern "C" int eagle_view_load_counts(eagle_ctx* ctx, long counts_out[4]) {
    if (!ctx || !counts_out) return EAGLE_ERR_ARG;
    for (int p = 0; p < 4; p++) {
        counts_out[p] = 0;
        for (int k = 0; k < ndev_of(ctx); k++) counts_out[p] += dev_ctx(ctx, k)->view_loads[p];
    }
    return EAGLE_OK;
}

static int reshape_fail(eagle_ctx* ctx, int code, const char* msg) {
    if (ctx) return eagle_fail(ctx, code, msg);
    snprintf(g_open_err, sizeof g_open_err, "%s", msg);
    return code;
}

extern "C" int eagle_reshape_m(eagle_ctx* ctx, const char* fnameM, const char* fnameMt, const long* indxNA, long nNA, const long dims[2],
                               int mode, long newdims_out[2]) {
    if (!fnameM || !fnameMt || !dims || !newdims_out) return reshape_fail(ctx, EAGLE_ERR_ARG, "ReshapeM: NULL argument");
    if (mode != EAGLE_RESHAPE_FILES && mode != EAGLE_RESHAPE_VIEW) return reshape_fail(ctx, EAGLE_ERR_ARG, "ReshapeM: unknown mode");
    if (mode == EAGLE_RESHAPE_VIEW && !ctx) return reshape_fail(ctx, EAGLE_ERR_ARG, "ReshapeM: a VIEW needs a context");
    std::vector<long> na;
    if (const char* why = reshape_check_na(indxNA, nNA, dims[0], na)) return reshape_fail(ctx, EAGLE_ERR_ARG, why);
    const std::string aM = std::string(fnameM) + "tmp", aMt = std::string(fnameMt) + "tmp";  // ReshapeM_rcpp.cpp:51,94
    if (ctx) {
        if (eagle_view_find(ctx, fnameM) || eagle_view_find(ctx, fnameMt)) return reshape_fail(ctx, EAGLE_ERR_ARG, "ReshapeM: the source is itself a view");
        for (int k = 0; k < ndev_of(ctx); k++) { view_drop(dev_ctx(ctx, k), aM); view_drop(dev_ctx(ctx, k), aMt); }
        (void)hipSetDevice(ctx->device);
    }
    if (mode == EAGLE_RESHAPE_FILES) {
        std::string msg;
        const int rc = reshape_write_files(fnameM, fnameMt, na, host_threads(), newdims_out, msg);
        return rc ? reshape_fail(ctx, rc, msg.c_str()) : EAGLE_OK;
    }
    ViewAlias vm, vt;
    long mlines, mfirst, mlast, tlines, tfirst, tlast;
    if (!file_key(fnameM, &vm.src_size, &vm.src_mtime_ns) || !text_shape(fnameM, &mlines, &mfirst, &mlast))
        return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", fnameM);
    if (!file_key(fnameMt, &vt.src_size, &vt.src_mtime_ns) || !text_shape(fnameMt, &tlines, &tfirst, &tlast))
        return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", fnameMt);
    if (!na.empty() && tlines > 0 && tfirst <= na.back())
        return failf(ctx, EAGLE_ERR_FORMAT, "ReshapeM: the lines of %s are shorter than the largest index of indxNA", fnameMt);
    vm.alias = aM; vm.src = fnameM; vm.axis = 0; vm.keep = reshape_keep_list(mlines, na); vm.lines = (long)vm.keep.size();
    vt.alias = aMt; vt.src = fnameMt; vt.axis = 1; vt.keep = reshape_keep_list(tfirst, na); vt.lines = tlines;
    newdims_out[0] = vm.lines;   // lines written to M (:66-72), length of M's last line (:74)
    newdims_out[1] = mlines > 0 ? mlast : 0;
    for (int k = 0; k < ndev_of(ctx); k++) { dev_ctx(ctx, k)->views.push_back(vm); dev_ctx(ctx, k)->views.push_back(vt); }
    return EAGLE_OK;
}
