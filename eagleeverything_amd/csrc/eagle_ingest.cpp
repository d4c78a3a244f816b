// eagle_ingest.cpp -- marker-file ingestion next to the hot path: the three host
// text-conversion entry points of the reference's .Call table, rebuilt around the HBM-resident genotype copy.
//
//   eagle_get_row_column ...... E/src/getRowColumn.cpp:20-72
//   eagle_create_M_ascii ...... E/src/createM_ASCII_rcpp.cpp:18-106 -> CreateASCIInospace.cpp:17-163 (text)
//                                                                   -> CreateASCIInospace_PLINK.cpp:16-249 (PLINK ped)
//   eagle_create_Mt_ascii ..... E/src/createMt_ASCII_rcpp.cpp:14-247
//   eagle_create_ascii_from_bed  both of them at once from a PLINK binary .bed file (no counterpart in the reference)
//
// The reference tokenises one line at a time through istringstream, and builds Mt.ascii by re-reading M.ascii once per
// column block.  Here the input is mmap()ed, its lines are indexed and tokenised by `host_threads()` workers straight
// into pinned staging, and everything after tokenisation happens on the device: the PLINK allele table walk (one
// thread per locus, k_plink_code), the genotype decode, the transpose (k_transpose_i8) and the re-encoding of text
// lines (k_encode_ascii).  Both files are written with pwrite() from pinned memory, and -- the point of doing it here --
// the int8 images of M.ascii and Mt.ascii stay resident in HBM under the output paths, so the calculateMMt /
// calculate_a_and_vara calls that follow ReadMarker() never parse a text file at all.
// Messages and return values follow the reference (false -> EAGLE_SOFT_SENTINEL after the messages were sent).
#include <ctype.h>
#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <functional>

#include "eagle_ctx.h"
#include "eagle_lines.h"

extern "C" int eagle_dev_encode_ascii(eagle_ctx* ctx, const int8_t* in, long rows, long cols, long ld_in, uint8_t* out, void* stream);
extern "C" int eagle_dev_plink_code(eagle_ctx* ctx, const uint8_t* chars, long rows, long L, long row0, uint8_t* alleles0,
                                    uint8_t* alleles1, int8_t* out, long ld, unsigned long long* first_err,
                                    unsigned long long* first_missing, void* stream);

namespace {

struct MappedFile {
    int fd = -1;
    const char* p = nullptr;
    size_t size = 0;
    ~MappedFile() {
        if (p && size) munmap((void*)p, size);
        if (fd >= 0) close(fd);
    }
};

bool map_file(const char* path, MappedFile& m) {
    m.fd = open(path, O_RDONLY);
    if (m.fd < 0) return false;
    struct stat st;
    if (fstat(m.fd, &st) != 0) return false;
    m.size = (size_t)st.st_size;
    if (m.size == 0) return true;
    void* p = mmap(nullptr, m.size, PROT_READ, MAP_PRIVATE, m.fd, 0);
    if (p == MAP_FAILED) { m.size = 0; return false; }
    m.p = (const char*)p;
    (void)madvise(p, m.size, MADV_SEQUENTIAL);
    return true;
}

// parallel_for, LineIndex, index_lines_buf, next_token, count_tokens: eagle_host.h (HIP-free, built under the CPU sanitizers)
void index_lines(const MappedFile& m, int threads, LineIndex& ix) { index_lines_buf(m.p, m.size, threads, ix); }

bool pread_all(int fd, char* dst, size_t bytes, off_t off, int threads) {
    std::atomic<bool> ok{true};
    parallel_for((long)bytes, bytes < ((size_t)8 << 20) ? 1 : threads, [&](long a, long b, int) {
        while (a < b) {
            ssize_t r = pread(fd, dst + a, (size_t)(b - a), off + a);
            if (r <= 0) { ok = false; return; }
            a += r;
        }
    });
    return ok;
}

bool pwrite_all(int fd, const char* src, size_t bytes, off_t off, int threads) {
    std::atomic<bool> ok{true};
    parallel_for((long)bytes, bytes < ((size_t)8 << 20) ? 1 : threads, [&](long a, long b, int) {
        while (a < b) {
            ssize_t w = pwrite(fd, src + a, (size_t)(b - a), off + a);
            if (w <= 0) { ok = false; return; }
            a += w;
        }
    });
    return ok;
}

// the reference echoes the head of the input after converting it (CreateASCIInospace.cpp:139-158, _PLINK.cpp:201-235)
void say_head(eagle_ctx* ctx, const MappedFile& m, const LineIndex& ix, long nrows_file, long ncols_file, int maxcols, const char* what) {
    const long nrowsp = std::min(5L, nrows_file);
    const long ncolsp = std::min((long)maxcols, ncols_file);
    say(ctx, " First %ld lines and %ld columns of the %s. ", nrowsp, ncolsp, what);
    for (long r = 0; r < nrowsp && r < ix.nlines(); r++) {
        std::string row;
        const char *p = m.p + ix.begin(r), *e = m.p + ix.end(r), *tok;
        long len;
        for (long c = 0; c < ncolsp && (p = next_token(p, e, &tok, &len)) != nullptr; c++) { row.append(tok, (size_t)len); row.push_back(' '); }
        say(ctx, "%s", row.c_str());
    }
}

// CreateASCIInospace_PLINK.cpp:112-121
void say_missing_alleles(eagle_ctx* ctx) {
    say(ctx, "\n");
    say(ctx, " Warning:  PLINK file contains missing alleles (i.e. 0 or - ) ");
    say(ctx, "           These missing genotypes should be imputed before running Eagle.");
    say(ctx, "           As an approximation, AMpus has set these missing genotypes to heterozygotes. ");
    say(ctx, "           Since Eagle assumes an additive model, heterozygote genotypes do not contribute to the estimation of ");
    say(ctx, "           the additive effects.  ");
    say(ctx, "\n");
}

// createMt_ASCII_rcpp.cpp:227-243
void say_summary(eagle_ctx* ctx, const char* type, const char* f_name, long n, long L, double max_memory_in_Gbytes) {
    say(ctx, "\n\n                    Summary of Marker File  ");
    say(ctx, "                   ~~~~~~~~~~~~~~~~~~~~~~~~   ");
    say(ctx, " File type:                   %s", type ? type : "");
    say(ctx, " Reformatted ASCII file name:  %s", f_name);
    say(ctx, " Number of individuals:        %ld", n);
    say(ctx, " Number of loci:               %ld", L);
    say(ctx, " File size (gigabytes):       %g", 3.5 * (double)n * (double)L * 3.0 / 1000000000.0);  // bits_in_int/8 = 31/8 = 3 (integer division)
    say(ctx, " Available memory (gigabytes): %g", max_memory_in_Gbytes);
    say(ctx, "\n\n");
    say(ctx, " The marker file has been Uploaded");
}

struct RowError {  // first failing row of a chunk (smallest row wins)
    long row = -1;
    int kind = 0;  // 1 unknown token, 2 unequal columns
    long cols = 0;
    std::string token;
};

// Does the whole int8 image (rows_pad x ld) fit beside what is already on the device?
bool fits_resident(size_t bytes) {
    if (bytes > eagle_resident_budget()) return false;
    size_t freeb = 0, totalb = 0;
    if (hipMemGetInfo(&freeb, &totalb) != hipSuccess) return false;
    return bytes + ((size_t)2 << 30) < freeb;
}


// Incremental writer of the 2-bit sidecar "<text file>.e2b" (layout: E2bHeader in eagle_ctx.h).  Rows are packed on the
// device from the int8 image the caller already holds, copied to its own pinned buffers and written with pwrite();
// the header goes in last, with the size and mtime of the finished text file, and the file is renamed into place.
struct SidecarWriter {
    eagle_ctx* ctx = nullptr;
    int fd = -1;
    std::string final_path, tmp_path;
    long rows = 0, cols = 0, row_bytes = 0, cap_rows = 0;
    PinBuf pin[2];
    DevBuf dev[2];
    bool active() const { return fd >= 0; }
    ~SidecarWriter() { abandon(); }
    void abandon() {
        if (fd >= 0) { close(fd); fd = -1; (void)unlink(tmp_path.c_str()); }
    }
    bool open_for(eagle_ctx* c, const char* text_path, long nrows, long ncols, long max_rows_per_call) {
        if (!eagle_sidecar_enabled() || nrows <= 0 || ncols <= 0) return false;
        ctx = c; rows = nrows; cols = ncols; cap_rows = std::max(1L, max_rows_per_call);
        row_bytes = sidecar_row_bytes(ncols);
        final_path = std::string(text_path) + ".e2b";
        tmp_path = final_path + ".tmp";
        (void)unlink(final_path.c_str());  // a sidecar of an older text file of that name must not survive a failed run
        fd = open(tmp_path.c_str(), O_CREAT | O_TRUNC | O_WRONLY, 0644);
        if (fd < 0) return false;
        for (int b = 0; b < 2; b++)
            if (pin[b].alloc((size_t)cap_rows * row_bytes) != hipSuccess || dev[b].alloc((size_t)cap_rows * row_bytes) != hipSuccess) { abandon(); return false; }
        return true;
    }
    // enqueue on the ctx stream: pack `nrows` rows of the int8 tile and copy them to pinned buffer b
    int pack(int b, const int8_t* tile, long nrows, long ld) {
        if (!active() || nrows <= 0) return EAGLE_OK;
        if (nrows > cap_rows) return eagle_fail(ctx, EAGLE_ERR_ARG, "sidecar: chunk larger than announced");
        int rc = eagle_dev_pack2b(ctx, tile, nrows, cols, ld, dev[b].as<uint8_t>(), row_bytes, ctx->stream);
        return rc ? rc : fetch(b, nrows);
    }
    // for a producer that packs the rows itself (k_bed_decode): where rows of chunk b go on the device (null: no sidecar) ...
    uint8_t* packed(int b) { return active() ? dev[b].as<uint8_t>() : nullptr; }
    // ... and, enqueued behind that producer, their copy to pinned buffer b
    int fetch(int b, long nrows) {
        if (!active() || nrows <= 0) return EAGLE_OK;
        if (nrows > cap_rows) return eagle_fail(ctx, EAGLE_ERR_ARG, "sidecar: chunk larger than announced");
        hipError_t e = hipMemcpyAsync(pin[b].p, dev[b].p, (size_t)nrows * row_bytes, hipMemcpyDeviceToHost, ctx->stream);
        return e == hipSuccess ? EAGLE_OK : eagle_fail_hip(ctx, e, "sidecar D2H");
    }
    // after the stream work of pack(b, ...) has completed
    void write(int b, long row0, long nrows, int threads) {
        if (!active() || nrows <= 0) return;
        if (!pwrite_all(fd, (const char*)pin[b].p, (size_t)nrows * row_bytes, (off_t)sizeof(E2bHeader) + (off_t)row0 * row_bytes, threads)) abandon();
    }
    void finish(const char* text_path) {
        if (!active()) return;
        struct stat st;
        if (stat(text_path, &st) != 0) { abandon(); return; }
        E2bHeader h;
        memset(&h, 0, sizeof h);
        memcpy(h.magic, "EAGLE2B", 8);
        h.version = 1;
        h.rows = (uint64_t)rows; h.cols = (uint64_t)cols; h.row_bytes = (uint64_t)row_bytes;
        h.src_size = (uint64_t)st.st_size;
        h.src_mtime_ns = (int64_t)st.st_mtim.tv_sec * 1000000000L + st.st_mtim.tv_nsec;
        const bool ok = pwrite(fd, &h, sizeof h, 0) == (ssize_t)sizeof h && ftruncate(fd, (off_t)sizeof h + (off_t)rows * row_bytes) == 0;
        close(fd);
        fd = -1;
        if (!ok || rename(tmp_path.c_str(), final_path.c_str()) != 0) (void)unlink(tmp_path.c_str());
    }
};

// Write-behind of a text file of `stride` bytes per line and its sidecar, from the pinned staging buffers: the lines of chunk k - 1 go to
// disk under the device work of chunk k.  next(): chunk k, lines [r0, r0 + n), is on its way into pinned buffer b with done.e[b] recorded
// behind it; chunk k - 1 is written now.
struct LinesBehind {
    eagle_ctx* ctx;
    int fd;
    const char* path;
    long stride;
    SidecarWriter& sc;
    EventPair& done;
    int threads;
    long r0 = -1, n = 0;   // the chunk not yet on disk (r0 < 0: none)
    int b = 0;
    int flush() {
        if (r0 < 0) return EAGLE_OK;
        hipError_t e = hipEventSynchronize(done.e[b]);
        if (e != hipSuccess) return eagle_fail_hip(ctx, e, "hipEventSynchronize");
        if (!pwrite_all(fd, (const char*)ctx->stage_pin[b], (size_t)n * stride, (off_t)r0 * stride, threads))
            return failf(ctx, EAGLE_ERR_OPEN, "ERROR: could not write %s", path);
        sc.write(b, r0, n, threads);
        r0 = -1;
        return EAGLE_OK;
    }
    int next(long r0_, long n_, int b_) {
        const int rc = flush();
        r0 = r0_; n = n_; b = b_;
        return rc;
    }
};

}  // namespace

extern "C" int eagle_get_row_column(eagle_ctx* ctx, const char* fname, long dims_out[2]) {
    if (!ctx || !fname || !dims_out) return EAGLE_ERR_ARG;
    if (const ViewAlias* v = eagle_view_find(ctx, fname)) {  // what the file eagle_reshape_m would have written gives
        off_t size; long mt;
        int rc = eagle_file_key(ctx, fname, &size, &mt);
        if (rc) return rc;
        dims_out[0] = v->lines;
        dims_out[1] = 0;
        if (v->lines == 0) return EAGLE_OK;
        FILE* f = fopen(v->src.c_str(), "r");
        if (!f) return failf(ctx, EAGLE_ERR_OPEN, "\n\n ERROR: Could not open  %s\n\n", v->src.c_str());
        char* line = nullptr;
        size_t cap = 0;
        ssize_t len = -1;
        for (long r = 0; r <= (v->axis == 0 ? (long)v->keep[0] : 0L); r++) len = getline(&line, &cap, f);  // the alias's first line
        fclose(f);
        if (len >= 0) {
            std::string first;
            if (v->axis == 0) first.assign(line, (size_t)len);
            else for (int32_t c : v->keep) if (c < len) first.push_back(line[c]);
            dims_out[1] = count_tokens(first.data(), first.data() + first.size());
        }
        free(line);
        return EAGLE_OK;
    }
    MappedFile m;
    if (!map_file(fname, m)) return failf(ctx, EAGLE_ERR_OPEN, "\n\n ERROR: Could not open  %s\n\n", fname);  // getRowColumn.cpp:35-38
    LineIndex ix;
    index_lines(m, host_threads(), ix);
    dims_out[0] = ix.nlines();
    dims_out[1] = ix.nlines() > 0 ? count_tokens(m.p + ix.begin(0), m.p + ix.end(0)) : 0;
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// text genotype file -> M.ascii
// ---------------------------------------------------------------------------------------------------------------
static int create_M_text(eagle_ctx* ctx, const char* fname, const char* asciifname, const char* AA, const char* AB, const char* BB,
                         const char* missing, const long dims[2], int quiet) {
    MappedFile m;
    if (!map_file(fname, m)) {
        say(ctx, "ERROR: Text file could not be opened with filename  %s\n", fname);  // CreateASCIInospace.cpp:42-45
        return EAGLE_SOFT_SENTINEL;
    }
    const int fdout = open(asciifname, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fdout < 0) return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", asciifname);
    struct Closer { int fd; ~Closer() { if (fd >= 0) close(fd); } } closer{fdout};
    if (!quiet) { say(ctx, ""); say(ctx, " Reading text File  "); say(ctx, ""); say(ctx, " Loading file "); }
    const int threads = host_threads();
    LineIndex ix;
    index_lines(m, threads, ix);
    const long nlines = ix.nlines(), L = dims[1], stride = L + 1;
    const size_t lAA = strlen(AA), lAB = strlen(AB), lBB = strlen(BB), lMS = strlen(missing);
    const bool single = lAA == 1 && lAB == 1 && lBB == 1;  // one-character codes: table lookup instead of compares

    const long chunk_rows = std::max(1L, std::min(std::max(nlines, 1L), (long)(67108864 / std::max(1L, stride))));
    int rc = eagle_stage_ensure(ctx, (size_t)chunk_rows * stride);
    if (rc) return rc;
    // resident image of M.ascii, filled as the chunks go by (only when the file is what dims says)
    const long n_pad = eagle_pad(nlines), ld = eagle_pad(L);
    int8_t* dev = nullptr;
    DevBuf bad;
    HIPCHK(ctx, bad.alloc(sizeof(int)));
    HIPCHK(ctx, hipMemsetAsync(bad.p, 0, sizeof(int), ctx->stream));
    if (nlines == dims[0] && nlines > 0 && L > 0 && fits_resident((size_t)n_pad * ld)) {
        if (dev_alloc(&dev, (size_t)n_pad * ld) != hipSuccess) dev = nullptr;
        else HIPCHK(ctx, hipMemsetAsync(dev, 0, (size_t)n_pad * ld, ctx->stream));
    }
    struct DevGuard { int8_t*& p; ~DevGuard() { if (p) (void)hipFree(p); } } guard{dev};
    EventPair done;
    HIPCHK(ctx, done.create());

    RowError err;
    long k = 0;
    for (long r0 = 0; r0 < nlines && err.row < 0; r0 += chunk_rows, k++) {
        const int b = (int)(k & 1);
        const long nr = std::min(chunk_rows, nlines - r0);
        char* buf = (char*)ctx->stage_pin[b];
        if (k >= 2) HIPCHK(ctx, hipEventSynchronize(done.e[b]));
        std::vector<RowError> terr((size_t)threads);
        parallel_for(nr, threads, [&](long a, long e, int t) {
            RowError& my = terr[(size_t)t];
            for (long r = a; r < e; r++) {
                const char *p = m.p + ix.begin(r0 + r), *end = m.p + ix.end(r0 + r), *tok;
                char* out = buf + r * stride;
                long len, i = 0;
                while ((p = next_token(p, end, &tok, &len)) != nullptr) {
                    char c;
                    if (single && len == 1) {
                        const char ch = *tok;
                        if (ch == BB[0]) c = '2';
                        else if (ch == AB[0]) c = '1';
                        else if (ch == AA[0]) c = '0';
                        else if (lMS == 1 && ch == missing[0]) c = '1';
                        else c = 0;
                    } else if ((size_t)len == lBB && memcmp(tok, BB, lBB) == 0) c = '2';        // CreateASCIInospace.cpp:95
                    else if ((size_t)len == lAB && memcmp(tok, AB, lAB) == 0) c = '1';          // :97
                    else if ((size_t)len == lAA && memcmp(tok, AA, lAA) == 0) c = '0';          // :99
                    else if ((size_t)len == lMS && memcmp(tok, missing, lMS) == 0) c = '1';     // :101-103
                    else c = 0;
                    if (!c) { my.row = r0 + r; my.kind = 1; my.token.assign(tok, (size_t)len); return; }
                    if (i < L) out[i] = c;
                    i++;
                }
                if (i != L) { my.row = r0 + r; my.kind = 2; my.cols = i; return; }              // :122-131
                out[L] = '\n';
            }
        });
        for (auto& e : terr)
            if (e.row >= 0 && (err.row < 0 || e.row < err.row)) err = e;
        const long good = err.row < 0 ? nr : err.row - r0;  // rows of this chunk written before the failure
        if (good > 0 && !pwrite_all(fdout, buf, (size_t)good * stride, (off_t)r0 * stride, threads))
            return failf(ctx, EAGLE_ERR_OPEN, "ERROR: could not write %s", asciifname);
        if (dev && err.row < 0) {
            HIPCHK(ctx, hipMemcpyAsync(ctx->stage_raw[b], buf, (size_t)nr * stride, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipEventRecord(done.e[b], ctx->stream));
            rc = eagle_dev_decode_ascii(ctx, (const uint8_t*)ctx->stage_raw[b], nr, L, stride, dev + r0 * ld, ld, bad.as<int>(), ctx->stream);
            if (rc) return rc;
        }
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (err.row >= 0) {
        if (err.kind == 1) {                                                                   // :104-116
            if (strcmp(AB, "NA") == 0) say(ctx, "\n Marker file contains marker genotypes that are different to AA=%s BB=%s", AA, BB);
            else say(ctx, "\n Marker file contains marker genotypes that are different to AA=%s AB=%s BB=%s", AA, AB, BB);
            say(ctx, " For example , %s in row %ld", err.token.c_str(), err.row + 1);
            say(ctx, "\n ReadMarker has terminated with errors\n");
        } else {
            say(ctx, "\n");
            say(ctx, "Error:  Marker text file contains an unequal number of columns per row.  ");
            say(ctx, "        The error has occurred at row %ld which contains %ld but ", err.row + 1, err.cols);
            say(ctx, "        it should contain %ld columns of data. ", L);
            say(ctx, "\n");
            say(ctx, " ReadMarkerData has terminated with errors");
        }
        snprintf(ctx->err, sizeof ctx->err, "createM_ASCII: %s at row %ld", err.kind == 1 ? "unknown genotype token" : "unequal number of columns", err.row + 1);
        return EAGLE_SOFT_SENTINEL;
    }
    say_head(ctx, m, ix, dims[0], dims[1], 12, "marker text  file");
    if (dev) {
        close(closer.fd);
        closer.fd = -1;  // the text file is final: its size and mtime key the sidecar and the cache entry
        SidecarWriter sc;
        if (sc.open_for(ctx, asciifname, nlines, L, chunk_rows)) {
            for (long r0 = 0; r0 < nlines && sc.active(); r0 += chunk_rows) {
                const long nr = std::min(chunk_rows, nlines - r0);
                rc = sc.pack(0, dev + r0 * ld, nr, ld);
                if (rc) return rc;
                HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
                sc.write(0, r0, nr, threads);
            }
            sc.finish(asciifname);
        }
        int8_t* give = dev;
        dev = nullptr;
        return eagle_cache_adopt(ctx, asciifname, nlines, L, n_pad, ld, give);
    }
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// PLINK ped -> M.ascii
// ---------------------------------------------------------------------------------------------------------------
static int create_M_plink(eagle_ctx* ctx, const char* fname, const char* asciifname, const long dims[2], int quiet) {
    MappedFile m;
    if (!map_file(fname, m)) {                                                                  // _PLINK.cpp:38-42
        say(ctx, "ERROR: PLINK ped file could not be opened with filename  %s", fname);
        say(ctx, "ERROR: ReadMarkerData has terminated with errors.  ");
        return EAGLE_SOFT_SENTINEL;
    }
    const int fdout = open(asciifname, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fdout < 0) return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", asciifname);
    struct Closer { int fd; ~Closer() { if (fd >= 0) close(fd); } } closer{fdout};
    const int threads = host_threads();
    LineIndex ix;
    index_lines(m, threads, ix);
    const long nlines = ix.nlines();
    const long ncols_total = dims[1];
    const long L = (long)((ncols_total - 6) / 2.0);                                             // :20
    if (L <= 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "createM_ASCII (PLINK): dims[1] must be 6 + 2 * loci");
    const long in_stride = 2 * L, out_stride = L + 1;
    const long chunk_rows = std::max(1L, std::min(std::max(nlines, 1L), (long)(67108864 / in_stride)));
    int rc = eagle_stage_ensure(ctx, (size_t)chunk_rows * in_stride);
    if (rc) return rc;
    const long n_pad = eagle_pad(nlines), ld = eagle_pad(L);
    const bool keep = nlines > 0 && fits_resident((size_t)n_pad * ld);
    DevBuf image, alleles;
    const long img_rows = keep ? n_pad : eagle_pad(chunk_rows);
    HIPCHK(ctx, image.alloc((size_t)img_rows * ld));
    HIPCHK(ctx, hipMemsetAsync(image.p, 0, (size_t)img_rows * ld, ctx->stream));
    HIPCHK(ctx, alleles.alloc((size_t)2 * L));
    HIPCHK(ctx, hipMemsetAsync(alleles.p, 0, (size_t)2 * L, ctx->stream));
    unsigned long long* flags = (unsigned long long*)scr_take(ctx, EAGLE_SCR_INGEST);   // [0] first third-allele, [1] first missing
    HIPCHK(ctx, hipMemsetAsync(flags, 0xff, 2 * sizeof(unsigned long long), ctx->stream));

    SidecarWriter sc;
    (void)sc.open_for(ctx, asciifname, nlines, L, chunk_rows);
    RowError err;          // unequal number of columns (found on the host)
    unsigned long long h_flags[2] = {~0ull, ~0ull};
    for (long r0 = 0; r0 < nlines; r0 += chunk_rows) {
        const long nr = std::min(chunk_rows, nlines - r0);
        char* cin = (char*)ctx->stage_pin[0];
        std::vector<RowError> terr((size_t)threads);
        parallel_for(nr, threads, [&](long a, long e, int t) {
            RowError& my = terr[(size_t)t];
            for (long r = a; r < e; r++) {
                const char *p = m.p + ix.begin(r0 + r), *end = m.p + ix.end(r0 + r), *tok;
                const long numcols = count_tokens(p, end);                                       // :60-63
                if (numcols != ncols_total) { my.row = r0 + r; my.kind = 2; my.cols = numcols; return; }
                long len;
                for (int i = 0; i <= 5; i++) p = next_token(p, end, &tok, &len);                 // :85-87
                char* out = cin + r * in_stride;
                for (long i = 0; i < in_stride; i++) {                                           // :88-90 one character per read
                    while (p < end && is_ws(*p)) p++;
                    out[i] = p < end ? *p++ : 0;
                }
            }
        });
        for (auto& e : terr)
            if (e.row >= 0 && (err.row < 0 || e.row < err.row)) err = e;
        const long good = err.row < 0 ? nr : err.row - r0;  // rows in front of a malformed line are still coded
        if (good > 0) {
            int8_t* img = image.as<int8_t>() + (keep ? r0 * ld : 0);
            HIPCHK(ctx, hipMemcpyAsync(ctx->stage_raw[0], cin, (size_t)good * in_stride, hipMemcpyHostToDevice, ctx->stream));
            rc = eagle_dev_plink_code(ctx, (const uint8_t*)ctx->stage_raw[0], good, L, r0, alleles.as<uint8_t>(), alleles.as<uint8_t>() + L, img, ld,
                                      flags, flags + 1, ctx->stream);
            if (rc) return rc;
            rc = eagle_dev_encode_ascii(ctx, img, good, L, ld, (uint8_t*)ctx->stage_raw[1], ctx->stream);
            if (rc) return rc;
            HIPCHK(ctx, hipMemcpyAsync(ctx->stage_pin[1], ctx->stage_raw[1], (size_t)good * out_stride, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(h_flags, flags, sizeof h_flags, hipMemcpyDeviceToHost, ctx->stream));
            rc = sc.pack(0, img, good, ld);
            if (rc) return rc;
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            sc.write(0, r0, good, threads);
            long ok_rows = good;
            if (h_flags[0] != ~0ull) ok_rows = (long)(h_flags[0] / (unsigned long long)L) - r0;  // the reference stops inside that row
            if (ok_rows > 0 && !pwrite_all(fdout, (const char*)ctx->stage_pin[1], (size_t)ok_rows * out_stride, (off_t)r0 * out_stride, threads))
                return failf(ctx, EAGLE_ERR_OPEN, "ERROR: could not write %s", asciifname);
        }
        if (err.row >= 0 || h_flags[0] != ~0ull) break;
    }
    const bool allele_err = h_flags[0] != ~0ull;
    const unsigned long long stop = allele_err ? h_flags[0] : (err.row >= 0 ? (unsigned long long)err.row * (unsigned long long)L : ~0ull);
    if (h_flags[1] != ~0ull && h_flags[1] < stop) say_missing_alleles(ctx);                      // :112-121, printed once
    if (allele_err) {                                                                            // :155-161
        const long row = (long)(h_flags[0] / (unsigned long long)L), locus = (long)(h_flags[0] % (unsigned long long)L);
        say(ctx, "\n");
        say(ctx, "Error:  PLINK file cannot contain more than two alleles at a locus.");
        say(ctx, "        The error has occurred at snp locus %ld for individual %ld", locus + 1, row + 1);
        say(ctx, "\n");
        say(ctx, " ReadMarkerData has terminated with errors");
        snprintf(ctx->err, sizeof ctx->err, "createM_ASCII: more than two alleles at locus %ld, individual %ld", locus + 1, row + 1);
        return EAGLE_SOFT_SENTINEL;
    }
    if (err.row >= 0) {                                                                          // :65-74
        say(ctx, "\n");
        say(ctx, "Error:  PLINK file contains an unequal number of columns per row.  ");
        say(ctx, "        The error has occurred at row %ld which contains %ld but ", err.row + 1, err.cols);
        say(ctx, "        it should contain %ld columns of data. ", ncols_total);
        say(ctx, "\n");
        say(ctx, " ReadMarkerData has terminated with errors");
        snprintf(ctx->err, sizeof ctx->err, "createM_ASCII: unequal number of columns at row %ld", err.row + 1);
        return EAGLE_SOFT_SENTINEL;
    }
    say_head(ctx, m, ix, dims[0], dims[1], dims[1] < 25 ? (int)dims[1] : 24, "PLINK ped file");  // :205-214
    close(closer.fd);
    closer.fd = -1;
    sc.finish(asciifname);
    if (keep && nlines == dims[0]) {
        int8_t* give = image.as<int8_t>();
        image.p = nullptr;
        return eagle_cache_adopt(ctx, asciifname, nlines, L, n_pad, ld, give);
    }
    return EAGLE_OK;
}

extern "C" int eagle_create_M_ascii(eagle_ctx* ctx, const char* f_name, const char* f_name_ascii, const char* type, const char* AA,
                                    const char* AB, const char* BB, double max_memory_in_Gbytes, const long dims[2], int quiet,
                                    const char* missing) {
    if (!ctx || !f_name || !f_name_ascii || !type || !dims) return EAGLE_ERR_ARG;
    if (dims[0] < 0 || dims[1] < 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "createM_ASCII: negative dims");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    (void)max_memory_in_Gbytes;  // both memory branches of the reference call the same converter (createM_ASCII_rcpp.cpp:88-95)
    if (strcmp(type, "PLINK") == 0) return create_M_plink(ctx, f_name, f_name_ascii, dims, quiet);
    if (!quiet) say(ctx, " A text file is being assumed as the input data file type. ");         // createM_ASCII_rcpp.cpp:85-86
    if (!AA || !AB || !BB || !missing) return eagle_fail(ctx, EAGLE_ERR_ARG, "createM_ASCII: AA, AB, BB and missing must be strings");
    return create_M_text(ctx, f_name, f_name_ascii, AA, AB, BB, missing, dims, quiet);
}

// ---------------------------------------------------------------------------------------------------------------
// M.ascii -> Mt.ascii
// ---------------------------------------------------------------------------------------------------------------
extern "C" int eagle_create_Mt_ascii(eagle_ctx* ctx, const char* f_name, const char* f_name_ascii, const char* type,
                                     double max_memory_in_Gbytes, const long dims[2], int quiet) {
    if (!ctx || !f_name || !f_name_ascii || !dims) return EAGLE_ERR_ARG;
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "createMt_ASCII: dims must be positive");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int threads = host_threads();
    const int fdout = open(f_name_ascii, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fdout < 0) return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", f_name_ascii);
    struct Closer { int fd; ~Closer() { if (fd >= 0) close(fd); } } closer{fdout};
    const long out_stride = n + 1;
    if (ftruncate(fdout, (off_t)L * out_stride) != 0) return failf(ctx, EAGLE_ERR_OPEN, "ERROR: could not size %s", f_name_ascii);

    // source: the resident image of M.ascii (left by eagle_create_M_ascii or an earlier call), else column windows of the file
    const GenoEntry* src = nullptr;
    int rc = eagle_get_resident(ctx, f_name, n, L, max_memory_in_Gbytes, threads, &src);
    if (rc != EAGLE_OK && rc != 2) return rc;                                                    // createMt_ASCII_rcpp.cpp:79-83 Rcpp::stop
    const long n_pad = eagle_pad(n), ldn = eagle_pad(n), L_pad = eagle_pad(L);
    // marker window: its text (w x (n+1)) fits one staging buffer; multiple of 256 markers
    long w = (long)(67108864 / out_stride) / 256 * 256;
    if (!src && eagle_resident_budget() != (size_t)-1)  // streaming under a resident budget: the window image obeys it too
        w = std::min(w, (long)(eagle_resident_budget() / (size_t)n_pad) / 256 * 256);
    if (w < 256) w = 256;
    if (w > L_pad) w = L_pad;
    rc = eagle_stage_ensure(ctx, (size_t)w * out_stride);
    if (rc) return rc;
    if (!src && !quiet) {                                                                        // :125-129
        say(ctx, " A block transpose is being performed due to lack of memory.  ");
        say(ctx, " Memory parameter availmemGb is set to %g gigabytes", max_memory_in_Gbytes);
        say(ctx, " If possible, increase availmemGb parameter. ");
    }
    const bool keep = fits_resident((size_t)L_pad * ldn);
    DevBuf mt, win;
    HIPCHK(ctx, mt.alloc(keep ? (size_t)L_pad * ldn : (size_t)w * ldn));
    if (keep) HIPCHK(ctx, hipMemsetAsync(mt.p, 0, (size_t)L_pad * ldn, ctx->stream));
    if (!src) HIPCHK(ctx, win.alloc((size_t)n_pad * w));
    EventPair done;
    HIPCHK(ctx, done.create());

    SidecarWriter sc;
    (void)sc.open_for(ctx, f_name_ascii, L, n, w);
    // Window k: transpose + encode on the stream, D2H into pinned buffer k&1; the pwrite of window k-1 overlaps it.
    LinesBehind behind{ctx, fdout, f_name_ascii, out_stride, sc, done, threads};
    long k = 0;
    for (long c0 = 0; c0 < L; c0 += w, k++) {
        const int b = (int)(k & 1);
        const long wc = std::min(w, L_pad - c0), real = std::min(w, L - c0);
        const int8_t* sp;
        long sld;
        if (src) { sp = src->dev + c0; sld = src->ld; }
        else {
            rc = behind.flush();  // the tile loader below uses the same staging buffers as the pending write
            if (rc) return rc;
            HIPCHK(ctx, hipMemsetAsync(win.p, 0, (size_t)n_pad * w, ctx->stream));
            rc = eagle_dev_load_ascii(ctx, f_name, 0, n, c0, real, win.as<int8_t>(), w, max_memory_in_Gbytes, threads);
            if (rc) return rc;
            sp = win.as<int8_t>();
            sld = w;
        }
        int8_t* dst = mt.as<int8_t>() + (keep ? c0 * ldn : 0);
        rc = eagle_dev_transpose_i8(ctx, sp, n_pad, wc, sld, dst, ldn, ctx->stream);
        if (rc) return rc;
        rc = eagle_dev_encode_ascii(ctx, dst, real, n, ldn, (uint8_t*)ctx->stage_raw[b], ctx->stream);
        if (rc) return rc;
        if (behind.b == b) { rc = behind.flush(); if (rc) return rc; }
        HIPCHK(ctx, hipMemcpyAsync(ctx->stage_pin[b], ctx->stage_raw[b], (size_t)real * out_stride, hipMemcpyDeviceToHost, ctx->stream));
        rc = sc.pack(b, dst, real, ldn);
        if (rc) return rc;
        HIPCHK(ctx, hipEventRecord(done.e[b], ctx->stream));
        rc = behind.next(c0, real, b);  // window k-1 goes to disk while window k is on the device
        if (rc) return rc;
    }
    rc = behind.flush();
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    say_summary(ctx, type, f_name, n, L, max_memory_in_Gbytes);
    close(closer.fd);
    closer.fd = -1;  // the text file is final: its size and mtime key the sidecar and the cache entry
    sc.finish(f_name_ascii);
    if (keep) {
        int8_t* give = mt.as<int8_t>();
        mt.p = nullptr;
        return eagle_cache_adopt(ctx, f_name_ascii, L, n, L_pad, ldn, give);
    }
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// PLINK binary (.bed, SNP-major) -> M.ascii + Mt.ascii
// ---------------------------------------------------------------------------------------------------------------
namespace {

// an output text file: pre-sized when opened, and cut back to nothing unless the call gets as far as finish()
struct TextOut {
    int fd = -1;
    ~TextOut() {
        if (fd >= 0) { (void)ftruncate(fd, 0); close(fd); }
    }
    bool open_sized(const char* path, off_t bytes) {
        fd = open(path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
        return fd >= 0 && ftruncate(fd, bytes) == 0;
    }
    void finish() { close(fd); fd = -1; }
};

// Lines [r0, r0 + nrows) of a text file of `cols` characters per line from the rows of an int8 image (`img`: the first of them), with their
// sidecar rows: encode + pack on the stream into staging buffer k & 1, the pwrite of chunk k - 1 under the device work of chunk k.
int write_lines_from_image(eagle_ctx* ctx, int fd, const char* path, const int8_t* img, long ld, long r0, long nrows, long cols, long chunk_rows,
                           SidecarWriter& sc, EventPair& done, int threads) {
    const long stride = cols + 1;
    LinesBehind behind{ctx, fd, path, stride, sc, done, threads};
    long k = 0;
    for (long r = 0; r < nrows; r += chunk_rows, k++) {
        const int b = (int)(k & 1);  // free: chunk k - 2 went to disk while chunk k - 1 was enqueued
        const long nr = std::min(chunk_rows, nrows - r);
        int rc = eagle_dev_encode_ascii(ctx, img + r * ld, nr, cols, ld, (uint8_t*)ctx->stage_raw[b], ctx->stream);
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->stage_pin[b], ctx->stage_raw[b], (size_t)nr * stride, hipMemcpyDeviceToHost, ctx->stream));
        rc = sc.pack(b, img + r * ld, nr, ld);
        if (rc) return rc;
        HIPCHK(ctx, hipEventRecord(done.e[b], ctx->stream));
        rc = behind.next(r0 + r, nr, b);
        if (rc) return rc;
    }
    return behind.flush();
}

// The one staging ring of the .bed entry points: a SNP-major .bed file of L markers of n individuals, opened and checked (header, size),
// whose rows go to the device in windows the caller chooses (they may overlap, or leave rows out) through the context's two pinned /
// device staging buffers in turn.  Window k: stage() -- pread into pinned buffer k & 1, upload -- then the caller's kernels on
// ctx->stream, then release(), which records the buffer's event behind the last operation that reads the staged rows or writes the
// pinned buffer.  THE buffer-reuse rule lives here and nowhere else: stage() of window k (its first step, acquire()) waits for the event of window k - 2, i.e.
// until window k - 2 has left staging buffer b, so the pread of window k runs under the device work of window k - 1.  A caller that
// fails inside its window loop drains the stream before it returns: the ring's buffers belong to the context and outlive the call.
struct BedRing {
    eagle_ctx* ctx = nullptr;
    const char* path = nullptr;
    int fd = -1, threads = 1;
    long rb = 0;            // bytes of a file row
    size_t byte_off = 0;    // where the rows lie in a staging buffer (eagle_create_ascii_from_bed keeps a window's text in front of them)
    long windows = 0;       // windows staged so far
    EventPair ev;
    ~BedRing() { if (fd >= 0) close(fd); }
    int open(eagle_ctx* c, const char* bed_path, long n, long L) {
        ctx = c; path = bed_path; threads = host_threads(); rb = bed_row_bytes(n);
        HIPCHK(ctx, hipSetDevice(ctx->device));
        fd = ::open(bed_path, O_RDONLY);
        struct stat st;
        if (fd < 0 || fstat(fd, &st) != 0) return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", bed_path);
        unsigned char head[BED_HEADER_BYTES];
        const ssize_t got = pread(fd, head, sizeof head, 0);
        switch (bed_check_header(head, got < 0 ? 0 : (long)got)) {
            case BED_HEADER_OK: break;
            case BED_HEADER_INDIVIDUAL_MAJOR:
                return failf(ctx, EAGLE_ERR_FORMAT, "%s is an individual-major .bed file (third byte 0x00); only SNP-major files are read", bed_path);
            case BED_HEADER_MODE:
                return failf(ctx, EAGLE_ERR_FORMAT, "%s: third byte 0x%02x is not a .bed mode (0x01 SNP-major)", bed_path, (unsigned)head[2]);
            default:
                return failf(ctx, EAGLE_ERR_FORMAT, "%s is not a PLINK .bed file (it does not start with 0x6c 0x1b)", bed_path);
        }
        if ((long long)st.st_size != bed_expected_size(n, L))
            return failf(ctx, EAGLE_ERR_FORMAT, "%s holds %lld bytes, but %ld markers of %ld individuals take %lld", bed_path, (long long)st.st_size, L,
                         n, bed_expected_size(n, L));
        HIPCHK(ctx, ev.create());
        return EAGLE_OK;
    }
    // staging buffers for windows of up to rows_max rows that start byte_off bytes into a buffer
    int ensure(long rows_max, size_t off = 0) {
        byte_off = off;
        return eagle_stage_ensure(ctx, off + (size_t)rows_max * rb);
    }
    int last() const { return (int)((windows - 1) & 1); }   // the buffer staged last
    char* pinned(int b) const { return (char*)ctx->stage_pin[b]; }
    uint8_t* device(int b) const { return (uint8_t*)ctx->stage_raw[b]; }
    // The same ring over a file that is no .bed file (eagle_vcf_to_bed's text): no header check, no rows; the caller stages byte spans
    // with acquire() / fill() / upload() and keeps the rule by calling release() once per window.  *size_out = the file's bytes.
    int open_bytes(eagle_ctx* c, const char* file_path, long long* size_out) {
        ctx = c; path = file_path; threads = host_threads(); rb = 1;
        HIPCHK(ctx, hipSetDevice(ctx->device));
        fd = ::open(file_path, O_RDONLY);
        struct stat st;
        if (fd < 0 || fstat(fd, &st) != 0) return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", file_path);
        *size_out = (long long)st.st_size;
        HIPCHK(ctx, ev.create());
        return EAGLE_OK;
    }
    // the next window's buffer, free: window k - 2 has left it
    int acquire() {
        const int b = (int)(windows & 1);
        if (windows >= 2) HIPCHK(ctx, hipEventSynchronize(ev.e[b]));
        windows++;
        return EAGLE_OK;
    }
    // `bytes` of the file from `off` into the acquired buffer's pinned half, `at` bytes in
    bool fill(off_t off, size_t bytes, size_t at) { return pread_all(fd, pinned(last()) + at, bytes, off, threads); }
    // that span on its way to the device half (stream order)
    int upload(size_t at, size_t bytes, const uint8_t** raw) {
        const int b = last();
        HIPCHK(ctx, hipMemcpyAsync(device(b) + at, pinned(b) + at, bytes, hipMemcpyHostToDevice, ctx->stream));
        *raw = device(b) + at;
        return EAGLE_OK;
    }
    // file rows [f0, f0 + rows) on their way to *raw (stream order)
    int stage(long f0, long rows, const uint8_t** raw) {
        if (int rc = acquire()) return rc;
        if (!fill((off_t)BED_HEADER_BYTES + (off_t)f0 * rb, (size_t)rows * rb, byte_off)) {
            (void)hipStreamSynchronize(ctx->stream);
            return failf(ctx, EAGLE_ERR_FORMAT, "%s: could not read markers %ld to %ld", path, f0 + 1, f0 + rows);
        }
        return upload(byte_off, (size_t)rows * rb, raw);
    }
    int release() {
        HIPCHK(ctx, hipEventRecord(ev.e[last()], ctx->stream));
        return EAGLE_OK;
    }
    // The plain pass: the file's L rows in disjoint windows of w, each staged and handed to body(r0, nr, raw), which launches on
    // ctx->stream and calls release() once the staged rows have been read.  A failure drains the stream (the rule of the header comment).
    template <class Body>
    int each(long L, long w, Body body) {
        RowWindows ws = row_windows_disjoint(L, w);
        RowWindow win;
        while (ws.next(win)) {
            const uint8_t* raw;
            int rc = stage(win.lo, win.nr, &raw);
            if (!rc) rc = body(win.lo, win.nr, raw);
            if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        }
        return EAGLE_OK;
    }
    // write-behind: until everything enqueued before release() of buffer b's last window is done
    int wait(int b) {
        HIPCHK(ctx, hipEventSynchronize(ev.e[b]));
        return EAGLE_OK;
    }
};

// Write-behind of the two imputers' output .bed file, pre-sized with its header and cut back to nothing unless the call gets as far as
// finish().  push(): window k's patched rows are copied back into the pinned buffer they were read into (stream order: behind its
// upload), the ring's buffer is released, and the pwrite of window k - 1 runs under the device work of window k.
struct BedRewrite {
    TextOut out;
    eagle_ctx* ctx = nullptr;
    const char* path = nullptr;
    long held_r0 = -1, held_n = 0, rb = 0;   // the window not yet on disk (held_r0 < 0: none)
    int held_b = 0;
    int open(eagle_ctx* c, const char* out_bed_path, long n, long L) {
        static const char head[BED_HEADER_BYTES] = {0x6c, 0x1b, 0x01};
        ctx = c; path = out_bed_path; rb = bed_row_bytes(n);
        if (!out.open_sized(path, (off_t)bed_expected_size(n, L)) || !pwrite_all(out.fd, head, sizeof head, 0, 1))
            return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", path);
        return EAGLE_OK;
    }
    int flush(BedRing& ring) {
        if (held_r0 < 0) return EAGLE_OK;
        if (int rc = ring.wait(held_b)) return rc;
        if (!pwrite_all(out.fd, ring.pinned(held_b), (size_t)held_n * rb, (off_t)BED_HEADER_BYTES + (off_t)held_r0 * rb, ring.threads))
            return failf(ctx, EAGLE_ERR_OPEN, "ERROR: could not write %s", path);
        held_r0 = -1;
        return EAGLE_OK;
    }
    // `patched` (device): the rows [r0, r0 + nr) of the output, made from the window staged last
    int push(BedRing& ring, const void* patched, long r0, long nr) {
        const int b = ring.last();
        HIPCHK(ctx, hipMemcpyAsync(ring.pinned(b), patched, (size_t)nr * rb, hipMemcpyDeviceToHost, ctx->stream));
        int rc = ring.release();
        if (!rc) rc = flush(ring);
        held_r0 = r0; held_n = nr; held_b = b;
        return rc;
    }
    int finish(BedRing& ring) {
        if (int rc = flush(ring)) return rc;
        out.finish();
        return EAGLE_OK;
    }
};

}  // namespace

// Mt.ascii is the bed file's own order: every marker window is decoded by k_bed_decode into its int8 tile and its sidecar rows, encoded
// to text and written while the next window is on the device.  M.ascii is the other order, so every window's tile is also transposed
// into an image of M: the whole of it when it fits (kept as the resident copy), else a band of individuals per PASS over the bed file --
// the first pass writes Mt.ascii as well, the later ones only decode (or, with Mt resident, transpose from its image) -- and M.ascii
// and its sidecar are written from the finished image or band in row chunks, in file order, by the same code either way.
extern "C" int eagle_create_ascii_from_bed(eagle_ctx* ctx, const char* bed_path, const char* f_name_ascii_M, const char* f_name_ascii_Mt,
                                           double max_memory_in_Gbytes, const long dims[2], int quiet, long* n_missing_out) {
    if (!ctx || !bed_path || !f_name_ascii_M || !f_name_ascii_Mt || !dims) return EAGLE_ERR_ARG;
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "create_ascii_from_bed: dims must be positive");
    BedRing ring;
    if (int orc = ring.open(ctx, bed_path, n, L)) return orc;

    const int threads = ring.threads;
    const long rb = ring.rb, n_pad = eagle_pad(n), ldn = n_pad, L_pad = eagle_pad(L);
    const size_t budget = eagle_resident_budget();
    const long w = bed_window_markers(n, n_pad, L_pad, (size_t)67108864, budget), nwin = bed_window_count(w, L);
    const long mt_stride = n + 1, bed_off = ((w * mt_stride + 255) / 256) * 256;   // staging buffer: the window's text, then its bed bytes
    const long m_chunk = std::max(1L, std::min(n, (long)(67108864 / (L + 1))));
    int rc = eagle_stage_ensure(ctx, std::max((size_t)bed_off + (size_t)w * rb, (size_t)m_chunk * (L + 1)));   // one growth for both files' needs
    if (!rc) rc = ring.ensure(w, (size_t)bed_off);
    if (rc) return rc;
    if (!quiet) { say(ctx, ""); say(ctx, " Reading PLINK binary File  "); say(ctx, ""); say(ctx, " Loading file "); }

    const bool keepMt = fits_resident((size_t)L_pad * ldn);
    DevBuf mt, mimg;
    HIPCHK(ctx, mt.alloc(keepMt ? (size_t)L_pad * ldn : (size_t)w * ldn));
    const bool keepM = fits_resident((size_t)n_pad * L_pad);
    const long band = keepM ? n_pad : stream_chunk_rows_core(budget, L_pad, n_pad);   // individuals per pass over the bed file
    HIPCHK(ctx, mimg.alloc((size_t)band * L_pad));
    unsigned long long* d_missing = (unsigned long long*)scr_take(ctx, EAGLE_SCR_INGEST);
    HIPCHK(ctx, hipMemsetAsync(d_missing, 0, sizeof(unsigned long long), ctx->stream));

    TextOut outM, outMt;
    if (!outMt.open_sized(f_name_ascii_Mt, (off_t)L * mt_stride)) return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", f_name_ascii_Mt);
    if (!outM.open_sized(f_name_ascii_M, (off_t)n * (L + 1))) return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", f_name_ascii_M);
    SidecarWriter scM, scMt;
    (void)scMt.open_for(ctx, f_name_ascii_Mt, L, n, w);
    (void)scM.open_for(ctx, f_name_ascii_M, n, L, m_chunk);
    unsigned long long n_missing = 0;

    for (long r0 = 0; r0 < n; r0 += band) {
        const bool first = r0 == 0;                       // the pass that writes Mt.ascii
        const bool decode = first || !keepMt;             // later passes find the tiles in Mt's resident image
        const long bcols = std::min(band, n_pad - r0);    // individuals (padded) of this pass's image of M
        LinesBehind behind{ctx, outMt.fd, f_name_ascii_Mt, mt_stride, scMt, ring.ev, threads};
        for (long k = 0; k < nwin; k++) {
            const BedWindow bw = bed_window(k, w, L, L_pad);
            int8_t* tile = mt.as<int8_t>() + (keepMt ? bw.c0 * ldn : 0);
            rc = EAGLE_OK;
            if (decode) {
                const uint8_t* raw;
                rc = ring.stage(bw.c0, bw.real, &raw);
                if (!rc) rc = eagle_dev_bed_decode(ctx, raw, bw.real, bw.padded, n, tile, ldn, first ? scMt.packed(ring.last()) : nullptr,
                                                   scMt.row_bytes, first ? d_missing : nullptr, ctx->stream);
            }
            if (!rc) rc = eagle_dev_transpose_i8(ctx, tile + r0, bw.padded, bcols, ldn, mimg.as<int8_t>() + bw.c0, L_pad, ctx->stream);
            if (!rc && first) {   // the window's text: encoded in front of its bed bytes, in the buffer they were staged in
                const int b = ring.last();
                rc = eagle_dev_encode_ascii(ctx, tile, bw.real, n, ldn, ring.device(b), ctx->stream);
                if (!rc) {
                    const hipError_t e = hipMemcpyAsync(ring.pinned(b), ring.device(b), (size_t)bw.real * mt_stride, hipMemcpyDeviceToHost, ctx->stream);
                    if (e != hipSuccess) rc = eagle_fail_hip(ctx, e, "hipMemcpyAsync");
                }
                if (!rc) rc = scMt.fetch(b, bw.real);
            }
            if (!rc && decode) rc = ring.release();
            if (!rc && first) rc = behind.next(bw.c0, bw.real, ring.last());  // window k - 1 goes to disk while window k is on the device
            if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        }
        if (first) {
            rc = behind.flush();
            if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            HIPCHK(ctx, hipMemcpy(&n_missing, d_missing, sizeof n_missing, hipMemcpyDeviceToHost));
            if (n_missing) say_missing_alleles(ctx);
            outMt.finish();  // Mt.ascii is final: its size and mtime key the sidecar and the cache entry
            scMt.finish(f_name_ascii_Mt);
        }
        rc = write_lines_from_image(ctx, outM.fd, f_name_ascii_M, mimg.as<int8_t>(), L_pad, r0, std::min(band, n - r0), L, m_chunk, scM, ring.ev, threads);
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (n_missing_out) *n_missing_out = (long)n_missing;
    say_summary(ctx, "PLINKbed", f_name_ascii_M, n, L, max_memory_in_Gbytes);
    outM.finish();
    scM.finish(f_name_ascii_M);
    if (keepM) {
        int8_t* give = mimg.as<int8_t>();
        mimg.p = nullptr;
        rc = eagle_cache_adopt(ctx, f_name_ascii_M, n, L, n_pad, L_pad, give);
        if (rc) return rc;
    }
    if (keepMt) {
        int8_t* give = mt.as<int8_t>();
        mt.p = nullptr;
        return eagle_cache_adopt(ctx, f_name_ascii_Mt, L, n, L_pad, ldn, give);
    }
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Marker QC: per-marker genotype counts and filtered panels (no counterpart in the reference; kernels in eagle_qc.hip)
// ---------------------------------------------------------------------------------------------------------------
namespace {

// argument errors are decided before the context is touched: without one the text goes where eagle_open_error() finds it
int qc_fail(eagle_ctx* ctx, int code, const char* msg) {
    if (ctx) return eagle_fail(ctx, code, msg);
    snprintf(g_open_err, sizeof g_open_err, "%s", msg);
    return code;
}

}  // namespace

// counts_out[3 i .. 3 i + 2] = the numbers of '0', '1', '2' characters of line i of a genotype file of L lines of n characters.
// The image is counted where it lies when it is (or can be made) resident; else in row windows of the size the streamed
// scans use, each loaded through eagle_dev_load_ascii (sidecar, text, or a VIEW's source) and counted before the next one is read.
static int line_counts(eagle_ctx* ctx, const char* f_name_ascii_Mt, long n, long L, double max_memory_in_Gbytes, int32_t* counts_out) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf counts;
    HIPCHK(ctx, counts.alloc(sizeof(int32_t) * 3 * (size_t)L));
    ImageLines lines;
    int rc = lines.open(ctx, f_name_ascii_Mt, L, n, max_memory_in_Gbytes);
    if (rc) return rc;
    rc = lines.each(lines.disjoint(lines.stream_rows()), [&](const int8_t* img, long r0, long nr, long, long) {
        return eagle_dev_marker_counts(ctx, img, nr, n, lines.ld(), counts.as<int32_t>() + 3 * r0, ctx->stream);
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(counts_out, counts.p, sizeof(int32_t) * 3 * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

extern "C" int eagle_marker_counts(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], double max_memory_in_Gbytes,
                                   int32_t* counts_out) {
    if (!f_name_ascii_Mt || !dims || !counts_out) return qc_fail(ctx, EAGLE_ERR_ARG, "marker_counts: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "marker_counts: dims must be positive");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "marker_counts: no context");
    return line_counts(ctx, f_name_ascii_Mt, n, L, max_memory_in_Gbytes, counts_out);
}

// The rows go through the staging ring (BedRing) in windows of bed_stage_rows: up to 64 MiB.
extern "C" int eagle_bed_marker_counts(eagle_ctx* ctx, const char* bed_path, const long dims[2], double max_memory_in_Gbytes,
                                       int32_t* counts_out) {
    if (!bed_path || !dims || !counts_out) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_marker_counts: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_marker_counts: dims must be positive");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_marker_counts: no context");
    BedRing ring;
    if (int orc = ring.open(ctx, bed_path, n, L)) return orc;
    const long w = std::min(L, bed_stage_rows(ring.rb, max_memory_in_Gbytes));
    int rc = ring.ensure(w);
    if (rc) return rc;
    DevBuf counts;
    HIPCHK(ctx, counts.alloc(sizeof(int32_t) * 4 * (size_t)L));
    rc = ring.each(L, w, [&](long r0, long nr, const uint8_t* raw) {
        const int brc = eagle_dev_bed_marker_counts(ctx, raw, nr, n, counts.as<int32_t>() + 4 * r0, ctx->stream);
        return brc ? brc : ring.release();
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(counts_out, counts.p, sizeof(int32_t) * 4 * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// VCF -> PLINK binary fileset (include/eagle_hip.h section 1b-vcf; kernels in eagle_vcf.hip)
// ---------------------------------------------------------------------------------------------------------------
namespace {

static_assert(VCF_A2_ALT == EAGLE_VCF_A2_ALT && VCF_SNPS_ONLY == EAGLE_VCF_SNPS_ONLY && VCF_PASS_ONLY == EAGLE_VCF_PASS_ONLY, "flag values");
#define VCF_MAX_WINDOW 1073741824L   /* 2^30: the longest line, and the largest window */

// the output fileset: what this call created is removed again unless the call gets as far as keep()
struct VcfFileset {
    std::string bed, bim, fam;
    FILE* fbim = nullptr;
    bool made_bed = false, made_fam = false, kept = false;
    ~VcfFileset() {
        if (fbim) fclose(fbim);
        if (kept) return;
        if (made_bed) unlink(bed.c_str());
        if (fbim) unlink(bim.c_str());
        if (made_fam) unlink(fam.c_str());
    }
    bool keep() {
        const bool ok = fbim && fclose(fbim) == 0;
        fbim = nullptr;
        if (!ok) unlink(bim.c_str());
        kept = ok;
        return ok;
    }
};

// the kept lines of one window, until their counters are back: file line numbers, and which staging buffer's pinned table holds them
struct VcfPending {
    bool live = false;
    long window = 0;
    std::vector<long> line_no;
};

// Where the line that starts at `from` ends: the offset behind its '\n', or the file size.  -1: a read failed.
long long vcf_line_end(int fd, long long from, long long fsize) {
    char buf[65536];
    for (long long at = from; at < fsize;) {
        const ssize_t got = pread(fd, buf, (size_t)std::min<long long>((long long)sizeof buf, fsize - at), (off_t)at);
        if (got <= 0) return -1;
        const char* q = (const char*)memchr(buf, '\n', (size_t)got);
        if (q) return at + (q - buf) + 1;
        at += got;
    }
    return fsize;
}

}  // namespace

// Window k: acquire a staging buffer (the ring's rule), pread whole lines into its pinned half and send them up; the host then splits
// the lines, parses the fixed fields, appends the .bim lines and fills the kept lines' table while the device still works on window
// k - 1; table up, k_vcf_fields, k_vcf_pack, counters and rows back into pinned memory, and BedRewrite writes window k - 1's rows.
// The counters of a window are checked when its buffer comes round again (or at the end): a kept line whose field count is not n fails
// the call.  Errors are reported in file order: before a host-side error is returned, the lines in front of it are checked.
extern "C" int eagle_vcf_to_bed(eagle_ctx* ctx, const char* vcf_path, const char* out_prefix, int flags, double max_memory_in_Gbytes,
                                long chunk_bytes, long dims_out[2], eagle_vcf_counts* counts_out) {
    if (!vcf_path || !out_prefix || !dims_out || !counts_out) return qc_fail(ctx, EAGLE_ERR_ARG, "vcf_to_bed: NULL argument");
    if (flags & ~VCF_FLAGS_ALL) return qc_fail(ctx, EAGLE_ERR_ARG, "vcf_to_bed: unknown flag bits (section 1b-vcf: A2_ALT 1, SNPS_ONLY 2, PASS_ONLY 4)");
    if (chunk_bytes < 0) return qc_fail(ctx, EAGLE_ERR_ARG, "vcf_to_bed: chunk_bytes must not be negative");
    if (chunk_bytes > VCF_MAX_WINDOW) return qc_fail(ctx, EAGLE_ERR_ARG, "vcf_to_bed: chunk_bytes above 2^30");
    if (!out_prefix[0]) return qc_fail(ctx, EAGLE_ERR_ARG, "vcf_to_bed: empty output prefix");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "vcf_to_bed: no context");

    BedRing ring;
    long long fsize = 0;
    if (int orc = ring.open_bytes(ctx, vcf_path, &fsize)) return orc;
    const double mem = max_memory_in_Gbytes;
    long cap = std::min(vcf_window_bytes(chunk_bytes, mem), VCF_MAX_WINDOW);
    if (chunk_bytes == 0) cap = std::min<long long>(cap, std::max<long long>(4096, fsize));   // a small file needs no 64 MiB
    auto text_room = [](long bytes) { return (size_t)((bytes + 16 + 255) / 256 * 256); };     // the rounded-up last 16-byte load stays inside
    int rc = eagle_stage_ensure(ctx, text_room(cap));
    if (rc) return rc;

    VcfFileset files;
    files.bed = std::string(out_prefix) + ".bed";
    files.bim = std::string(out_prefix) + ".bim";
    files.fam = std::string(out_prefix) + ".fam";
    BedRewrite out;
    eagle_vcf_counts cn;
    memset(&cn, 0, sizeof cn);
    bool have_header = false;
    long n = 0, rb = 0, line_no = 0, window = 0, lines_cap = 0;
    const int a2_alt = (flags & VCF_A2_ALT) ? 1 : 0;
    PinBuf pin_tab[2];                      // per staging buffer: the table (16 bytes a line), then the counters (16 bytes a line)
    DevBuf d_tab, d_codes, d_cnt, d_bed;    // one of each: window k follows window k - 1 in stream order
    VcfPending pend[2];
    std::string bimbuf;
    char msg[400];

    // (re)size what depends on the kept lines a window can hold; the stream is idle and nothing is pending when this is called
    auto size_lines = [&](long text_bytes) -> int {
        const long want = vcf_window_lines(text_bytes, n);
        if (want <= lines_cap) return EAGLE_OK;
        for (int b = 0; b < 2; b++) {
            if (pin_tab[b].p) { (void)hipHostFree(pin_tab[b].p); pin_tab[b].p = nullptr; }
            HIPCHK(ctx, pin_tab[b].alloc(32 * (size_t)want));
        }
        for (DevBuf* d : {&d_tab, &d_codes, &d_cnt, &d_bed})
            if (d->p) { (void)hipFree(d->p); d->p = nullptr; }
        HIPCHK(ctx, d_tab.alloc(16 * (size_t)want));
        HIPCHK(ctx, d_cnt.alloc(16 * (size_t)want));
        HIPCHK(ctx, d_codes.alloc((size_t)want * (size_t)n));
        HIPCHK(ctx, d_bed.alloc((size_t)want * (size_t)rb));
        lines_cap = want;
        return EAGLE_OK;
    };
    // the counters of the window that used buffer b: every kept line has n fields, or the call fails with the first that has not
    auto check = [&](int b) -> int {
        VcfPending& p = pend[b];
        if (!p.live) return EAGLE_OK;
        p.live = false;
        const int32_t* c = (const int32_t*)((const char*)pin_tab[b].p + 16 * (size_t)lines_cap);
        for (size_t i = 0; i < p.line_no.size(); i++, c += 4) {
            if (c[0] != n)
                return failf(ctx, EAGLE_ERR_FORMAT, "%s line %ld: %d sample fields, the header names %ld (section 1b-vcf)", vcf_path, p.line_no[i],
                             (int)c[0], n);
            cn.missing += c[1];
            cn.haploid += c[2];
            cn.malformed += c[3];
        }
        return EAGLE_OK;
    };
    // everything enqueued is done, both windows' counters are checked (the older first) and the rows held back are on disk
    auto settle = [&]() -> int {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        const int first = (pend[0].live && pend[1].live && pend[1].window < pend[0].window) ? 1 : 0;
        int src = check(first);
        if (!src) src = check(1 - first);
        if (!src && have_header) src = out.flush(ring);
        return src;
    };
    // a host-side error: what lies in front of it in the file is judged first
    auto fail_at = [&](int code, const char* text, const std::vector<long>& here_no, const int64_t* here_tab, const char* txt) -> int {
        int src = settle();
        if (src) { (void)hipStreamSynchronize(ctx->stream); return src; }
        for (size_t i = 0; i < here_no.size(); i++) {
            const long found = vcf_count_fields(txt + here_tab[2 * i], txt + here_tab[2 * i + 1]);
            if (found != n)
                return failf(ctx, EAGLE_ERR_FORMAT, "%s line %ld: %ld sample fields, the header names %ld (section 1b-vcf)", vcf_path, here_no[i],
                             found, n);
        }
        return failf(ctx, code, "%s", text);
    };

    std::vector<long> here_no;
    std::vector<std::string> names;
    for (long long pos = 0; pos < fsize;) {
        long want = (long)std::min<long long>(cap, fsize - pos);
        rc = ring.acquire();
        if (!rc) rc = check((int)ring.last());   // the window that used this buffer is through
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        const int b = ring.last();
        here_no.clear();
        bool ok = ring.fill((off_t)pos, (size_t)want, 0);
        size_t wbytes = 0;
        if (ok) wbytes = pos + want == fsize ? (size_t)want : vcf_whole_lines(ring.pinned(b), (size_t)want);
        if (ok && wbytes == 0) {   // the line is longer than the window: the window grows to it
            const long long le = vcf_line_end(ring.fd, pos + want, fsize);
            ok = le >= 0;
            if (ok && (le - pos > VCF_MAX_WINDOW || !vcf_line_fits((long)(le - pos), mem))) {
                snprintf(msg, sizeof msg, "vcf_to_bed: line %ld of %s holds %lld bytes and does not fit max_memory_in_Gbytes (section 1b-vcf, rule 6)",
                         line_no + 1, vcf_path, le - pos);
                return fail_at(EAGLE_ERR_ARG, msg, here_no, nullptr, nullptr);
            }
            if (ok) {
                want = (long)(le - pos);
                rc = settle();
                if (!rc) rc = eagle_stage_ensure(ctx, text_room(want));
                if (!rc && have_header) rc = size_lines(want);
                if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
                ok = ring.fill((off_t)pos, (size_t)want, 0);
                wbytes = (size_t)want;
            }
        }
        if (!ok) {
            snprintf(msg, sizeof msg, "%s: could not read the bytes from %lld", vcf_path, pos);
            return fail_at(EAGLE_ERR_FORMAT, msg, here_no, nullptr, nullptr);
        }
        const char* txt = ring.pinned(b);
        const uint8_t* d_text;
        rc = ring.upload(0, wbytes, &d_text);   // on its way while the host reads the same bytes
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }

        int64_t* tab = (int64_t*)pin_tab[b].p;   // NULL until the header is read: no line is kept before
        bimbuf.clear();
        size_t p = 0, lb, le, next;
        for (; vcf_next_line(txt, wbytes, p, true, &lb, &le, &next); p = next) {
            line_no++;
            if (le == lb) continue;
            if (le - lb >= 2 && txt[lb] == '#' && txt[lb + 1] == '#') continue;
            if (!have_header) {
                std::vector<VcfSpan> spans;
                if (const char* what = vcf_header_error(txt + lb, txt + le, spans)) {
                    snprintf(msg, sizeof msg, "%s line %ld: %s (section 1b-vcf)", vcf_path, line_no, what);
                    return fail_at(EAGLE_ERR_FORMAT, msg, here_no, tab, txt);
                }
                n = (long)spans.size();
                rb = bed_row_bytes(n);
                for (const VcfSpan& s : spans) names.emplace_back(s.p, (size_t)s.len);
                FILE* ffam = fopen(files.fam.c_str(), "w");
                if (ffam) files.made_fam = true;
                bool wrote = ffam != nullptr;
                for (size_t i = 0; wrote && i < names.size(); i++) wrote = fprintf(ffam, "%s %s 0 0 0 -9\n", names[i].c_str(), names[i].c_str()) > 0;
                if (ffam && fclose(ffam) != 0) wrote = false;
                if (!wrote) { (void)hipStreamSynchronize(ctx->stream); return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", files.fam.c_str()); }
                files.fbim = fopen(files.bim.c_str(), "w");
                if (!files.fbim) { (void)hipStreamSynchronize(ctx->stream); return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", files.bim.c_str()); }
                rc = out.open(ctx, files.bed.c_str(), n, 0);
                files.made_bed = out.out.fd >= 0;
                if (!rc) {   // nothing but this window's upload is in flight, and it does not touch what size_lines makes
                    rc = size_lines((long)std::max<size_t>(wbytes, (size_t)cap));
                    tab = (int64_t*)pin_tab[b].p;
                }
                if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
                have_header = true;
                continue;
            }
            cn.lines++;
            VcfSpan f[9];
            const char* rest;
            if (vcf_split_tabs(txt + lb, txt + le, f, 9, &rest) < 9) {
                snprintf(msg, sizeof msg, "%s line %ld: a data line with fewer than nine fixed fields (section 1b-vcf)", vcf_path, line_no);
                return fail_at(EAGLE_ERR_FORMAT, msg, here_no, tab, txt);
            }
            switch (vcf_verdict(f, flags)) {
                case VCF_MULTIALLELIC: cn.multiallelic++; continue;
                case VCF_NO_ALT: cn.no_alt++; continue;
                case VCF_NO_GT: cn.no_gt++; continue;
                case VCF_NOT_SNP: cn.not_snp++; continue;
                case VCF_FILTERED: cn.filtered++; continue;
                default: break;
            }
            // a line too short for n fields is judged here, so that the kept lines of a window always fit lines_cap
            const long found = !rest ? 0 : ((txt + le) - rest < 2 * n - 1 ? vcf_count_fields(rest, txt + le) : n);
            if (found != n || (long)here_no.size() >= lines_cap) {
                snprintf(msg, sizeof msg, "%s line %ld: %ld sample fields, the header names %ld (section 1b-vcf)", vcf_path, line_no, found, n);
                return fail_at(EAGLE_ERR_FORMAT, msg, here_no, tab, txt);
            }
            tab[2 * here_no.size()] = (int64_t)(rest - txt);
            tab[2 * here_no.size() + 1] = (int64_t)le;
            here_no.push_back(line_no);
            const VcfSpan &a1 = a2_alt ? f[3] : f[4], &a2 = a2_alt ? f[4] : f[3];
            bimbuf.append(f[0].p, (size_t)f[0].len).push_back('\t');
            if (vcf_span_is(f[2], ".")) {
                bimbuf.append(f[0].p, (size_t)f[0].len).push_back(':');
                bimbuf.append(f[1].p, (size_t)f[1].len);
            } else {
                bimbuf.append(f[2].p, (size_t)f[2].len);
            }
            bimbuf.append("\t0\t").append(f[1].p, (size_t)f[1].len).push_back('\t');
            bimbuf.append(a1.p, (size_t)a1.len).push_back('\t');
            bimbuf.append(a2.p, (size_t)a2.len).push_back('\n');
        }
        pos += (long long)wbytes;
        const long kept_here = (long)here_no.size();
        if (!bimbuf.empty() && fwrite(bimbuf.data(), 1, bimbuf.size(), files.fbim) != bimbuf.size()) {
            (void)hipStreamSynchronize(ctx->stream);
            return failf(ctx, EAGLE_ERR_OPEN, "ERROR: could not write %s", files.bim.c_str());
        }
        if (kept_here > 0) {
            int32_t* h_cnt = (int32_t*)((char*)pin_tab[b].p + 16 * (size_t)lines_cap);
            const hipError_t e1 = hipMemcpyAsync(d_tab.p, tab, 16 * (size_t)kept_here, hipMemcpyHostToDevice, ctx->stream);
            if (e1 != hipSuccess) rc = eagle_fail_hip(ctx, e1, "hipMemcpyAsync");
            if (!rc) rc = eagle_dev_vcf_fields(ctx, d_text, d_tab.as<int64_t>(), kept_here, n, a2_alt, d_codes.as<uint8_t>(), d_cnt.as<int32_t>(), ctx->stream);
            if (!rc) rc = eagle_dev_vcf_pack(ctx, d_codes.as<uint8_t>(), kept_here, n, d_bed.as<uint8_t>(), ctx->stream);
            if (!rc) {
                const hipError_t e2 = hipMemcpyAsync(h_cnt, d_cnt.p, 16 * (size_t)kept_here, hipMemcpyDeviceToHost, ctx->stream);
                if (e2 != hipSuccess) rc = eagle_fail_hip(ctx, e2, "hipMemcpyAsync");
            }
            if (!rc) rc = out.push(ring, d_bed.p, cn.kept, kept_here);   // releases the buffer; window k - 1's rows go to disk meanwhile
            pend[b].live = true;
            pend[b].window = window;
            pend[b].line_no = here_no;
            cn.kept += kept_here;
        } else {   // nothing for the device: the buffer is released behind its upload, and rows held in the other one go to disk
            rc = ring.release();
            if (!rc && have_header) rc = out.flush(ring);
        }
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        window++;
    }
    here_no.clear();
    if (!have_header) {
        snprintf(msg, sizeof msg, "%s line %ld: no #CHROM line (section 1b-vcf)", vcf_path, line_no + 1);
        return fail_at(EAGLE_ERR_FORMAT, msg, here_no, nullptr, nullptr);
    }
    rc = settle();
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    if (cn.kept == 0) return failf(ctx, EAGLE_ERR_FORMAT, "%s: no data line is kept, so there is no fileset to write (section 1b-vcf)", vcf_path);
    rc = out.finish(ring);
    if (rc) return rc;
    if (!files.keep()) return failf(ctx, EAGLE_ERR_OPEN, "ERROR: could not write %s", files.bim.c_str());
    dims_out[0] = n;
    dims_out[1] = cn.kept;
    *counts_out = cn;
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Per-group genotype counts and Fisher's exact test (include/eagle_hip.h section 1b''''iii; kernels in eagle_groups.hip)
// ---------------------------------------------------------------------------------------------------------------
namespace {

// The argument errors the two counting entry points share, decided without a context; sizes[k] = the individuals of group k.
int group_args(eagle_ctx* ctx, const char* who, const void* path, const long* dims, const int32_t* labels, int K, const void* out,
               int32_t sizes[EAGLE_GROUPS_MAX]) {
    char msg[160];
    auto fail = [&](const char* what) {
        snprintf(msg, sizeof msg, "%s: %s", who, what);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    };
    if (!path || !dims || !labels || !out) return fail("NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return fail("dims must be positive");
    if (n > 0x3fffffffL) return fail("more than 2^30 - 1 individuals");
    if (K < 1 || K > EAGLE_GROUPS_MAX) return fail("K outside [1, 64]");
    for (int k = 0; k < EAGLE_GROUPS_MAX; k++) sizes[k] = 0;
    for (long i = 0; i < n; i++) {
        if (labels[i] < -1 || labels[i] >= K) return fail("a label outside [-1, K)");
        if (labels[i] >= 0) sizes[labels[i]]++;
    }
    if (!ctx) return fail("no context");
    return EAGLE_OK;
}

// labels (n int32) and sizes (EAGLE_GROUPS_MAX int32 behind them) on the device
int group_upload(eagle_ctx* ctx, const int32_t* labels, long n, const int32_t* sizes, DevBuf& d_lab) {
    HIPCHK(ctx, d_lab.alloc(sizeof(int32_t) * ((size_t)n + EAGLE_GROUPS_MAX)));
    HIPCHK(ctx, hipMemcpyAsync(d_lab.p, labels, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_lab.as<int32_t>() + n, sizes, sizeof(int32_t) * EAGLE_GROUPS_MAX, hipMemcpyHostToDevice, ctx->stream));
    return EAGLE_OK;
}

}  // namespace

// line_counts' routes: the image is counted where it lies when it is (or can be made) resident, else in the row windows of the
// streamed scans.  The label operand is built once per call; rows are independent, so every route gives the same integers.
extern "C" int eagle_group_counts(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const int32_t* labels, int K,
                                  double max_memory_in_Gbytes, int32_t* counts_out) {
    int32_t sizes[EAGLE_GROUPS_MAX];
    if (int arc = group_args(ctx, "group_counts", f_name_ascii_Mt, dims, labels, K, counts_out, sizes)) return arc;
    const long n = dims[0], L = dims[1];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long ldh = (n + 15) / 16 * 16;
    const size_t per_row = sizeof(int32_t) * 3 * (size_t)K;
    DevBuf d_lab, onehot, counts;
    HIPCHK(ctx, onehot.alloc((size_t)EAGLE_GROUPS_MAX * ldh));
    HIPCHK(ctx, counts.alloc(per_row * (size_t)L));
    int rc = group_upload(ctx, labels, n, sizes, d_lab);
    if (rc) return rc;
    const int32_t* d_sizes = d_lab.as<int32_t>() + n;
    rc = eagle_dev_group_onehot(ctx, d_lab.as<int32_t>(), n, onehot.as<int8_t>(), ldh, ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    ImageLines lines;
    rc = lines.open(ctx, f_name_ascii_Mt, L, n, max_memory_in_Gbytes);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }   // the one-hot kernel reads this frame's buffers
    rc = lines.each(lines.disjoint(lines.stream_rows()), [&](const int8_t* img, long r0, long nr, long, long) {
        return eagle_dev_group_counts(ctx, img, nr, n, lines.ld(), onehot.as<int8_t>(), ldh, K, d_sizes,
                                      counts.as<int32_t>() + 3 * (size_t)K * (size_t)r0, ctx->stream);
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(counts_out, counts.p, per_row * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// max(T) permutation testing (include/eagle_hip.h section 1b''''vi; kernels in eagle_maxt.hip).  eagle_group_counts' routes.  The
// operand of all R arrangements is built once per call (the seeded keys are sorted in blocks of at most MAXT_SORT_BYTES); per window of
// marker rows: S and V from the `used` group's counts, the observed pass, the permuted pass.  The finish merges the tiles' partials.
// ---------------------------------------------------------------------------------------------------------------
static_assert(MAXT_MAX_N == EAGLE_MAXT_MAX_N && MAXT_TMAX == EAGLE_MAXT_TMAX && MAXT_RMAX == EAGLE_MAXT_RMAX, "eagle_host.h and eagle_hip.h disagree");
#define MAXT_SORT_BYTES (128L << 20)
extern "C" int eagle_maxt(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const int32_t* t, const uint8_t* used,
                          const int32_t* strata, uint64_t seed, long first, long R, const int32_t* perm, double max_memory_in_Gbytes,
                          int64_t* d_obs, int64_t* V, double* key_obs, int32_t* count1, double* maxkey, int32_t* argmax) {
    auto fail = [&](const char* what) {
        char msg[160];
        snprintf(msg, sizeof msg, "maxt: %s", what);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    };
    if (!f_name_ascii_Mt || !dims || !t || !d_obs || !V || !key_obs || !count1 || !maxkey || !argmax) return fail("NULL argument");
    const long n = dims[0], L = dims[1];
    long N = 0;
    int64_t tmax = 0;
    if (const char* bad = maxt_arg_error(n, L, t, used, strata, first, R, perm, &N, &tmax)) return fail(bad);
    if (!maxt_bound_ok(N, tmax)) return fail("|d| would reach 2^53");
    if (!ctx) return fail("no context");

    // u_0 < ... < u_{N-1}; tu[k] = t[u_k]; rank_obs[i] = k of u_k = i; rank_fill[u_sigma[k]] = k (sigma: by stratum, then by position)
    const int P = maxt_planes(tmax);
    std::vector<int32_t> tu((size_t)N), rank_obs((size_t)n, -1), rank_fill, labels((size_t)n), u((size_t)N);
    std::vector<uint16_t> su((size_t)N, 0);
    int64_t T = 0;
    for (long i = 0, k = 0; i < n; i++) {
        const bool in = !used || used[i];
        labels[(size_t)i] = in ? 0 : -1;
        if (!in) continue;
        u[(size_t)k] = (int32_t)i;
        tu[(size_t)k] = t[i];
        T += t[i];
        rank_obs[(size_t)i] = (int32_t)k;
        if (strata && !perm) su[(size_t)k] = (uint16_t)strata[i];
        k++;
    }
    const bool stratified = strata && !perm;
    if (stratified) {
        std::vector<int32_t> sigma((size_t)N);
        for (long k = 0; k < N; k++) sigma[(size_t)k] = (int32_t)k;
        std::stable_sort(sigma.begin(), sigma.end(), [&](int32_t a, int32_t b) { return su[(size_t)a] < su[(size_t)b]; });
        rank_fill.assign((size_t)n, -1);
        for (long k = 0; k < N; k++) rank_fill[(size_t)u[(size_t)sigma[(size_t)k]]] = (int32_t)k;
    }
    int32_t sizes[EAGLE_GROUPS_MAX] = {0};
    sizes[0] = (int32_t)N;
    long NP2 = 2;
    while (NP2 < N) NP2 <<= 1;

    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long ldh = (n + 15) / 16 * 16;
    const long sort_rows = perm ? 0 : std::max(1L, std::min(R, MAXT_SORT_BYTES / (NP2 * 8)));
    DevBuf d_lab, onehot, counts, d_tu, d_rank_obs, d_rank_fill, d_su, d_perm, keys, op, op_obs, dS, dV, dD, dK, dC, pkey, parg, dmax, darg;
    HIPCHK(ctx, onehot.alloc((size_t)EAGLE_GROUPS_MAX * ldh));
    HIPCHK(ctx, counts.alloc(sizeof(int32_t) * 3 * (size_t)L));
    HIPCHK(ctx, d_tu.alloc(sizeof(int32_t) * (size_t)N));
    HIPCHK(ctx, d_rank_obs.alloc(sizeof(int32_t) * (size_t)n));
    HIPCHK(ctx, op.alloc((size_t)P * (size_t)R * ldh));
    HIPCHK(ctx, op_obs.alloc((size_t)P * ldh));
    HIPCHK(ctx, dS.alloc(sizeof(int32_t) * (size_t)L));
    HIPCHK(ctx, dV.alloc(sizeof(int64_t) * (size_t)L));
    HIPCHK(ctx, dD.alloc(sizeof(int64_t) * (size_t)L));
    HIPCHK(ctx, dK.alloc(sizeof(double) * (size_t)L));
    HIPCHK(ctx, dC.alloc(sizeof(int32_t) * (size_t)L));
    HIPCHK(ctx, dmax.alloc(sizeof(double) * (size_t)R));
    HIPCHK(ctx, darg.alloc(sizeof(int32_t) * (size_t)R));
    int rc = group_upload(ctx, labels.data(), n, sizes, d_lab);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(d_tu.p, tu.data(), sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_rank_obs.p, rank_obs.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(dC.p, 0, sizeof(int32_t) * (size_t)L, st));
    const int32_t* rank_dev = d_rank_obs.as<int32_t>();
    if (stratified) {
        HIPCHK(ctx, d_rank_fill.alloc(sizeof(int32_t) * (size_t)n));
        HIPCHK(ctx, d_su.alloc(sizeof(uint16_t) * (size_t)N));
        HIPCHK(ctx, hipMemcpyAsync(d_rank_fill.p, rank_fill.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(d_su.p, su.data(), sizeof(uint16_t) * (size_t)N, hipMemcpyHostToDevice, st));
        rank_dev = d_rank_fill.as<int32_t>();
    }
    // every later error path drains the stream first: kernels may be queued on this frame's buffers and host vectors
    auto drain = [&](int code) { (void)hipStreamSynchronize(st); return code; };
    rc = eagle_dev_group_onehot(ctx, d_lab.as<int32_t>(), n, onehot.as<int8_t>(), ldh, st);
    if (!rc) rc = eagle_dev_maxt_operand(ctx, nullptr, NP2, nullptr, N, d_rank_obs.as<int32_t>(), d_tu.as<int32_t>(), n, ldh, P, 1, 0, 1, op_obs.as<int8_t>(), st);
    if (rc) return drain(rc);
    if (perm) {
        const size_t pbytes = sizeof(int32_t) * (size_t)R * (size_t)N;
        hipError_t e = d_perm.alloc(pbytes);
        if (e == hipSuccess) e = hipMemcpyAsync(d_perm.p, perm, pbytes, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return drain(eagle_fail_hip(ctx, e, "maxt: perm upload"));
        rc = eagle_dev_maxt_operand(ctx, nullptr, NP2, d_perm.as<int32_t>(), N, rank_dev, d_tu.as<int32_t>(), n, ldh, P, R, 0, R, op.as<int8_t>(), st);
    } else {
        const hipError_t e = keys.alloc(sizeof(uint64_t) * (size_t)sort_rows * (size_t)NP2);
        if (e != hipSuccess) return drain(eagle_fail_hip(ctx, e, "maxt: keys"));
        for (long r0 = 0; r0 < R && !rc; r0 += sort_rows) {
            const long nr = std::min(sort_rows, R - r0);
            rc = eagle_dev_maxt_permutations(ctx, seed, first + r0, nr, N, NP2, stratified ? d_su.as<uint16_t>() : nullptr, keys.as<uint64_t>(), st);
            if (!rc) rc = eagle_dev_maxt_operand(ctx, keys.as<uint64_t>(), NP2, nullptr, N, rank_dev, d_tu.as<int32_t>(), n, ldh, P, R, r0, nr, op.as<int8_t>(), st);
        }
    }
    if (rc) return drain(rc);

    ImageLines lines;
    rc = lines.open(ctx, f_name_ascii_Mt, L, n, max_memory_in_Gbytes);
    if (rc) return drain(rc);
    const RowWindows ws = lines.disjoint(lines.stream_rows());
    const long wcap = std::min(ws.cap, L), tiles_cap = ((L + wcap - 1) / wcap) * ((wcap + 127) / 128);
    {
        hipError_t e = pkey.alloc(sizeof(double) * (size_t)tiles_cap * (size_t)R);
        if (e == hipSuccess) e = parg.alloc(sizeof(int32_t) * (size_t)tiles_cap * (size_t)R);
        if (e != hipSuccess) return drain(eagle_fail_hip(ctx, e, "maxt: partials"));
    }
    long tile_base = 0;
    rc = lines.each(ws, [&](const int8_t* img, long r0, long nr, long, long) {
        if (tile_base + (nr + 127) / 128 > tiles_cap) return eagle_fail(ctx, EAGLE_ERR_ARG, "maxt: more tiles than planned");
        int32_t* cw = counts.as<int32_t>() + 3 * (size_t)r0;
        int32_t* Sw = dS.as<int32_t>() + r0;
        int64_t* Vw = dV.as<int64_t>() + r0;
        int64_t* Dw = dD.as<int64_t>() + r0;
        double* Kw = dK.as<double>() + r0;
        int32_t* Cw = dC.as<int32_t>() + r0;
        int wrc = eagle_dev_group_counts(ctx, img, nr, n, lines.ld(), onehot.as<int8_t>(), ldh, 1, d_lab.as<int32_t>() + n, cw, st);
        if (!wrc) wrc = eagle_dev_maxt_sv(ctx, cw, nr, N, Sw, Vw, st);
        if (!wrc) wrc = eagle_dev_maxt_tile(ctx, 1, img, nr, n, lines.ld(), op_obs.as<int8_t>(), ldh, P, 1, 1, N, T, Sw, Vw, Dw, Kw, Cw, pkey.as<double>(),
                                            parg.as<int32_t>(), tile_base, r0, st);
        if (!wrc) wrc = eagle_dev_maxt_tile(ctx, 0, img, nr, n, lines.ld(), op.as<int8_t>(), ldh, P, R, R, N, T, Sw, Vw, Dw, Kw, Cw, pkey.as<double>(),
                                            parg.as<int32_t>(), tile_base, r0, st);
        tile_base += (nr + 127) / 128;
        return wrc;
    });
    if (rc) return drain(rc);
    rc = eagle_dev_maxt_finish(ctx, pkey.as<double>(), parg.as<int32_t>(), tile_base, R, dmax.as<double>(), darg.as<int32_t>(), st);
    if (rc) return drain(rc);
    HIPCHK(ctx, hipMemcpyAsync(d_obs, dD.p, sizeof(int64_t) * (size_t)L, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(V, dV.p, sizeof(int64_t) * (size_t)L, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(key_obs, dK.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(count1, dC.p, sizeof(int32_t) * (size_t)L, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(maxkey, dmax.p, sizeof(double) * (size_t)R, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(argmax, darg.p, sizeof(int32_t) * (size_t)R, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return EAGLE_OK;
}

// eagle_bed_marker_counts' windows through the staging ring; the K mask planes are built once per call.
extern "C" int eagle_bed_group_counts(eagle_ctx* ctx, const char* bed_path, const long dims[2], const int32_t* labels, int K,
                                      double max_memory_in_Gbytes, int32_t* counts_out) {
    int32_t sizes[EAGLE_GROUPS_MAX];
    if (int arc = group_args(ctx, "bed_group_counts", bed_path, dims, labels, K, counts_out, sizes)) return arc;
    const long n = dims[0], L = dims[1];
    BedRing ring;
    if (int orc = ring.open(ctx, bed_path, n, L)) return orc;
    const long w = std::min(L, bed_stage_rows(ring.rb, max_memory_in_Gbytes)), nd = (ring.rb + 3) / 4;
    int rc = ring.ensure(w);
    if (rc) return rc;
    const size_t per_row = sizeof(int32_t) * 4 * (size_t)K;
    DevBuf d_lab, planes, counts;
    HIPCHK(ctx, planes.alloc(sizeof(uint32_t) * (size_t)K * (size_t)nd));
    HIPCHK(ctx, counts.alloc(per_row * (size_t)L));
    rc = group_upload(ctx, labels, n, sizes, d_lab);
    if (!rc) rc = eagle_dev_group_bedmask(ctx, d_lab.as<int32_t>(), n, K, planes.as<uint32_t>(), ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    rc = ring.each(L, w, [&](long r0, long nr, const uint8_t* raw) {
        const int brc = eagle_dev_bed_group_counts(ctx, raw, nr, n, K, planes.as<uint32_t>(), d_lab.as<int32_t>() + n,
                                                   counts.as<int32_t>() + 4 * (size_t)K * (size_t)r0, ctx->stream);
        return brc ? brc : ring.release();
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(counts_out, counts.p, per_row * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

extern "C" int eagle_fisher_2x2(eagle_ctx* ctx, const int32_t* tables, long L, double* p_out) {
    if (!tables || !p_out) return qc_fail(ctx, EAGLE_ERR_ARG, "fisher_2x2: NULL argument");
    if (L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "fisher_2x2: the number of tables must be positive");
    for (long i = 0; i < L; i++) {
        const int32_t* t = tables + 4 * i;
        if (t[0] < 0 || t[1] < 0 || t[2] < 0 || t[3] < 0 || (long)t[0] + t[1] + t[2] + t[3] > (1L << 30))
            return qc_fail(ctx, EAGLE_ERR_ARG, "fisher_2x2: an entry is negative or a table sums to more than 2^30");
    }
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "fisher_2x2: no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf dt, dp;
    const size_t tb = sizeof(int32_t) * 4 * (size_t)L;
    HIPCHK(ctx, dt.alloc(tb));
    HIPCHK(ctx, dp.alloc(sizeof(double) * (size_t)L));
    HIPCHK(ctx, hipMemcpyAsync(dt.p, tables, tb, hipMemcpyHostToDevice, ctx->stream));
    int rc = eagle_dev_fisher_2x2(ctx, dt.as<int32_t>(), L, dp.as<double>(), ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    HIPCHK(ctx, hipMemcpyAsync(p_out, dp.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Logistic regression of a binary trait on covariates and one marker at a time (include/eagle_hip.h section 1b''''iv; the kernel is
// in eagle_logit.hip).  eagle_group_counts' routes; the covariates are staged once per call as the n64 x 16 padded image the kernel
// reads (rows of unused individuals zero, so a NaN there is never met) with the status as one byte per individual.
// ---------------------------------------------------------------------------------------------------------------
extern "C" int eagle_logistic(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const int32_t* status, const double* X, int c,
                              const double* beta0, int firth, double tol, int max_iter, double max_memory_in_Gbytes, double* stat_out,
                              int32_t* info_out) {
    auto fail = [&](const char* what) {
        char msg[160];
        snprintf(msg, sizeof msg, "logistic: %s", what);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    };
    if (!f_name_ascii_Mt || !dims || !status || !X || !beta0 || !stat_out || !info_out) return fail("NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return fail("dims must be positive");
    if (n > 0x3fffffffL) return fail("more than 2^30 - 1 individuals");
    if (c < 1 || c > 15) return fail("c outside [1, 15]");
    if (firth < 0 || firth > 2) return fail("firth outside {0, 1, 2}");
    if (!(tol > 0.0 && tol < 1.0)) return fail("tol not in (0, 1)");
    if (max_iter < 1 || max_iter > 1000) return fail("max_iter outside [1, 1000]");
    long ncase = 0, nctrl = 0;
    for (long i = 0; i < n; i++) {
        if (status[i] < -1 || status[i] > 1) return fail("a status outside {-1, 0, 1}");
        if (status[i] < 0) continue;
        (status[i] ? ncase : nctrl)++;
        for (int j = 0; j < c; j++)
            if (!std::isfinite(X[i + (size_t)n * j])) return fail("a non-finite X entry of a used individual");
    }
    for (int j = 0; j < c; j++)
        if (!std::isfinite(beta0[j])) return fail("a non-finite beta0 entry");
    if (!ncase || !nctrl) return fail("no case or no control among the used individuals");
    if (!ctx) return fail("no context");

    const long n64 = (n + 63) / 64 * 64;
    std::vector<double> x16((size_t)n64 * 16, 0.0);
    std::vector<uint8_t> vy((size_t)n64, 0);
    for (long i = 0; i < n; i++) {
        if (status[i] < 0) continue;
        vy[i] = (uint8_t)(2 | status[i]);
        for (int j = 0; j < c; j++) x16[(size_t)i * 16 + j] = X[i + (size_t)n * j];
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf d_x, d_vy, d_b0, stat, info;
    HIPCHK(ctx, d_x.alloc(sizeof(double) * x16.size()));
    HIPCHK(ctx, d_vy.alloc(vy.size()));
    HIPCHK(ctx, d_b0.alloc(sizeof(double) * 16));
    HIPCHK(ctx, stat.alloc(sizeof(double) * 4 * (size_t)L));
    HIPCHK(ctx, info.alloc(sizeof(int32_t) * 2 * (size_t)L));
    HIPCHK(ctx, hipMemcpyAsync(d_x.p, x16.data(), sizeof(double) * x16.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_vy.p, vy.data(), vy.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_b0.p, beta0, sizeof(double) * (size_t)c, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                  // x16 and vy are pageable host vectors
    ImageLines lines;
    int rc = lines.open(ctx, f_name_ascii_Mt, L, n, max_memory_in_Gbytes);
    if (rc) return rc;
    rc = lines.each(lines.disjoint(lines.stream_rows()), [&](const int8_t* img, long r0, long nr, long, long) {
        return eagle_dev_logistic(ctx, img, nr, n, lines.ld(), d_x.as<double>(), d_vy.as<uint8_t>(), d_b0.as<double>(), c + 1, firth, tol, max_iter,
                                  stat.as<double>() + 4 * (size_t)r0, info.as<int32_t>() + 2 * (size_t)r0, ctx->stream);
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(stat_out, stat.p, sizeof(double) * 4 * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(info_out, info.p, sizeof(int32_t) * 2 * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Saddlepoint p-values of the score test under the logistic mixed model (include/eagle_hip.h section 1d'''; the kernel is in
// eagle_glmm.hip).  eagle_logistic's routes; the covariates are staged once per call as eagle_logistic stages them, mu, 1 - mu,
// D = mu (1 - mu) and the residual as a second padded image of four columns, (X'DX)^-1 as a 16 x 16 one.
// ---------------------------------------------------------------------------------------------------------------
extern "C" int eagle_glmm_spa(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const double* mu, const double* resid,
                              const double* X, int c, const double* A, const double* vara_or_NULL, double cutoff, double tol, int max_iter,
                              double max_memory_in_Gbytes, double* stat_out, int32_t* info_out) {
    auto fail = [&](const char* what) {
        char msg[160];
        snprintf(msg, sizeof msg, "glmm_spa: %s", what);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    };
    if (!f_name_ascii_Mt || !dims || !mu || !resid || !X || !A || !stat_out || !info_out) return fail("NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return fail("dims must be positive");
    if (n > 0x3fffffffL) return fail("more than 2^30 - 1 individuals");
    if (c < 1 || c > 15) return fail("c outside [1, 15]");
    for (long i = 0; i < n; i++)
        if (!(mu[i] > 0.0 && mu[i] < 1.0)) return fail("a mu outside (0, 1)");
    for (long i = 0; i < n; i++) {
        if (!std::isfinite(resid[i])) return fail("a non-finite resid entry");
        for (int j = 0; j < c; j++)
            if (!std::isfinite(X[i + (size_t)n * j])) return fail("a non-finite X entry");
    }
    for (int j = 0; j < c * c; j++)
        if (!std::isfinite(A[j])) return fail("a non-finite A entry");
    if (!(cutoff >= 0.0)) return fail("cutoff negative or NaN");
    if (!(tol > 0.0 && tol < 1.0)) return fail("tol not in (0, 1)");
    if (max_iter < 1 || max_iter > 1000) return fail("max_iter outside [1, 1000]");
    if (!ctx) return fail("no context");

    const long n64 = (n + 63) / 64 * 64;
    std::vector<double> x16((size_t)n64 * 16, 0.0), p4((size_t)n64 * 4, 0.0), a16(256, 0.0);
    for (long i = 0; i < n64; i++) {
        double* p = &p4[(size_t)i * 4];
        if (i >= n) { p[0] = p[1] = 0.5; continue; }
        p[0] = mu[i];
        p[1] = 1.0 - mu[i];
        p[2] = mu[i] * (1.0 - mu[i]);
        p[3] = resid[i];
        for (int j = 0; j < c; j++) x16[(size_t)i * 16 + j] = X[i + (size_t)n * j];
    }
    for (int i = 0; i < c; i++)
        for (int j = 0; j < c; j++) a16[i * 16 + j] = A[i + (size_t)c * j];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf d_x, d_p4, d_a16, d_vara, stat, info;
    HIPCHK(ctx, d_x.alloc(sizeof(double) * x16.size()));
    HIPCHK(ctx, d_p4.alloc(sizeof(double) * p4.size()));
    HIPCHK(ctx, d_a16.alloc(sizeof(double) * a16.size()));
    if (vara_or_NULL) HIPCHK(ctx, d_vara.alloc(sizeof(double) * (size_t)L));
    HIPCHK(ctx, stat.alloc(sizeof(double) * 7 * (size_t)L));
    HIPCHK(ctx, info.alloc(sizeof(int32_t) * 2 * (size_t)L));
    HIPCHK(ctx, hipMemcpyAsync(d_x.p, x16.data(), sizeof(double) * x16.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_p4.p, p4.data(), sizeof(double) * p4.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_a16.p, a16.data(), sizeof(double) * a16.size(), hipMemcpyHostToDevice, ctx->stream));
    if (vara_or_NULL) HIPCHK(ctx, hipMemcpyAsync(d_vara.p, vara_or_NULL, sizeof(double) * (size_t)L, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                  // the staged images are pageable host vectors
    ImageLines lines;
    int rc = lines.open(ctx, f_name_ascii_Mt, L, n, max_memory_in_Gbytes);
    if (rc) return rc;
    rc = lines.each(lines.disjoint(lines.stream_rows()), [&](const int8_t* img, long r0, long nr, long, long) {
        return eagle_dev_glmm_spa(ctx, img, nr, n, lines.ld(), d_x.as<double>(), d_p4.as<double>(), d_a16.as<double>(), c,
                                  vara_or_NULL ? d_vara.as<double>() + (size_t)r0 : nullptr, cutoff, tol, max_iter,
                                  stat.as<double>() + 7 * (size_t)r0, info.as<int32_t>() + 2 * (size_t)r0, ctx->stream);
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(stat_out, stat.p, sizeof(double) * 7 * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(info_out, info.p, sizeof(int32_t) * 2 * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Admixture: EM steps of the ancestry model (include/eagle_hip.h section 1b''''v; the kernels are in eagle_admix.hip).
// eagle_group_counts' routes, one pass over the image per step and one more for the likelihood of the result.  Q and F are staged once
// per call as 16-column padded images, the steps alternate between two buffers of each, and nothing comes back before the last pass.
// The streamed windows' cap (lines.stream_rows(): a multiple of 256) is a multiple of 16, which the kernels' tiles and ranges need.
// ---------------------------------------------------------------------------------------------------------------
extern "C" int eagle_admixture_em(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], int K, int steps, double* Q, double* F,
                                  double max_memory_in_Gbytes, double* loglik_out) {
    auto fail = [&](const char* what) {
        char msg[160];
        snprintf(msg, sizeof msg, "admixture_em: %s", what);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    };
    if (!f_name_ascii_Mt || !dims || !Q || !F || !loglik_out) return fail("NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return fail("dims must be positive");
    if (n > 0x3fffffffL) return fail("more than 2^30 - 1 individuals");
    if (K < 1 || K > EAGLE_ADMIX_KMAX) return fail("K outside [1, 16]");
    if (steps < 0 || steps > 10000) return fail("steps outside [0, 10000]");
    for (long i = 0; i < n; i++) {
        double sum = 0.0;
        for (int k = 0; k < K; k++) {
            const double q = Q[(size_t)i * K + k];
            if (!std::isfinite(q)) return fail("a non-finite Q entry");
            if (q < 0.0) return fail("a negative Q entry");
            sum += q;
        }
        if (!(fabs(sum - 1.0) <= 1e-9)) return fail("a Q row whose sum is off 1 by more than 1e-9");
    }
    for (size_t e = 0; e < (size_t)L * K; e++) {
        if (!std::isfinite(F[e])) return fail("a non-finite F entry");
        if (F[e] < EAGLE_ADMIX_EPS || F[e] > 1.0 - EAGLE_ADMIX_EPS) return fail("an F entry outside [eps, 1 - eps]");
    }
    if (!ctx) return fail("no context");

    const long n16 = (n + 15) / 16 * 16, L16 = (L + 15) / 16 * 16;
    const AdmixPlan plan = admix_range_plan(n, L);
    std::vector<double> q16((size_t)n16 * 16, 0.0), f16((size_t)L16 * 16, 0.0);
    for (long i = 0; i < n; i++)
        for (int k = 0; k < K; k++) q16[(size_t)i * 16 + k] = Q[(size_t)i * K + k];
    for (long m = 0; m < L; m++)
        for (int k = 0; k < K; k++) f16[(size_t)m * 16 + k] = F[(size_t)m * K + k];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t qb = sizeof(double) * q16.size(), fb = sizeof(double) * f16.size();
    DevBuf dq[2], df[2], llpart, part, ll;
    for (int b = 0; b < 2; b++) {
        HIPCHK(ctx, dq[b].alloc(qb));
        HIPCHK(ctx, df[b].alloc(fb));
    }
    HIPCHK(ctx, llpart.alloc(sizeof(double) * (size_t)(L16 / 16)));
    HIPCHK(ctx, part.alloc(sizeof(double) * 16 * (size_t)plan.S * (size_t)n16));
    HIPCHK(ctx, ll.alloc(sizeof(double) * ((size_t)steps + 1)));
    HIPCHK(ctx, hipMemcpyAsync(dq[0].p, q16.data(), qb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(df[0].p, f16.data(), fb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(dq[1].p, 0, qb, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(df[1].p, 0, fb, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                  // q16 and f16 are pageable host vectors
    ImageLines lines;
    int rc = lines.open(ctx, f_name_ascii_Mt, L, n, max_memory_in_Gbytes);
    if (rc) return rc;
    int cur = 0;
    for (int t = 0; t <= steps; t++) {                               // pass t: the likelihood at the parameters entering step t, and the step
        const int update = t < steps;
        rc = lines.each(lines.disjoint(lines.stream_rows()), [&](const int8_t* img, long r0, long nr, long, long) {
            return eagle_dev_admix_window(ctx, img, r0, nr, n, L, lines.ld(), K, update, dq[cur].as<double>(), df[cur].as<double>(),
                                          df[cur ^ 1].as<double>(), llpart.as<double>(), part.as<double>(), (int)plan.S, plan.len, ctx->stream);
        });
        if (rc) return rc;
        rc = eagle_dev_admix_finish(ctx, n, L, K, update, llpart.as<double>(), ll.as<double>() + t, part.as<double>(), (int)plan.S,
                                    dq[cur].as<double>(), dq[cur ^ 1].as<double>(), ctx->stream);
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        if (update) cur ^= 1;
    }
    HIPCHK(ctx, hipMemcpyAsync(q16.data(), dq[cur].p, qb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(f16.data(), df[cur].p, fb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(loglik_out, ll.p, sizeof(double) * ((size_t)steps + 1), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (long i = 0; i < n; i++)
        for (int k = 0; k < K; k++) Q[(size_t)i * K + k] = q16[(size_t)i * 16 + k];
    for (long m = 0; m < L; m++)
        for (int k = 0; k < K; k++) F[(size_t)m * K + k] = f16[(size_t)m * 16 + k];
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// kNN imputation of a .bed file (no counterpart in the reference; kernels in eagle_impute.hip)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int eagle_knn_rows(eagle_ctx* ctx, const int32_t* ibs0, const int32_t* hethet, long n, int K, int32_t* nbr_out) {
    if (!ibs0 || !hethet || !nbr_out) return qc_fail(ctx, EAGLE_ERR_ARG, "knn_rows: NULL argument");
    if (n <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "knn_rows: n must be positive");
    if (n > EAGLE_KNN_MAX_N) return qc_fail(ctx, EAGLE_ERR_ARG, "knn_rows: more than EAGLE_KNN_MAX_N individuals");
    if (K < 1 || K > EAGLE_KNN_MAX_K) return qc_fail(ctx, EAGLE_ERR_ARG, "knn_rows: K outside [1, 256]");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "knn_rows: no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t mb = sizeof(int32_t) * (size_t)n * (size_t)n, nb = sizeof(int32_t) * (size_t)n * (size_t)K;
    DevBuf d0, dh, dn;
    HIPCHK(ctx, d0.alloc(mb));
    HIPCHK(ctx, dh.alloc(mb));
    HIPCHK(ctx, dn.alloc(nb));
    HIPCHK(ctx, hipMemcpyAsync(d0.p, ibs0, mb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dh.p, hethet, mb, hipMemcpyHostToDevice, ctx->stream));
    int rc = eagle_dev_knn_rows(ctx, d0.as<int32_t>(), dh.as<int32_t>(), n, K, dn.as<int32_t>(), ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    HIPCHK(ctx, hipMemcpyAsync(nbr_out, dn.p, nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

// The windows of eagle_bed_marker_counts through the staging ring, with BedRewrite's write-behind.  Window k: count (the fallback
// genotypes), patch into `patched`.
extern "C" int eagle_bed_impute_knn(eagle_ctx* ctx, const char* bed_path, const long dims[2], const int32_t* nbr, int K, int k, int min_votes,
                                    const char* out_bed_path, double max_memory_in_Gbytes, int32_t* counts_out) {
    if (!bed_path || !dims || !nbr || !out_bed_path) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_knn: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_knn: dims must be positive");
    if (n > EAGLE_IMPUTE_MAX_N) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_knn: more than EAGLE_IMPUTE_MAX_N individuals");
    if (K < 1 || K > EAGLE_KNN_MAX_K) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_knn: K outside [1, 256]");
    if (k < 1 || k > K) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_knn: k outside [1, K]");
    if (min_votes < 1) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_knn: min_votes must be at least 1");
    if (std::string(bed_path) == out_bed_path) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_knn: the output file must differ from the input file");
    const size_t nn = (size_t)n * (size_t)K;
    for (size_t i = 0; i < nn; i++)
        if (nbr[i] < -1 || nbr[i] >= n) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_knn: a neighbour outside [-1, n)");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_knn: no context");
    BedRing ring;
    if (int orc = ring.open(ctx, bed_path, n, L)) return orc;
    const long rb = ring.rb, w = std::min(L, bed_stage_rows(rb, max_memory_in_Gbytes));
    int rc = ring.ensure(w);
    if (rc) return rc;
    DevBuf d_nbr, mcounts, counts, patched;
    HIPCHK(ctx, d_nbr.alloc(sizeof(int32_t) * nn));
    HIPCHK(ctx, mcounts.alloc(sizeof(int32_t) * 4 * (size_t)w));
    HIPCHK(ctx, counts.alloc(sizeof(int32_t) * 2 * (size_t)L));
    HIPCHK(ctx, patched.alloc((size_t)w * rb));
    HIPCHK(ctx, hipMemcpyAsync(d_nbr.p, nbr, sizeof(int32_t) * nn, hipMemcpyHostToDevice, ctx->stream));
    BedRewrite out;
    if (int orc = out.open(ctx, out_bed_path, n, L)) return orc;
    for (long r0 = 0; r0 < L; r0 += w) {
        const long nr = std::min(w, L - r0);
        const uint8_t* raw;
        rc = ring.stage(r0, nr, &raw);
        if (!rc) rc = eagle_dev_bed_marker_counts(ctx, raw, nr, n, mcounts.as<int32_t>(), ctx->stream);
        if (!rc) rc = eagle_dev_bed_impute(ctx, raw, nr, n, d_nbr.as<int32_t>(), K, k, min_votes, mcounts.as<int32_t>(), patched.as<uint8_t>(),
                                           counts.as<int32_t>() + 2 * r0, ctx->stream);
        if (!rc) rc = out.push(ring, patched.p, r0, nr);
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    }
    if (counts_out) HIPCHK(ctx, hipMemcpyAsync(counts_out, counts.p, sizeof(int32_t) * 2 * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return out.finish(ring);
}

// LD-kNNi (kernel in eagle_ldknn.hip).  The ring and the write-behind of eagle_bed_impute_knn; the rows staged for window [r0, r0 + nr) are
// [max(0, r0 - 256), min(L, r0 + nr + 256)): every partner of every marker of the window (checked below to lie within 256 rows of it) is
// among them.  The halo is read again with the next window -- from the page cache -- so that a window is one pread and one upload.
#define LDKNN_HALO 256L
extern "C" int eagle_bed_impute_ldknn(eagle_ctx* ctx, const char* bed_path, const long dims[2], const int32_t* partners, int l, int k, int min_votes,
                                      int min_overlap, const char* out_bed_path, double max_memory_in_Gbytes, int32_t* counts_out) {
    if (!bed_path || !dims || !partners || !out_bed_path) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_ldknn: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0 || L > 0x7fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_ldknn: dims must be positive (L below 2^31)");
    if (n > EAGLE_LDKNN_MAX_N) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_ldknn: more than EAGLE_LDKNN_MAX_N individuals");
    if (l < 1 || l > EAGLE_LDKNN_MAX_PARTNERS) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_ldknn: l outside [1, 32]");
    if (k < 1 || k > EAGLE_LDKNN_MAX_K) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_ldknn: k outside [1, 64]");
    if (min_votes < 1) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_ldknn: min_votes must be at least 1");
    if (min_overlap < 1 || min_overlap > EAGLE_LDKNN_MAX_PARTNERS) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_ldknn: min_overlap outside [1, 32]");
    if (std::string(bed_path) == out_bed_path) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_ldknn: the output file must differ from the input file");
    for (long m = 0; m < L; m++)
        for (int t = 0; t < l; t++) {
            const long p = partners[(size_t)m * (size_t)l + (size_t)t];
            if (p < -1 || p >= L) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_ldknn: a partner outside [-1, L)");
            if (p >= 0 && (p - m > LDKNN_HALO || m - p > LDKNN_HALO))
                return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_ldknn: a partner more than 256 rows from its marker");
        }
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_impute_ldknn: no context");
    BedRing ring;
    if (int orc = ring.open(ctx, bed_path, n, L)) return orc;
    const long rb = ring.rb, w = std::min(L, bed_stage_rows(rb, max_memory_in_Gbytes));
    int rc = ring.ensure(std::min(L, w + 2 * LDKNN_HALO));   // rows staged for a window, at most
    if (rc) return rc;
    const size_t np = (size_t)L * (size_t)l;
    DevBuf d_part, mcounts, counts, patched;
    HIPCHK(ctx, d_part.alloc(sizeof(int32_t) * np));
    HIPCHK(ctx, mcounts.alloc(sizeof(int32_t) * 4 * (size_t)w));
    HIPCHK(ctx, counts.alloc(sizeof(int32_t) * 2 * (size_t)L));
    HIPCHK(ctx, patched.alloc((size_t)w * rb));
    HIPCHK(ctx, hipMemcpyAsync(d_part.p, partners, sizeof(int32_t) * np, hipMemcpyHostToDevice, ctx->stream));
    BedRewrite out;
    if (int orc = out.open(ctx, out_bed_path, n, L)) return orc;
    for (long r0 = 0; r0 < L; r0 += w) {
        const long nr = std::min(w, L - r0);
        const long h_lo = std::max(0L, r0 - LDKNN_HALO), h_hi = std::min(L, r0 + nr + LDKNN_HALO), staged = h_hi - h_lo;
        const uint8_t* raw;
        rc = ring.stage(h_lo, staged, &raw);
        if (!rc) rc = eagle_dev_bed_marker_counts(ctx, raw + (r0 - h_lo) * rb, nr, n, mcounts.as<int32_t>(), ctx->stream);
        if (!rc) rc = eagle_dev_bed_impute_ldknn(ctx, raw, staged, r0 - h_lo, nr, r0, h_lo, n, d_part.as<int32_t>(), l, k, min_votes, min_overlap,
                                                 mcounts.as<int32_t>(), patched.as<uint8_t>(), counts.as<int32_t>() + 2 * r0, ctx->stream);
        if (!rc) rc = out.push(ring, patched.p, r0, nr);
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    }
    if (counts_out) HIPCHK(ctx, hipMemcpyAsync(counts_out, counts.p, sizeof(int32_t) * 2 * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return out.finish(ring);
}

namespace {

// One of the two output files of eagle_filter_markers: `rows` lines of `cols` characters with sidecar, made band by band of `band`
// rows (a multiple of 256; one band when the image is kept) by fill(r0, nr, tile), which leaves the int8 rows [r0, r0 + nr) of the
// subset at `tile` (leading dimension ld, every byte beyond the subset zero), and adopted as the resident copy when `keep`.
template <class Fill>
int filter_write(eagle_ctx* ctx, const char* path, long rows, long cols, long rows_pad, long ld, long band, bool keep, int threads, Fill fill) {
    const long chunk = std::max(1L, std::min(rows, (long)(67108864 / (cols + 1))));
    int rc = eagle_stage_ensure(ctx, (size_t)chunk * (cols + 1));
    if (rc) return rc;
    DevBuf img;
    HIPCHK(ctx, img.alloc((size_t)(keep ? rows_pad : band) * ld));
    EventPair done;
    HIPCHK(ctx, done.create());
    TextOut out;
    if (!out.open_sized(path, (off_t)rows * (cols + 1))) return failf(ctx, EAGLE_ERR_OPEN, "ERROR: Could not open  %s", path);
    SidecarWriter sc;
    (void)sc.open_for(ctx, path, rows, cols, chunk);
    for (long r0 = 0; r0 < rows; r0 += band) {
        const long nr = std::min(band, rows - r0);
        int8_t* tile = img.as<int8_t>() + (keep ? r0 * ld : 0);
        rc = fill(r0, nr, std::min(band, rows_pad - r0), tile);
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        rc = write_lines_from_image(ctx, out.fd, path, tile, ld, r0, nr, cols, chunk, sc, done, threads);
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    out.finish();  // the text file is final: its size and mtime key the sidecar and the cache entry
    sc.finish(path);
    if (keep) {
        int8_t* give = img.as<int8_t>();
        img.p = nullptr;
        return eagle_cache_adopt(ctx, path, rows, cols, rows_pad, ld, give);
    }
    return EAGLE_OK;
}

}  // namespace

// Mt first (row copies of the kept markers), then M (the kept columns of every individual), each from the resident image of its source
// when there is one -- k_gather_rows_i8 / k_gather_cols_i8, HBM to HBM -- and else from windows of the source: the kept lines of
// Mt.ascii as runs through the staged reader, bands of whole lines of M.ascii gathered on the device.  Both outputs are written by the
// code that writes the converters' files, from images with the padding a freshly loaded file of (n, nkeep) has.
extern "C" int eagle_filter_markers(eagle_ctx* ctx, const char* fnameM, const char* fnameMt, const long dims[2], const long* keep, long nkeep,
                                    const char* outM, const char* outMt, double max_memory_in_Gbytes, long newdims_out[2]) {
    if (!fnameM || !fnameMt || !dims || !outM || !outMt || !newdims_out) return qc_fail(ctx, EAGLE_ERR_ARG, "filter_markers: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0 || L > 0x7fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "filter_markers: bad dims");
    if (!keep || nkeep <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "filter_markers: the keep-list is empty");
    for (long i = 0; i < nkeep; i++) {
        if (keep[i] < 0 || keep[i] >= L) return qc_fail(ctx, EAGLE_ERR_ARG, "filter_markers: keep-list entry outside [0, L)");
        if (i > 0 && keep[i] <= keep[i - 1]) return qc_fail(ctx, EAGLE_ERR_ARG, "filter_markers: the keep-list must be strictly increasing");
    }
    const std::string sM = fnameM, sMt = fnameMt, oM = outM, oMt = outMt;
    if (oM == sM || oM == sMt || oMt == sM || oMt == sMt || oM == oMt)
        return qc_fail(ctx, EAGLE_ERR_ARG, "filter_markers: the output files must differ from the input files and from each other");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "filter_markers: no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int threads = host_threads();
    const long Lk = nkeep, n_pad = eagle_pad(n), L_pad = eagle_pad(L), Lk_pad = eagle_pad(Lk);
    std::vector<int32_t> keep32((size_t)Lk);
    for (long i = 0; i < Lk; i++) keep32[(size_t)i] = (int32_t)keep[i];
    DevBuf d_keep;
    HIPCHK(ctx, d_keep.alloc(sizeof(int32_t) * (size_t)Lk));
    HIPCHK(ctx, hipMemcpyAsync(d_keep.p, keep32.data(), sizeof(int32_t) * (size_t)Lk, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t budget = eagle_resident_budget();

    {   // Mt: nkeep lines of n characters
        const GenoEntry* g = nullptr;
        int rc = eagle_get_resident(ctx, fnameMt, L, n, max_memory_in_Gbytes, threads, &g);
        if (rc != EAGLE_OK && rc != EAGLE_STREAM) return rc;
        const int8_t* src = g ? g->dev : nullptr;
        const long ld_src = g ? g->ld : 0;
        const bool keepimg = fits_resident((size_t)Lk_pad * n_pad);
        const long band = keepimg ? Lk_pad : stream_chunk_rows_core(budget, n_pad, Lk_pad);
        rc = filter_write(ctx, outMt, Lk, n, Lk_pad, n_pad, band, keepimg, threads, [&](long r0, long nr, long padded, int8_t* tile) -> int {
            if (src) return eagle_dev_gather_rows_i8(ctx, src, ld_src, d_keep.as<int32_t>() + r0, nr, padded, tile, n_pad, ctx->stream);
            HIPCHK(ctx, hipMemsetAsync(tile, 0, (size_t)padded * n_pad, ctx->stream));
            std::vector<RowRun> runs;
            append_keep_runs(keep32.data() + r0, nr, runs);
            return eagle_load_rows(ctx, fnameMt, runs, 0, n, tile, n_pad, max_memory_in_Gbytes, threads);
        });
        if (rc) return rc;
    }
    {   // M: n lines of nkeep characters
        const GenoEntry* g = nullptr;
        int rc = eagle_get_resident(ctx, fnameM, n, L, max_memory_in_Gbytes, threads, &g);
        if (rc != EAGLE_OK && rc != EAGLE_STREAM) return rc;
        const int8_t* src = g ? g->dev : nullptr;
        const long ld_src = g ? g->ld : L_pad;
        const bool keepimg = src && fits_resident((size_t)n_pad * Lk_pad);
        const long band = keepimg ? n_pad : stream_chunk_rows_core(budget, L_pad, n_pad);
        DevBuf win;   // a band of whole lines of M.ascii when the source is not resident
        if (!src) HIPCHK(ctx, win.alloc((size_t)band * L_pad));
        rc = filter_write(ctx, outM, n, Lk, n_pad, Lk_pad, band, keepimg, threads, [&](long r0, long nr, long padded, int8_t* tile) -> int {
            HIPCHK(ctx, hipMemsetAsync(tile, 0, (size_t)padded * Lk_pad, ctx->stream));
            const int8_t* s = src ? src + r0 * ld_src : win.as<int8_t>();
            if (!src) {
                int r = eagle_dev_load_ascii(ctx, fnameM, r0, nr, 0, L, win.as<int8_t>(), L_pad, max_memory_in_Gbytes, threads);
                if (r) return r;
            }
            return eagle_dev_gather_cols_i8(ctx, s, ld_src, d_keep.as<int32_t>(), 0, nr, Lk, tile, Lk_pad, ctx->stream);
        });
        if (rc) return rc;
    }
    newdims_out[0] = n;
    newdims_out[1] = Lk;
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Linkage disequilibrium between markers (no counterpart in the reference; kernels in eagle_ld.hip)
// ---------------------------------------------------------------------------------------------------------------
namespace {

// (s, q) of the `rows` markers of an int8 Mt tile: k_marker_counts, then k_ld_sq
int ld_tile_sq(eagle_ctx* ctx, const int8_t* img, long rows, long n, long ld, int32_t* counts, int32_t* sq) {
    int rc = eagle_dev_marker_counts(ctx, img, rows, n, ld, counts, ctx->stream);
    if (rc) return rc;
    return eagle_dev_ld_sq(ctx, counts, rows, sq, ctx->stream);
}

// Rows of a streamed window of Mt: the streamed scans' rule, and at least 512 so that windows overlapping by up to 256 rows advance.
long ld_stream_rows(const ImageLines& lines) { return std::max(512L, lines.stream_rows()); }

}  // namespace

// The mask of a resident image is one launch over it.  A file that is not resident is read in windows of w rows that start every
// w - window rows: a window's launch writes the mask rows of all its markers, those of its last `window` markers without the partners
// the window does not hold, and the next window, which starts on exactly those markers, writes them again in full (stream order).
// Every marker's final words therefore come from a launch that held all of its partners: the bits of the resident pass.
extern "C" int eagle_ld_window(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], long window, double r2,
                               double max_memory_in_Gbytes, uint64_t* mask_out, long* npairs_out) {
    if (!f_name_ascii_Mt || !dims || !mask_out || !npairs_out) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_window: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_window: dims must be positive");
    if (window < 1 || window > 256) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_window: window must be in [1, 256]");
    if (!(r2 >= 0.0 && r2 <= 1.0)) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_window: r2 must be in [0, 1]");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_window: no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long wpr = (window + 63) / 64;
    const size_t mask_bytes = sizeof(uint64_t) * (size_t)L * (size_t)wpr;
    DevBuf mask, counts, sq;
    HIPCHK(ctx, mask.alloc(mask_bytes));
    ImageLines lines;
    int rc = lines.open(ctx, f_name_ascii_Mt, L, n, max_memory_in_Gbytes);
    if (rc) return rc;
    const long ld = lines.ld();
    const RowWindows ws = lines.resident() ? row_windows_disjoint(L, L) : row_windows_overlapped(L, ld_stream_rows(lines), window);
    HIPCHK(ctx, counts.alloc(sizeof(int32_t) * 3 * (size_t)ws.cap));
    HIPCHK(ctx, sq.alloc(sizeof(int32_t) * 2 * (size_t)ws.cap));
    rc = lines.each(ws, [&](const int8_t* img, long r0, long nr, long, long) {
        const int trc = ld_tile_sq(ctx, img, nr, n, ld, counts.as<int32_t>(), sq.as<int32_t>());
        return trc ? trc : eagle_dev_ld_band(ctx, img, nr, n, ld, sq.as<int32_t>(), window, r2, mask.as<uint64_t>() + r0 * wpr, wpr, ctx->stream);
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(mask_out, mask.p, mask_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    long pairs = 0;
    for (size_t x = 0; x < (size_t)L * (size_t)wpr; x++) pairs += __builtin_popcountll(mask_out[x]);
    *npairs_out = pairs;
    return EAGLE_OK;
}

// Ranked partner lists, LD scores and the decay curve.  The panel is worked on in CORE ranges of markers: the rows held for a core
// [c0, c1) are [max(0, c0 - window), min(L, c1 + window)) -- all candidates of its markers on both sides -- the tile kernel writes the
// r^2 band of the rows held, and consume(band, rows held, c0 - lo, c1 - lo, lo) works on the core alone (k_ld_partners: the partner
// rows; k_ld_reduce: the sums), so every output word is written once, from a band that held all of the marker's candidates, and every
// pair belongs to one core: the result does not depend on the cores' size.  A resident image is cut only where its band would pass
// 256 MiB; a file that is not resident is read in row windows of the streamed scans' size (at least 1,024 rows: twice the widest
// overlap and a core).
namespace {

template <class Consume>
int ld_panel_cores(eagle_ctx* ctx, const char* f_name_ascii_Mt, long n, long L, long window, double max_memory_in_Gbytes, Consume consume) {
    DevBuf counts, sq, band;
    ImageLines lines;
    int rc = lines.open(ctx, f_name_ascii_Mt, L, n, max_memory_in_Gbytes);
    if (rc) return rc;
    const long ld = lines.ld();
    // rows held for a core, at most
    const long held_max = std::min(L, std::max(1024L, lines.resident() ? (long)(((size_t)256 << 20) / (sizeof(double) * (size_t)window)) : lines.stream_rows()));
    HIPCHK(ctx, counts.alloc(sizeof(int32_t) * 3 * (size_t)held_max));
    HIPCHK(ctx, sq.alloc(sizeof(int32_t) * 2 * (size_t)held_max));
    HIPCHK(ctx, band.alloc(sizeof(double) * (size_t)held_max * (size_t)window));
    rc = lines.each(row_windows_cores(L, held_max, window), [&](const int8_t* img, long lo, long nr, long c0, long c1) {
        int brc = ld_tile_sq(ctx, img, nr, n, ld, counts.as<int32_t>(), sq.as<int32_t>());
        if (!brc) brc = eagle_dev_ld_r2band(ctx, img, nr, n, ld, sq.as<int32_t>(), window, band.as<double>(), ctx->stream);
        return brc ? brc : consume(band.as<double>(), nr, c0 - lo, c1 - lo, lo);
    });
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // the band leaves with this frame
    return EAGLE_OK;
}

// What eagle_ld_stats and eagle_bed_ld_stats hold on the device besides the band, and the argument checks they share (include/
// eagle_hip.h section 1b'''v; lp = the panel's markers; the rule itself is eagle_host.h's ld_stats_arg_error).
struct LdStatsBufs {
    DevBuf U, cnt, chrom, pos, edges, bsum, bpairs;
    int nbins = 0;
    long lp = 0;
};

int ld_stats_check(eagle_ctx* ctx, const char* who, long lp, long window, const int64_t* pos, long max_dist, const int64_t* edges, long nbins,
                   const void* bin_sum_out, const void* bin_pairs_out) {
    const char* bad = ld_stats_arg_error(lp, window, pos != nullptr, max_dist, edges, nbins, bin_sum_out && bin_pairs_out);
    if (!bad) return EAGLE_OK;
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", who, bad);
    return qc_fail(ctx, EAGLE_ERR_ARG, msg);
}

int ld_stats_begin(eagle_ctx* ctx, LdStatsBufs& b, long lp, const int32_t* chrom, const int64_t* pos, const int64_t* edges, long nbins) {
    b.lp = lp;
    b.nbins = edges ? (int)nbins : 0;
    HIPCHK(ctx, b.U.alloc(sizeof(uint64_t) * (size_t)lp));
    HIPCHK(ctx, b.cnt.alloc(sizeof(int32_t) * (size_t)lp));
    if (chrom) {
        HIPCHK(ctx, b.chrom.alloc(sizeof(int32_t) * (size_t)lp));
        HIPCHK(ctx, hipMemcpyAsync(b.chrom.p, chrom, sizeof(int32_t) * (size_t)lp, hipMemcpyHostToDevice, ctx->stream));
    }
    if (pos) {
        HIPCHK(ctx, b.pos.alloc(sizeof(int64_t) * (size_t)lp));
        HIPCHK(ctx, hipMemcpyAsync(b.pos.p, pos, sizeof(int64_t) * (size_t)lp, hipMemcpyHostToDevice, ctx->stream));
    }
    if (b.nbins) {
        HIPCHK(ctx, b.edges.alloc(sizeof(int64_t) * (size_t)(b.nbins + 1)));
        HIPCHK(ctx, b.bsum.alloc(sizeof(uint64_t) * (size_t)b.nbins));
        HIPCHK(ctx, b.bpairs.alloc(sizeof(int64_t) * (size_t)b.nbins));
        HIPCHK(ctx, hipMemcpyAsync(b.edges.p, edges, sizeof(int64_t) * (size_t)(b.nbins + 1), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(b.bsum.p, 0, sizeof(uint64_t) * (size_t)b.nbins, ctx->stream));   // once, before the first core
        HIPCHK(ctx, hipMemsetAsync(b.bpairs.p, 0, sizeof(int64_t) * (size_t)b.nbins, ctx->stream));
    }
    return EAGLE_OK;
}

int ld_stats_core(eagle_ctx* ctx, LdStatsBufs& b, const double* band, long nr, long window, long c_lo, long c_hi, long g0, long max_dist) {
    return eagle_dev_ld_reduce(ctx, band, nr, window, c_lo, c_hi, g0, b.chrom.p ? b.chrom.as<int32_t>() : nullptr,
                               b.pos.p ? b.pos.as<int64_t>() : nullptr, max_dist, b.nbins ? b.edges.as<int64_t>() : nullptr, b.nbins,
                               b.U.as<uint64_t>(), b.cnt.as<int32_t>(), b.nbins ? b.bsum.as<uint64_t>() : nullptr,
                               b.nbins ? b.bpairs.as<int64_t>() : nullptr, ctx->stream);
}

int ld_stats_end(eagle_ctx* ctx, LdStatsBufs& b, uint64_t* U_out, int32_t* cnt_out, uint64_t* bin_sum_out, int64_t* bin_pairs_out) {
    HIPCHK(ctx, hipMemcpyAsync(U_out, b.U.p, sizeof(uint64_t) * (size_t)b.lp, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(cnt_out, b.cnt.p, sizeof(int32_t) * (size_t)b.lp, hipMemcpyDeviceToHost, ctx->stream));
    if (b.nbins) {
        HIPCHK(ctx, hipMemcpyAsync(bin_sum_out, b.bsum.p, sizeof(uint64_t) * (size_t)b.nbins, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(bin_pairs_out, b.bpairs.p, sizeof(int64_t) * (size_t)b.nbins, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

}  // namespace

extern "C" int eagle_ld_partners(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], long window, int l, double min_r2,
                                 const int32_t* chrom, double max_memory_in_Gbytes, int32_t* partners_out, double* r2_out) {
    if (!f_name_ascii_Mt || !dims || !partners_out) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_partners: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_partners: dims must be positive");
    if (L > 0x7fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_partners: 2^31 markers or more");
    if (window < 1 || window > 256) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_partners: window must be in [1, 256]");
    if (l < 1 || l > EAGLE_LDKNN_MAX_PARTNERS) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_partners: l outside [1, 32]");
    if (!(min_r2 >= 0.0 && min_r2 <= 1.0)) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_partners: min_r2 must be in [0, 1]");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_partners: no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)L * (size_t)l;
    DevBuf part, r2, d_chrom;
    HIPCHK(ctx, part.alloc(sizeof(int32_t) * cells));
    HIPCHK(ctx, r2.alloc(sizeof(double) * cells));
    if (chrom) {
        HIPCHK(ctx, d_chrom.alloc(sizeof(int32_t) * (size_t)L));
        HIPCHK(ctx, hipMemcpyAsync(d_chrom.p, chrom, sizeof(int32_t) * (size_t)L, hipMemcpyHostToDevice, ctx->stream));
    }
    int rc = ld_panel_cores(ctx, f_name_ascii_Mt, n, L, window, max_memory_in_Gbytes, [&](const double* band, long nr, long c_lo, long c_hi, long g0) {
        return eagle_dev_ld_partners(ctx, band, nr, window, c_lo, c_hi, g0, chrom ? d_chrom.as<int32_t>() : nullptr, min_r2, l, part.as<int32_t>(),
                                     r2.as<double>(), ctx->stream);
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(partners_out, part.p, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, ctx->stream));
    if (r2_out) HIPCHK(ctx, hipMemcpyAsync(r2_out, r2.p, sizeof(double) * cells, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

// eagle_ld_partners' cores with k_ld_reduce in k_ld_partners' place (include/eagle_hip.h section 1b'''v)
extern "C" int eagle_ld_stats(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], long window, const int32_t* chrom, const int64_t* pos,
                              long max_dist, const int64_t* edges, long nbins, double max_memory_in_Gbytes, uint64_t* U_out, int32_t* cnt_out,
                              uint64_t* bin_sum_out, int64_t* bin_pairs_out) {
    if (!f_name_ascii_Mt || !dims || !U_out || !cnt_out) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_stats: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_stats: dims must be positive");
    if (int rc = ld_stats_check(ctx, "ld_stats", L, window, pos, max_dist, edges, nbins, bin_sum_out, bin_pairs_out)) return rc;
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_stats: no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LdStatsBufs b;
    int rc = ld_stats_begin(ctx, b, L, chrom, pos, edges, nbins);
    if (rc) return rc;
    rc = ld_panel_cores(ctx, f_name_ascii_Mt, n, L, window, max_memory_in_Gbytes, [&](const double* band, long nr, long c_lo, long c_hi, long g0) {
        return ld_stats_core(ctx, b, band, nr, window, c_lo, c_hi, g0, max_dist);
    });
    if (rc) return rc;
    return ld_stats_end(ctx, b, U_out, cnt_out, bin_sum_out, bin_pairs_out);
}

// ---------------------------------------------------------------------------------------------------------------
// Pairwise haplotype EM, D' and the verdict masks (include/eagle_hip.h section 1b''''vii; the kernel in eagle_hapld.hip)
// ---------------------------------------------------------------------------------------------------------------
// eagle_ld_window's walk: a resident image is one launch; a file that is not resident is read in windows of w rows that start every
// w - window rows.  Unlike eagle_ld_window a launch writes and counts only the markers its window OWNS -- all but its last `window`
// markers, which the next window owns, and everything up to the end in the window that holds the last row -- so every output word and
// every counted pair comes from one launch that held all `window` partners of its marker: the words of the resident pass.
extern "C" int eagle_hap_ld(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], long window, double tol, int max_iter, double fg_cut,
                            double dprime_cut, double max_memory_in_Gbytes, uint64_t* recomb_mask_out, uint64_t* strong_mask_out,
                            double* dprime_out, double* r2_out, int64_t* counts_out) {
    if (!f_name_ascii_Mt || !dims || !counts_out) return qc_fail(ctx, EAGLE_ERR_ARG, "hap_ld: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "hap_ld: dims must be positive");
    if (n > 0x3fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "hap_ld: 2^30 individuals or more");
    if (window < 1 || window > 256) return qc_fail(ctx, EAGLE_ERR_ARG, "hap_ld: window must be in [1, 256]");
    if (!(tol > 0.0 && tol < 1.0)) return qc_fail(ctx, EAGLE_ERR_ARG, "hap_ld: tol must be in (0, 1)");
    if (max_iter < 1 || max_iter > 100000) return qc_fail(ctx, EAGLE_ERR_ARG, "hap_ld: max_iter must be in [1, 100000]");
    if (!(fg_cut >= 0.0 && fg_cut <= 1.0)) return qc_fail(ctx, EAGLE_ERR_ARG, "hap_ld: fg_cut must be in [0, 1]");
    if (!(dprime_cut >= 0.0 && dprime_cut <= 1.0)) return qc_fail(ctx, EAGLE_ERR_ARG, "hap_ld: dprime_cut must be in [0, 1]");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "hap_ld: no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long wpr = (window + 63) / 64;
    const size_t mask_bytes = sizeof(uint64_t) * (size_t)L * (size_t)wpr, band_bytes = sizeof(double) * (size_t)L * (size_t)window;
    DevBuf rec, str, dp, r2, tot, counts, sq;
    if (recomb_mask_out) HIPCHK(ctx, rec.alloc(mask_bytes));
    if (strong_mask_out) HIPCHK(ctx, str.alloc(mask_bytes));
    if (dprime_out) HIPCHK(ctx, dp.alloc(band_bytes));
    if (r2_out) HIPCHK(ctx, r2.alloc(band_bytes));
    HIPCHK(ctx, tot.alloc(sizeof(uint64_t) * 4));
    HIPCHK(ctx, hipMemsetAsync(tot.p, 0, sizeof(uint64_t) * 4, ctx->stream));
    ImageLines lines;
    int rc = lines.open(ctx, f_name_ascii_Mt, L, n, max_memory_in_Gbytes);
    if (rc) return rc;
    const long ld = lines.ld();
    const RowWindows ws = lines.resident() ? row_windows_disjoint(L, L) : row_windows_overlapped(L, ld_stream_rows(lines), window);
    HIPCHK(ctx, counts.alloc(sizeof(int32_t) * 3 * (size_t)ws.cap));
    HIPCHK(ctx, sq.alloc(sizeof(int32_t) * 2 * (size_t)ws.cap));
    rc = lines.each(ws, [&](const int8_t* img, long r0, long nr, long c0, long c1) {
        const int trc = ld_tile_sq(ctx, img, nr, n, ld, counts.as<int32_t>(), sq.as<int32_t>());
        if (trc) return trc;
        const long at = c0 - r0;   // the first owned row of the window
        return eagle_dev_hap_ld(ctx, img + at * ld, nr - at, c1 - c0, n, ld, sq.as<int32_t>() + 2 * at, window, tol, max_iter, fg_cut, dprime_cut,
                                rec.p ? rec.as<uint64_t>() + c0 * wpr : nullptr, str.p ? str.as<uint64_t>() + c0 * wpr : nullptr, wpr,
                                dp.p ? dp.as<double>() + c0 * window : nullptr, r2.p ? r2.as<double>() + c0 * window : nullptr,
                                tot.as<uint64_t>(), ctx->stream);
    });
    if (rc) return rc;
    if (recomb_mask_out) HIPCHK(ctx, hipMemcpyAsync(recomb_mask_out, rec.p, mask_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (strong_mask_out) HIPCHK(ctx, hipMemcpyAsync(strong_mask_out, str.p, mask_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (dprime_out) HIPCHK(ctx, hipMemcpyAsync(dprime_out, dp.p, band_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (r2_out) HIPCHK(ctx, hipMemcpyAsync(r2_out, r2.p, band_bytes, hipMemcpyDeviceToHost, ctx->stream));
    uint64_t t4[4];
    HIPCHK(ctx, hipMemcpyAsync(t4, tot.p, sizeof t4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < 4; c++) counts_out[c] = (int64_t)t4[c];
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Pairwise-complete LD from the .bed file (include/eagle_hip.h section 1b'''iv; kernels in eagle_bedld.hip)
// ---------------------------------------------------------------------------------------------------------------
namespace {

// The panel of a call (the included markers of the file, in file order) on the staging ring: the window rule of the header, and the
// staging of one window -- the span of file rows that holds the panel markers [lo, hi) goes through the ring to the device, with the
// offsets of its panel markers' rows when include left rows out.  open() walks the windows once to size the buffers and each() walks them
// again for the call, both through windows(): the two walks are one loop.
struct BedPanel {
    BedRing ring;
    long n = 0, linc = 0;
    long S = 0;      // file rows the staging budget holds
    long wmax = 0;   // panel markers of a window, at most
    long need = 0;   // the markers a window must hold for the call to advance
    std::function<long(long)> next_of;   // the start of the window after one that ends at hi, or linc when that was the last one
    std::vector<long> fidx;   // panel marker -> file row; empty: the identity
    std::vector<long> offs[2];
    DevBuf d_offs[2];
    long file_row(long p) const { return bed_panel_file_row(fidx, p); }
    // f(lo, hi) for every window [lo, hi) of panel markers in turn, until one returns non-zero
    template <class F>
    int windows(F f) const {
        for (long lo = 0; lo < linc;) {
            const long hi = bed_panel_window_end(lo, need, wmax, S, linc, fidx);
            if (int rc = f(lo, hi)) return rc;
            lo = next_of(hi);
        }
        return EAGLE_OK;
    }
    // Opens the file and sizes everything a call needs; band_rows_max caps the window further (the partners call's band), 0 = no cap.
    int open(eagle_ctx* ctx, const char* bed_path, long n_, long L, const uint8_t* include, long linc_, double mem_gb, long band_rows_max, long need_,
             std::function<long(long)> next) {
        n = n_; linc = linc_; need = need_; next_of = std::move(next);
        if (int orc = ring.open(ctx, bed_path, n, L)) return orc;
        S = bed_stage_rows(ring.rb, mem_gb);
        wmax = std::max(1024L, (long)(((size_t)1 << 27) / (size_t)ld()));   // one operand image of the LD calls stays under 128 MiB
        if (band_rows_max > 0) wmax = std::min(wmax, band_rows_max);
        if (include) {
            fidx.reserve((size_t)linc);
            for (long m = 0; m < L; m++) if (include[m]) fidx.push_back(m);
        }
        long span_max = 1, p_max = 1;
        (void)windows([&](long lo, long hi) {
            span_max = std::max(span_max, file_row(hi - 1) - file_row(lo) + 1);
            p_max = std::max(p_max, hi - lo);
            return 0;
        });
        int rc = ring.ensure(span_max);
        if (rc) return rc;
        if (include) for (int b = 0; b < 2; b++) HIPCHK(ctx, d_offs[b].alloc(sizeof(long) * (size_t)p_max));
        wmax = std::min(wmax, p_max);
        return EAGLE_OK;
    }
    long ld() const { return (n + 15) / 16 * 16; }   // leading dimension of the LD calls' operand images
    // *raw: the staged span, whose row 0 is the file row of panel marker lo; *d_off: the rows of the markers [lo, hi) in it (null: the identity)
    int stage(long lo, long hi, const uint8_t** raw, const long** d_off) {
        const long f0 = file_row(lo), P = hi - lo;
        if (int rc = ring.stage(f0, file_row(hi - 1) - f0 + 1, raw)) return rc;
        *d_off = nullptr;
        if (!fidx.empty()) {
            const int b = ring.last();   // the offsets of window k - 2 left with its rows
            offs[b].resize((size_t)P);
            for (long p = 0; p < P; p++) offs[b][(size_t)p] = fidx[(size_t)(lo + p)] - f0;   // in [0, span): fidx increases
            HIPCHK(ring.ctx, hipMemcpyAsync(d_offs[b].p, offs[b].data(), sizeof(long) * (size_t)P, hipMemcpyHostToDevice, ring.ctx->stream));
            *d_off = d_offs[b].as<long>();
        }
        return EAGLE_OK;
    }
    // The call's pass: every window staged and handed to body(lo, hi, raw, d_off), which launches on the ring's stream and calls
    // ring.release() once the staged span has been read.  A failure drains the stream (BedRing's rule).
    template <class Body>
    int each(Body body) {
        const int rc = windows([&](long lo, long hi) {
            const uint8_t* raw;
            const long* d_off;
            const int src = stage(lo, hi, &raw, &d_off);
            return src ? src : body(lo, hi, raw, d_off);
        });
        if (rc) (void)hipStreamSynchronize(ring.ctx->stream);
        return rc;
    }
};

// Linc of an include mask (L when it is NULL)
long bedld_count(const uint8_t* include, long L) {
    if (!include) return L;
    long c = 0;
    for (long m = 0; m < L; m++) c += include[m] != 0;
    return c;
}

// The three marker-major operand images of the two LD calls: k_bed_ld_pack writes those of a window's panel markers from the staged
// span, which is free once the pack has read it.
struct BedLdOperands {
    DevBuf X, C, U;
    int alloc(eagle_ctx* ctx, const BedPanel& pl) {
        for (DevBuf* d : {&X, &C, &U}) HIPCHK(ctx, d->alloc((size_t)pl.wmax * pl.ld()));
        return EAGLE_OK;
    }
    int stage(BedPanel& pl, long lo, long hi, const uint8_t* raw, const long* d_off) {
        const int rc = eagle_dev_bed_ld_pack(pl.ring.ctx, raw, pl.file_row(hi - 1) - pl.file_row(lo) + 1, d_off, hi - lo, pl.n, pl.ld(), X.as<int8_t>(),
                                             C.as<int8_t>(), U.as<int8_t>(), pl.ring.ctx->stream);
        return rc ? rc : pl.ring.release();
    }
};

}  // namespace

// eagle_ld_window's streamed pass over panel markers: a window [lo, hi) writes the mask rows of all its markers, those of its last
// `window` markers without the partners it does not hold, and the next window, which starts on exactly those markers, writes them again
// in full (stream order).
extern "C" int eagle_bed_ld_window(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, long window, double r2,
                                   int min_overlap, double max_memory_in_Gbytes, uint64_t* mask_out, long* npairs_out) {
    if (!bed_path || !dims || !mask_out || !npairs_out) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_window: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_window: dims must be positive");
    if (n > 0x3fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_window: 2^30 individuals or more");
    if (window < 1 || window > 256) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_window: window must be in [1, 256]");
    if (!(r2 >= 0.0 && r2 <= 1.0)) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_window: r2 must be in [0, 1]");
    if (min_overlap < 1) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_window: min_overlap must be at least 1");
    const long linc = bedld_count(include, L);
    if (linc < 1) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_window: include selects no marker");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_window: no context");
    BedPanel pl;
    BedLdOperands op;
    const long need = window + 1;
    auto next_of = [&](long hi) { return hi >= linc ? linc : hi - window; };
    int rc = pl.open(ctx, bed_path, n, L, include, linc, max_memory_in_Gbytes, 0, need, next_of);
    if (!rc) rc = op.alloc(ctx, pl);
    if (rc) return rc;
    const long wpr = (window + 63) / 64;
    const size_t mask_bytes = sizeof(uint64_t) * (size_t)linc * (size_t)wpr;
    DevBuf mask;
    HIPCHK(ctx, mask.alloc(mask_bytes));
    rc = pl.each([&](long lo, long hi, const uint8_t* raw, const long* d_off) {
        const int src = op.stage(pl, lo, hi, raw, d_off);
        return src ? src : eagle_dev_bedld_band(ctx, op.X.as<int8_t>(), op.C.as<int8_t>(), op.U.as<int8_t>(), hi - lo, n, pl.ld(), window, r2,
                                                min_overlap, mask.as<uint64_t>() + lo * wpr, wpr, ctx->stream);
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(mask_out, mask.p, mask_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    long pairs = 0;
    for (size_t x = 0; x < (size_t)linc * (size_t)wpr; x++) pairs += __builtin_popcountll(mask_out[x]);
    *npairs_out = pairs;
    return EAGLE_OK;
}

// eagle_ld_partners' cores over panel markers: the window held for a core [c0, c1) is [lo, hi) = [max(0, c0 - window), min(Linc,
// c1 + window)); the tile kernel writes the r2 band of the markers held and consume(band, markers held, c0 - lo, c1 - lo, lo) works
// on the core alone (k_ld_partners: the partner rows; k_ld_reduce: the sums).  The first core starts at 0 = lo, every later one at
// lo + window; a window holds at least 2 window + 1 markers (or the rest of the panel), so that the next one starts after it did.
namespace {

template <class Consume>
int bedld_panel_cores(eagle_ctx* ctx, const char* bed_path, long n, long L, const uint8_t* include, long linc, long window, int min_overlap,
                      double max_memory_in_Gbytes, Consume consume) {
    BedPanel pl;
    BedLdOperands op;
    const long need = 2 * window + 1;
    auto next_of = [&](long hi) { return hi >= linc ? linc : hi - 2 * window; };              // c1 = hi - window; the next window starts at c1 - window
    const long band_rows = std::max(1024L, (long)(((size_t)256 << 20) / (sizeof(double) * (size_t)window)));   // eagle_ld_partners' cap
    int rc = pl.open(ctx, bed_path, n, L, include, linc, max_memory_in_Gbytes, band_rows, need, next_of);
    if (!rc) rc = op.alloc(ctx, pl);
    if (rc) return rc;
    DevBuf band;
    HIPCHK(ctx, band.alloc(sizeof(double) * (size_t)pl.wmax * (size_t)window));
    rc = pl.each([&](long lo, long hi, const uint8_t* raw, const long* d_off) {
        const long nr = hi - lo, c0 = lo == 0 ? 0 : lo + window, c1 = hi >= linc ? linc : hi - window;
        int brc = op.stage(pl, lo, hi, raw, d_off);
        if (!brc) brc = eagle_dev_bedld_r2band(ctx, op.X.as<int8_t>(), op.C.as<int8_t>(), op.U.as<int8_t>(), nr, n, pl.ld(), window, min_overlap,
                                               band.as<double>(), ctx->stream);
        return brc ? brc : consume(band.as<double>(), nr, c0 - lo, c1 - lo, lo);
    });
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // the operand images and the band leave with this frame
    return EAGLE_OK;
}

}  // namespace

extern "C" int eagle_bed_ld_partners(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, long window, int l,
                                     double min_r2, int min_overlap, const int32_t* chrom, double max_memory_in_Gbytes, int32_t* partners_out,
                                     double* r2_out) {
    if (!bed_path || !dims || !partners_out) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_partners: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_partners: dims must be positive");
    if (n > 0x3fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_partners: 2^30 individuals or more");
    if (window < 1 || window > 256) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_partners: window must be in [1, 256]");
    if (l < 1 || l > EAGLE_LDKNN_MAX_PARTNERS) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_partners: l outside [1, 32]");
    if (!(min_r2 >= 0.0 && min_r2 <= 1.0)) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_partners: min_r2 must be in [0, 1]");
    if (min_overlap < 1) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_partners: min_overlap must be at least 1");
    const long linc = bedld_count(include, L);
    if (linc < 1) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_partners: include selects no marker");
    if (linc > 0x7fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_partners: 2^31 markers or more");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_partners: no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)linc * (size_t)l;
    DevBuf part, r2, d_chrom;
    HIPCHK(ctx, part.alloc(sizeof(int32_t) * cells));
    HIPCHK(ctx, r2.alloc(sizeof(double) * cells));
    if (chrom) {
        HIPCHK(ctx, d_chrom.alloc(sizeof(int32_t) * (size_t)linc));
        HIPCHK(ctx, hipMemcpyAsync(d_chrom.p, chrom, sizeof(int32_t) * (size_t)linc, hipMemcpyHostToDevice, ctx->stream));
    }
    int rc = bedld_panel_cores(ctx, bed_path, n, L, include, linc, window, min_overlap, max_memory_in_Gbytes,
                               [&](const double* band, long nr, long c_lo, long c_hi, long g0) {
        return eagle_dev_ld_partners(ctx, band, nr, window, c_lo, c_hi, g0, chrom ? d_chrom.as<int32_t>() : nullptr, min_r2, l, part.as<int32_t>(),
                                     r2.as<double>(), ctx->stream);
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(partners_out, part.p, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, ctx->stream));
    if (r2_out) HIPCHK(ctx, hipMemcpyAsync(r2_out, r2.p, sizeof(double) * cells, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

// eagle_bed_ld_partners' cores with k_ld_reduce in k_ld_partners' place (include/eagle_hip.h section 1b'''v); chrom / pos by panel marker
extern "C" int eagle_bed_ld_stats(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, long window, int min_overlap,
                                  const int32_t* chrom, const int64_t* pos, long max_dist, const int64_t* edges, long nbins,
                                  double max_memory_in_Gbytes, uint64_t* U_out, int32_t* cnt_out, uint64_t* bin_sum_out, int64_t* bin_pairs_out) {
    if (!bed_path || !dims || !U_out || !cnt_out) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_stats: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_stats: dims must be positive");
    if (n > 0x3fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_stats: 2^30 individuals or more");
    if (min_overlap < 1) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_stats: min_overlap must be at least 1");
    const long linc = bedld_count(include, L);
    if (linc < 1) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_stats: include selects no marker");
    if (int rc = ld_stats_check(ctx, "bed_ld_stats", linc, window, pos, max_dist, edges, nbins, bin_sum_out, bin_pairs_out)) return rc;
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ld_stats: no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LdStatsBufs b;
    int rc = ld_stats_begin(ctx, b, linc, chrom, pos, edges, nbins);
    if (rc) return rc;
    rc = bedld_panel_cores(ctx, bed_path, n, L, include, linc, window, min_overlap, max_memory_in_Gbytes,
                           [&](const double* band, long nr, long c_lo, long c_hi, long g0) {
        return ld_stats_core(ctx, b, band, nr, window, c_lo, c_hi, g0, max_dist);
    });
    if (rc) return rc;
    return ld_stats_end(ctx, b, U_out, cnt_out, bin_sum_out, bin_pairs_out);
}

// ---------------------------------------------------------------------------------------------------------------
// Runs of homozygosity (include/eagle_hip.h section 1b'''vi; kernels in eagle_roh.hip)
// ---------------------------------------------------------------------------------------------------------------
static_assert(ROH_MAX_WINDOW == EAGLE_ROH_MAX_WINDOW, "eagle_host.h restates the public limit");
namespace {

// What both entry points hold on the device: the three bit planes of the panel, the block table, pos, and the segment passes' arrays.
struct RohBufs {
    DevBuf planes, blk, pos, cnt, offs, ind, seg;
    std::vector<int32_t> h_blk;
    long lp = 0, n = 0;
    long nb() const { return (long)h_blk.size() - 1; }
};

// The argument rule of eagle_host.h, the block table and the check of pos: everything that is decided before the context is used.
int roh_check(eagle_ctx* ctx, const char* who, long lp, const int32_t* chrom, const int64_t* pos, const eagle_roh_params* prm, const void* seg_out,
              long seg_cap, std::vector<int32_t>& blk) {
    const int64_t f[9] = {prm->w, prm->win_het, prm->win_miss, prm->thr16, prm->min_snp, prm->min_len, prm->max_gap, prm->max_density, prm->max_het};
    char msg[160];
    if (const char* bad = roh_arg_error(f, lp, seg_cap, seg_out != nullptr)) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    }
    roh_block_table(chrom, lp, blk);
    const long m = roh_pos_check(pos, blk);
    if (m >= 0) {
        snprintf(msg, sizeof msg, "%s: pos decreases inside a block (panel marker %ld)", who, m);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    }
    return EAGLE_OK;
}

// The planes against the memory budget (rule 8), then the allocations and uploads; no kernel has run when this fails.
int roh_begin(eagle_ctx* ctx, const char* who, RohBufs& b, long n, long lp, const int64_t* pos) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    b.n = n;
    b.lp = lp;
    const size_t nw = (size_t)((n + 63) / 64), plane_bytes = sizeof(uint64_t) * 3 * (size_t)lp * nw;
    size_t budget = eagle_resident_budget();
    if (budget == (size_t)-1) {
        size_t freeb = 0, totalb = 0;
        HIPCHK(ctx, hipMemGetInfo(&freeb, &totalb));
        budget = freeb > ((size_t)1 << 30) ? freeb - ((size_t)1 << 30) : 0;
    }
    if (plane_bytes > budget) return failf(ctx, EAGLE_ERR_NOMEM, "%s: the three bit planes (%zu bytes) do not fit the memory budget", who, plane_bytes);
    const size_t cells = (size_t)n * (size_t)b.nb();
    HIPCHK(ctx, b.planes.alloc(plane_bytes));
    HIPCHK(ctx, b.blk.alloc(sizeof(int32_t) * b.h_blk.size()));
    HIPCHK(ctx, b.cnt.alloc(sizeof(int32_t) * cells));
    HIPCHK(ctx, b.offs.alloc(sizeof(int64_t) * cells));
    HIPCHK(ctx, b.ind.alloc(sizeof(int64_t) * 4 * (size_t)n));
    HIPCHK(ctx, hipMemcpyAsync(b.blk.p, b.h_blk.data(), sizeof(int32_t) * b.h_blk.size(), hipMemcpyHostToDevice, ctx->stream));
    if (pos) {
        HIPCHK(ctx, b.pos.alloc(sizeof(int64_t) * (size_t)lp));
        HIPCHK(ctx, hipMemcpyAsync(b.pos.p, pos, sizeof(int64_t) * (size_t)lp, hipMemcpyHostToDevice, ctx->stream));
    }
    return EAGLE_OK;
}

// The count pass, the exclusive scan of the counts by (individual, block) on the host, and the fill pass when the rows fit seg_cap.
int roh_end(eagle_ctx* ctx, RohBufs& b, const eagle_roh_params* prm, int64_t* ind_out, int32_t* seg_out, long seg_cap, long* nseg_out) {
    const size_t cells = (size_t)b.n * (size_t)b.nb();
    const int64_t* d_pos = b.pos.p ? b.pos.as<int64_t>() : nullptr;
    HIPCHK(ctx, hipMemsetAsync(b.ind.p, 0, sizeof(int64_t) * 4 * (size_t)b.n, ctx->stream));
    int rc = eagle_dev_roh_segments(ctx, b.planes.as<uint64_t>(), b.lp, b.n, b.blk.as<int32_t>(), b.nb(), d_pos, prm, 0, b.cnt.as<int32_t>(),
                                    b.ind.as<int64_t>(), nullptr, nullptr, ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    std::vector<int32_t> h_cnt(cells);
    std::vector<int64_t> h_offs(cells);
    HIPCHK(ctx, hipMemcpyAsync(h_cnt.data(), b.cnt.p, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ind_out, b.ind.p, sizeof(int64_t) * 4 * (size_t)b.n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t total = roh_offsets(h_cnt.data(), cells, h_offs.data());
    *nseg_out = (long)total;
    if (total == 0 || total > seg_cap) return EAGLE_OK;
    HIPCHK(ctx, b.seg.alloc(sizeof(int32_t) * 6 * (size_t)total));
    HIPCHK(ctx, hipMemcpyAsync(b.offs.p, h_offs.data(), sizeof(int64_t) * cells, hipMemcpyHostToDevice, ctx->stream));
    rc = eagle_dev_roh_segments(ctx, b.planes.as<uint64_t>(), b.lp, b.n, b.blk.as<int32_t>(), b.nb(), d_pos, prm, 1, nullptr, nullptr,
                                b.offs.as<int64_t>(), b.seg.as<int32_t>(), ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    HIPCHK(ctx, hipMemcpyAsync(seg_out, b.seg.p, sizeof(int32_t) * 6 * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // h_offs leaves with this frame
    return EAGLE_OK;
}

}  // namespace

// The flags pass over a resident image is one launch.  A file that is not resident is read in row windows of the streamed size, each a
// CORE of markers held with w - 1 rows of overlap on both sides (ld_panel_cores' scheme): the launch writes the plane rows of the core
// alone, from rows that hold every window of its markers, so every plane word is written once.
extern "C" int eagle_roh(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const int32_t* chrom, const int64_t* pos,
                         const eagle_roh_params* params, double max_memory_in_Gbytes, int64_t* ind_out, int32_t* seg_out, long seg_cap,
                         long* nseg_out) {
    if (!f_name_ascii_Mt || !dims || !params || !ind_out || !nseg_out) return qc_fail(ctx, EAGLE_ERR_ARG, "roh: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "roh: dims must be positive");
    RohBufs b;
    if (int rc = roh_check(ctx, "roh", L, chrom, pos, params, seg_out, seg_cap, b.h_blk)) return rc;
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "roh: no context");
    int rc = roh_begin(ctx, "roh", b, n, L, pos);
    if (rc) return rc;
    ImageLines lines;
    rc = lines.open(ctx, f_name_ascii_Mt, L, n, max_memory_in_Gbytes);
    if (rc) return rc;
    const long held_max = lines.resident() ? L : std::min(L, std::max(256L, lines.stream_rows()));
    rc = lines.each(row_windows_cores(L, held_max, params->w - 1), [&](const int8_t* img, long lo, long, long c0, long c1) {
        return eagle_dev_roh_flags_i8(ctx, img, lines.ld(), n, lo, c0, c1, b.blk.as<int32_t>(), b.nb(), params, b.planes.as<uint64_t>(), L, ctx->stream);
    });
    if (rc) return rc;
    return roh_end(ctx, b, params, ind_out, seg_out, seg_cap, nseg_out);
}

// The .bed rows go through the pinned ring in eagle_bed_ld_partners' windows of panel markers, with w - 1 markers in the place of its
// `window`: the window held for the core [c0, c1) is [lo, hi) = [max(0, c0 - (w - 1)), min(Linc, c1 + w - 1)).
extern "C" int eagle_bed_roh(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, const int32_t* chrom,
                             const int64_t* pos, const eagle_roh_params* params, double max_memory_in_Gbytes, int64_t* ind_out, int32_t* seg_out,
                             long seg_cap, long* nseg_out) {
    if (!bed_path || !dims || !params || !ind_out || !nseg_out) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_roh: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_roh: dims must be positive");
    if (n > 0x3fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_roh: 2^30 individuals or more");
    const long linc = bedld_count(include, L);
    if (linc < 1) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_roh: include selects no marker");
    RohBufs b;
    if (int rc = roh_check(ctx, "bed_roh", linc, chrom, pos, params, seg_out, seg_cap, b.h_blk)) return rc;
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_roh: no context");
    int rc = roh_begin(ctx, "bed_roh", b, n, linc, pos);
    if (rc) return rc;
    BedPanel pl;
    const long h = params->w - 1, need = 2 * h + 1;
    auto next_of = [&](long hi) { return hi >= linc ? linc : hi - 2 * h; };
    rc = pl.open(ctx, bed_path, n, L, include, linc, max_memory_in_Gbytes, 0, need, next_of);
    if (rc) return rc;
    rc = pl.each([&](long lo, long hi, const uint8_t* raw, const long* d_off) {
        const long c0 = lo == 0 ? 0 : lo + h, c1 = hi >= linc ? linc : hi - h;
        const int brc = eagle_dev_roh_flags_bed(ctx, raw, d_off, n, lo, c0, c1, b.blk.as<int32_t>(), b.nb(), params, b.planes.as<uint64_t>(), linc,
                                                ctx->stream);
        return brc ? brc : pl.ring.release();
    });
    if (rc) return rc;
    return roh_end(ctx, b, params, ind_out, seg_out, seg_cap, nseg_out);
}

// ---------------------------------------------------------------------------------------------------------------
// Pairwise IBD-type segments (include/eagle_hip.h section 1b'''vii; kernels in eagle_ibd.hip)
// ---------------------------------------------------------------------------------------------------------------
static_assert(IBD_MAX_PAIRS == EAGLE_IBD_MAX_PAIRS, "eagle_host.h restates the public limit");
namespace {

// The bit planes of a call (eagle_ibd.hip): A and B from the ingested panel, A, B and C from the .bed file, resident for the whole call.
// build() is the one place that makes them: the budget test of IBD rule 9 over the planes and `extra` further bytes the caller will
// allocate (named by extra_what in the message) -- EAGLE_ERR_NOMEM before any kernel runs --, the allocation, and the fill: from
// M.ascii (bed_path null) the resident image in one launch, else bands of whole lines of the streamed size from the sidecar, the text
// or a VIEW alias's source; from the .bed file the ring's windows of panel markers, each but the last cut back to a multiple of 64
// markers (it holds at least 64) so that a window writes whole plane words.  Every plane word is written once.
struct GenoPlanes {
    DevBuf planes;
    long n = 0, lp = 0;
    int nplanes = 2;
    size_t bytes() const { return sizeof(uint64_t) * (size_t)nplanes * (size_t)((lp + 63) / 64) * (size_t)((n + 63) / 64 * 64); }
    uint64_t* p() { return planes.as<uint64_t>(); }
    // The memory budget of rule 9: the resident budget where one is set, else the device's free memory less 1 GiB.
    static int budget_bytes(eagle_ctx* ctx, size_t* out) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        size_t budget = eagle_resident_budget();
        if (budget == (size_t)-1) {
            size_t freeb = 0, totalb = 0;
            HIPCHK(ctx, hipMemGetInfo(&freeb, &totalb));
            budget = freeb > ((size_t)1 << 30) ? freeb - ((size_t)1 << 30) : 0;
        }
        *out = budget;
        return EAGLE_OK;
    }
    // path: M.ascii of dims (n, L), or with is_bed the .bed file of dims (n, L) whose panel is the linc markers of include
    int build(eagle_ctx* ctx, const char* who, bool is_bed, const char* path, long n_, long L, const uint8_t* include, long linc, double mem_gb,
              size_t extra, const char* extra_what) {
        n = n_;
        lp = is_bed ? linc : L;
        nplanes = is_bed ? 3 : 2;
        const size_t plane_bytes = bytes();
        size_t budget = 0;
        if (int rc = budget_bytes(ctx, &budget)) return rc;
        if (plane_bytes > budget || extra > budget - plane_bytes)
            return failf(ctx, EAGLE_ERR_NOMEM, "%s: the bit planes (%zu bytes) and %s (%zu bytes) do not fit the memory budget", who, plane_bytes,
                         extra_what, extra);
        HIPCHK(ctx, planes.alloc(plane_bytes));
        return is_bed ? fill_bed(ctx, path, L, include, mem_gb) : fill_image(ctx, path, L, mem_gb);
    }

  private:
    int fill_image(eagle_ctx* ctx, const char* f_name_ascii_M, long L, double mem_gb) {
        ImageLines lines;
        if (int rc = lines.open(ctx, f_name_ascii_M, n, L, mem_gb)) return rc;
        return lines.each(lines.disjoint(std::min(n, lines.stream_rows())), [&](const int8_t* img, long r0, long nr, long, long) {
            return eagle_dev_ibd_planes_i8(ctx, img, lines.ld(), r0, nr, n, L, p(), ctx->stream);
        });
    }
    int fill_bed(eagle_ctx* ctx, const char* bed_path, long L, const uint8_t* include, double mem_gb) {
        BedPanel pl;
        const long linc = lp, need = 64;
        auto next_of = [&](long hi) { return hi >= linc ? linc : hi / 64 * 64; };
        int rc = pl.open(ctx, bed_path, n, L, include, linc, mem_gb, 0, need, next_of);
        if (rc) return rc;
        rc = pl.each([&](long lo, long hi, const uint8_t* raw, const long* d_off) {
            const int brc = eagle_dev_ibd_planes_bed(ctx, raw, d_off, n, lo, lo / 64, (next_of(hi) + 63) / 64, linc, p(), ctx->stream);
            return brc ? brc : pl.ring.release();
        });
        if (rc) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // the ring and the offsets leave with this frame
        return EAGLE_OK;
    }
};

// What both entry points hold on the device beside the planes: the cut plane, the block table, pos, the pair list and the walk's arrays.
struct IbdBufs {
    GenoPlanes g;
    DevBuf cut, blk, pos, pairs, tot, offs, seg;
    std::vector<int32_t> h_blk;
    long lp = 0, n = 0, P = 0;
    long nb() const { return (long)h_blk.size() - 1; }
};

// The argument rule of eagle_host.h, the pair list, the block table and the check of pos: everything that is decided before the
// context is used.
int ibd_check(eagle_ctx* ctx, const char* who, long n, long lp, const int32_t* pairs, long npairs, const int32_t* chrom, const int64_t* pos,
              const eagle_ibd_params* prm, const void* seg_out, long seg_cap, std::vector<int32_t>& blk) {
    const int64_t f[5] = {prm->mode, prm->min_snp, prm->min_len, prm->max_gap, prm->merge_min};
    char msg[160];
    if (const char* bad = ibd_arg_error(f, n, lp, pairs != nullptr, npairs, seg_cap, seg_out != nullptr)) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    }
    if (pairs) {
        const long k = ibd_pairs_check(pairs, npairs, n);
        if (k >= 0) {
            snprintf(msg, sizeof msg, "%s: pair %ld is not 0 <= i < j < n", who, k);
            return qc_fail(ctx, EAGLE_ERR_ARG, msg);
        }
    }
    roh_block_table(chrom, lp, blk);
    const long m = roh_pos_check(pos, blk);
    if (m >= 0) {
        snprintf(msg, sizeof msg, "%s: pos decreases inside a block (panel marker %ld)", who, m);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    }
    return EAGLE_OK;
}

// The bytes of the per-pair arrays of rule 9.
size_t ibd_pair_bytes(long n, const int32_t* pairs, long npairs) { return (size_t)40 * (size_t)ibd_pair_count(n, pairs != nullptr, npairs); }

// After the planes (GenoPlanes::build, which holds the budget test of rule 9): the allocations and uploads of everything else.
int ibd_begin(eagle_ctx* ctx, IbdBufs& b, long n, long lp, const int32_t* pairs, long npairs, const int32_t* chrom, const int64_t* pos,
              const eagle_ibd_params* prm) {
    b.n = n;
    b.lp = lp;
    b.P = ibd_pair_count(n, pairs != nullptr, npairs);
    const size_t nwords = (size_t)((lp + 63) / 64);
    std::vector<uint64_t> h_cut;
    ibd_cut_plane(chrom, pos, prm->max_gap, lp, h_cut);
    HIPCHK(ctx, b.cut.alloc(sizeof(uint64_t) * nwords));
    HIPCHK(ctx, b.blk.alloc(sizeof(int32_t) * b.h_blk.size()));
    HIPCHK(ctx, b.tot.alloc(sizeof(int64_t) * 4 * (size_t)b.P));
    HIPCHK(ctx, b.offs.alloc(sizeof(int64_t) * (size_t)b.P));
    HIPCHK(ctx, hipMemcpyAsync(b.cut.p, h_cut.data(), sizeof(uint64_t) * nwords, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(b.blk.p, b.h_blk.data(), sizeof(int32_t) * b.h_blk.size(), hipMemcpyHostToDevice, ctx->stream));
    if (pos) {
        HIPCHK(ctx, b.pos.alloc(sizeof(int64_t) * (size_t)lp));
        HIPCHK(ctx, hipMemcpyAsync(b.pos.p, pos, sizeof(int64_t) * (size_t)lp, hipMemcpyHostToDevice, ctx->stream));
    }
    if (pairs) {
        HIPCHK(ctx, b.pairs.alloc(sizeof(int32_t) * 2 * (size_t)b.P));
        HIPCHK(ctx, hipMemcpyAsync(b.pairs.p, pairs, sizeof(int32_t) * 2 * (size_t)b.P, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // h_cut leaves with this frame
    return EAGLE_OK;
}

// The count pass, the exclusive scan of the per-pair counts on the host, and the fill pass when the rows fit seg_cap.
int ibd_end(eagle_ctx* ctx, IbdBufs& b, const eagle_ibd_params* prm, int64_t* pair_out, int32_t* seg_out, long seg_cap, long* nseg_out) {
    const int64_t* d_pos = b.pos.p ? b.pos.as<int64_t>() : nullptr;
    const int32_t* d_pairs = b.pairs.p ? b.pairs.as<int32_t>() : nullptr;
    int rc = eagle_dev_ibd_walk(ctx, b.g.p(), b.g.nplanes, b.cut.as<uint64_t>(), b.n, b.lp, d_pairs, b.P, b.blk.as<int32_t>(), b.nb(),
                                d_pos, prm, 0, b.tot.as<int64_t>(), nullptr, nullptr, ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    HIPCHK(ctx, hipMemcpyAsync(pair_out, b.tot.p, sizeof(int64_t) * 4 * (size_t)b.P, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int64_t> h_offs((size_t)b.P);
    const int64_t total = ibd_offsets(pair_out, (size_t)b.P, h_offs.data());
    *nseg_out = (long)total;
    if (total == 0 || total > seg_cap) return EAGLE_OK;
    HIPCHK(ctx, b.seg.alloc(sizeof(int32_t) * 6 * (size_t)total));
    HIPCHK(ctx, hipMemcpyAsync(b.offs.p, h_offs.data(), sizeof(int64_t) * (size_t)b.P, hipMemcpyHostToDevice, ctx->stream));
    rc = eagle_dev_ibd_walk(ctx, b.g.p(), b.g.nplanes, b.cut.as<uint64_t>(), b.n, b.lp, d_pairs, b.P, b.blk.as<int32_t>(), b.nb(), d_pos,
                            prm, 1, nullptr, b.offs.as<int64_t>(), b.seg.as<int32_t>(), ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    HIPCHK(ctx, hipMemcpyAsync(seg_out, b.seg.p, sizeof(int32_t) * 6 * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // h_offs leaves with this frame
    return EAGLE_OK;
}

}  // namespace

// A line of M.ascii is an individual; the planes are GenoPlanes::build's.
extern "C" int eagle_ibd(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], const int32_t* pairs, long npairs, const int32_t* chrom,
                         const int64_t* pos, const eagle_ibd_params* params, double max_memory_in_Gbytes, int64_t* pair_out, int32_t* seg_out,
                         long seg_cap, long* nseg_out) {
    if (!f_name_ascii_M || !dims || !params || !pair_out || !nseg_out) return qc_fail(ctx, EAGLE_ERR_ARG, "ibd: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "ibd: dims must be positive");
    IbdBufs b;
    if (int rc = ibd_check(ctx, "ibd", n, L, pairs, npairs, chrom, pos, params, seg_out, seg_cap, b.h_blk)) return rc;
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "ibd: no context");
    int rc = b.g.build(ctx, "ibd", false, f_name_ascii_M, n, L, nullptr, L, max_memory_in_Gbytes, ibd_pair_bytes(n, pairs, npairs),
                       "the per-pair arrays");
    if (!rc) rc = ibd_begin(ctx, b, n, L, pairs, npairs, chrom, pos, params);
    if (rc) return rc;
    return ibd_end(ctx, b, params, pair_out, seg_out, seg_cap, nseg_out);
}

// The same from the .bed file (GenoPlanes::build with the ring's windows).
extern "C" int eagle_bed_ibd(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, const int32_t* pairs, long npairs,
                             const int32_t* chrom, const int64_t* pos, const eagle_ibd_params* params, double max_memory_in_Gbytes,
                             int64_t* pair_out, int32_t* seg_out, long seg_cap, long* nseg_out) {
    if (!bed_path || !dims || !params || !pair_out || !nseg_out) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ibd: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ibd: dims must be positive");
    if (n > 0x3fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ibd: 2^30 individuals or more");
    const long linc = bedld_count(include, L);
    if (linc < 1) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ibd: include selects no marker");
    IbdBufs b;
    if (int rc = ibd_check(ctx, "bed_ibd", n, linc, pairs, npairs, chrom, pos, params, seg_out, seg_cap, b.h_blk)) return rc;
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_ibd: no context");
    int rc = b.g.build(ctx, "bed_ibd", true, bed_path, n, L, include, linc, max_memory_in_Gbytes, ibd_pair_bytes(n, pairs, npairs),
                       "the per-pair arrays");
    if (!rc) rc = ibd_begin(ctx, b, n, linc, pairs, npairs, chrom, pos, params);
    if (rc) return rc;
    return ibd_end(ctx, b, params, pair_out, seg_out, seg_cap, nseg_out);
}

// ---------------------------------------------------------------------------------------------------------------
// Mendel errors and parentage assignment (include/eagle_hip.h section 1b'''viii; kernels in eagle_mendel.hip)
// ---------------------------------------------------------------------------------------------------------------
static_assert(MENDEL_MAX_TRIOS == EAGLE_MENDEL_MAX_TRIOS, "eagle_host.h restates the public limit");
namespace {

// Everything of the trio rule that is decided before the context is used.
int mendel_check(eagle_ctx* ctx, const char* who, long n, long lp, const int32_t* trios, long ntrios) {
    char msg[160];
    if (const char* bad = mendel_arg_error(lp, ntrios)) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    }
    const long k = mendel_trios_check(trios, ntrios, n);
    if (k >= 0) {
        snprintf(msg, sizeof msg, "%s: trio %ld is not (c, f, m) with 0 <= c < n, -1 <= f, m < n, c != f, c != m, f != m", who, k);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    }
    return EAGLE_OK;
}

// The trio list, the six counts a trio and the marker counts.
size_t mendel_extra_bytes(long lp, long ntrios, bool marker) { return (size_t)36 * (size_t)ntrios + (marker ? sizeof(int32_t) * (size_t)lp : 0); }

// The trio pass over the planes of g and the download of its tables.
int mendel_run(eagle_ctx* ctx, GenoPlanes& g, const int32_t* trios, long ntrios, int32_t* trio_out, int32_t* marker_out) {
    DevBuf d_trios, d_out, d_marker;
    const size_t T = (size_t)ntrios;
    HIPCHK(ctx, d_trios.alloc(sizeof(int32_t) * 3 * T));
    HIPCHK(ctx, d_out.alloc(sizeof(int32_t) * 6 * T));
    HIPCHK(ctx, hipMemcpyAsync(d_trios.p, trios, sizeof(int32_t) * 3 * T, hipMemcpyHostToDevice, ctx->stream));
    if (marker_out) {
        HIPCHK(ctx, d_marker.alloc(sizeof(int32_t) * (size_t)g.lp));
        HIPCHK(ctx, hipMemsetAsync(d_marker.p, 0, sizeof(int32_t) * (size_t)g.lp, ctx->stream));
    }
    int rc = eagle_dev_mendel_trios(ctx, g.p(), g.nplanes, g.n, g.lp, d_trios.as<int32_t>(), ntrios, d_out.as<int32_t>(),
                                    marker_out ? d_marker.as<int32_t>() : nullptr, ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    HIPCHK(ctx, hipMemcpyAsync(trio_out, d_out.p, sizeof(int32_t) * 6 * T, hipMemcpyDeviceToHost, ctx->stream));
    if (marker_out) HIPCHK(ctx, hipMemcpyAsync(marker_out, d_marker.p, sizeof(int32_t) * (size_t)g.lp, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

// Everything of rules 6 and 7 that is decided before the context is used.
int parentage_check(eagle_ctx* ctx, const char* who, long n, long lp, const int32_t* offspring, long n_o, const int32_t* sires, long n_s,
                    const int32_t* dams, long n_d, long min_overlap, long allow_self) {
    char msg[160];
    if (const char* bad = parentage_arg_error(lp, n_o, n_s, n_d, min_overlap, allow_self)) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    }
    if ((n_s > 0 && !sires) || (n_d > 0 && !dams)) {
        snprintf(msg, sizeof msg, "%s: NULL argument (a candidate list with a positive length)", who);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    }
    const struct { const char* name; const int32_t* list; long cnt; } lists[3] = {{"offspring", offspring, n_o}, {"sires", sires, n_s}, {"dams", dams, n_d}};
    for (const auto& l : lists) {
        bool dup = false;
        const long k = parentage_list_check(l.list, l.cnt, n, &dup);
        if (k >= 0) {
            snprintf(msg, sizeof msg, dup ? "%s: %s entry %ld is a duplicate" : "%s: %s entry %ld is outside [0, n)", who, l.name, k);
            return qc_fail(ctx, EAGLE_ERR_ARG, msg);
        }
    }
    return EAGLE_OK;
}

long par_pad(long cnt) { return ((cnt > 0 ? cnt : 1) + 63) / 64 * 64; }
// Offspring of one launch: the partials of a chunk stay under 256 MiB (12 bytes an entry, two entries a part), and gridDim.y under 65536.
long parentage_chunk(long n_o, long n_s, long n_d) {
    const long per = 24 * eagle_parentage_parts(n_s, n_d);
    return std::max(1L, std::min(std::min(n_o, 65535L), ((long)1 << 28) / per));
}
// The gathered sub-planes of the three lists, the partials of a chunk, the rows and the lists.
size_t parentage_extra_bytes(int nplanes, long lp, long n_o, long n_s, long n_d) {
    const size_t nwords = (size_t)((lp + 63) / 64);
    return sizeof(uint64_t) * (size_t)nplanes * nwords * (size_t)(par_pad(n_o) + par_pad(n_s) + par_pad(n_d)) +
           (size_t)24 * (size_t)eagle_parentage_parts(n_s, n_d) * (size_t)parentage_chunk(n_o, n_s, n_d) + (size_t)36 * (size_t)n_o +
           sizeof(int32_t) * (size_t)(n_s + n_d + 2);
}

// The gathers of the three lists, the chunks of offspring and the download of the rows.
int parentage_run(eagle_ctx* ctx, GenoPlanes& g, const int32_t* offspring, long n_o, const int32_t* sires, long n_s, const int32_t* dams, long n_d,
                  int min_overlap, int allow_self, int32_t* best_out) {
    const size_t nwords = (size_t)((g.lp + 63) / 64);
    const int32_t unknown = -1;
    struct Side { const int32_t* list; long cnt; DevBuf idx, sub; } side[3] = {{offspring, n_o, {}, {}}, {sires, n_s, {}, {}}, {dams, n_d, {}, {}}};
    for (Side& sd : side) {
        const long cnt = sd.cnt > 0 ? sd.cnt : 1;            // an empty list: the one index -1
        HIPCHK(ctx, sd.idx.alloc(sizeof(int32_t) * (size_t)cnt));
        HIPCHK(ctx, sd.sub.alloc(sizeof(uint64_t) * (size_t)g.nplanes * nwords * (size_t)par_pad(cnt)));
        HIPCHK(ctx, hipMemcpyAsync(sd.idx.p, sd.cnt > 0 ? sd.list : &unknown, sizeof(int32_t) * (size_t)cnt, hipMemcpyHostToDevice, ctx->stream));
        int rc = eagle_dev_plane_gather(ctx, g.p(), g.nplanes, g.n, g.lp, sd.idx.as<int32_t>(), cnt, sd.sub.as<uint64_t>(), ctx->stream);
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    }
    const long chunk = parentage_chunk(n_o, n_s, n_d), nparts = eagle_parentage_parts(n_s, n_d);
    DevBuf part_k, part_n, best;
    HIPCHK(ctx, part_k.alloc(sizeof(uint64_t) * 2 * (size_t)nparts * (size_t)chunk));
    HIPCHK(ctx, part_n.alloc(sizeof(int32_t) * 2 * (size_t)nparts * (size_t)chunk));
    HIPCHK(ctx, best.alloc(sizeof(int32_t) * 8 * (size_t)n_o));
    for (long o0 = 0; o0 < n_o; o0 += chunk) {               // stream order: a chunk's finish has read the partials before the next one writes them
        int rc = eagle_dev_parentage(ctx, side[0].sub.as<uint64_t>(), n_o, side[1].sub.as<uint64_t>(), n_s, side[2].sub.as<uint64_t>(), n_d, g.nplanes,
                                     g.lp, side[0].idx.as<int32_t>(), side[1].idx.as<int32_t>(), side[2].idx.as<int32_t>(), o0, std::min(chunk, n_o - o0),
                                     min_overlap, allow_self, part_k.as<uint64_t>(), part_n.as<int32_t>(), best.as<int32_t>(), ctx->stream);
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    }
    HIPCHK(ctx, hipMemcpyAsync(best_out, best.p, sizeof(int32_t) * 8 * (size_t)n_o, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // `unknown` and the buffers leave with this frame
    return EAGLE_OK;
}

}  // namespace

extern "C" int eagle_mendel(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], const int32_t* trios, long ntrios,
                            double max_memory_in_Gbytes, int32_t* trio_out, int32_t* marker_out) {
    if (!f_name_ascii_M || !dims || !trios || !trio_out) return qc_fail(ctx, EAGLE_ERR_ARG, "mendel: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "mendel: dims must be positive");
    if (int rc = mendel_check(ctx, "mendel", n, L, trios, ntrios)) return rc;
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "mendel: no context");
    GenoPlanes g;
    int rc = g.build(ctx, "mendel", false, f_name_ascii_M, n, L, nullptr, L, max_memory_in_Gbytes, mendel_extra_bytes(L, ntrios, marker_out != nullptr),
                     "the per-trio and per-marker arrays");
    if (rc) return rc;
    return mendel_run(ctx, g, trios, ntrios, trio_out, marker_out);
}

extern "C" int eagle_bed_mendel(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, const int32_t* trios, long ntrios,
                                double max_memory_in_Gbytes, int32_t* trio_out, int32_t* marker_out) {
    if (!bed_path || !dims || !trios || !trio_out) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_mendel: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_mendel: dims must be positive");
    if (n > 0x3fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_mendel: 2^30 individuals or more");
    const long linc = bedld_count(include, L);
    if (linc < 1) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_mendel: include selects no marker");
    if (int rc = mendel_check(ctx, "bed_mendel", n, linc, trios, ntrios)) return rc;
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_mendel: no context");
    GenoPlanes g;
    int rc = g.build(ctx, "bed_mendel", true, bed_path, n, L, include, linc, max_memory_in_Gbytes,
                     mendel_extra_bytes(linc, ntrios, marker_out != nullptr), "the per-trio and per-marker arrays");
    if (rc) return rc;
    return mendel_run(ctx, g, trios, ntrios, trio_out, marker_out);
}

extern "C" int eagle_parentage(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], const int32_t* offspring, long n_o, const int32_t* sires,
                               long n_s, const int32_t* dams, long n_d, long min_overlap, int allow_self, double max_memory_in_Gbytes,
                               int32_t* best_out) {
    if (!f_name_ascii_M || !dims || !offspring || !best_out) return qc_fail(ctx, EAGLE_ERR_ARG, "parentage: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "parentage: dims must be positive");
    if (int rc = parentage_check(ctx, "parentage", n, L, offspring, n_o, sires, n_s, dams, n_d, min_overlap, allow_self)) return rc;
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "parentage: no context");
    GenoPlanes g;
    int rc = g.build(ctx, "parentage", false, f_name_ascii_M, n, L, nullptr, L, max_memory_in_Gbytes, parentage_extra_bytes(2, L, n_o, n_s, n_d),
                     "the candidates' planes and the partial minima");
    if (rc) return rc;
    return parentage_run(ctx, g, offspring, n_o, sires, n_s, dams, n_d, (int)min_overlap, allow_self, best_out);
}

extern "C" int eagle_bed_parentage(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, const int32_t* offspring, long n_o,
                                   const int32_t* sires, long n_s, const int32_t* dams, long n_d, long min_overlap, int allow_self,
                                   double max_memory_in_Gbytes, int32_t* best_out) {
    if (!bed_path || !dims || !offspring || !best_out) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_parentage: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_parentage: dims must be positive");
    if (n > 0x3fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_parentage: 2^30 individuals or more");
    const long linc = bedld_count(include, L);
    if (linc < 1) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_parentage: include selects no marker");
    if (int rc = parentage_check(ctx, "bed_parentage", n, linc, offspring, n_o, sires, n_s, dams, n_d, min_overlap, allow_self)) return rc;
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_parentage: no context");
    GenoPlanes g;
    int rc = g.build(ctx, "bed_parentage", true, bed_path, n, L, include, linc, max_memory_in_Gbytes, parentage_extra_bytes(3, linc, n_o, n_s, n_d),
                     "the candidates' planes and the partial minima");
    if (rc) return rc;
    return parentage_run(ctx, g, offspring, n_o, sires, n_s, dams, n_d, (int)min_overlap, allow_self, best_out);
}

// ---------------------------------------------------------------------------------------------------------------
// Transmission disequilibrium test of trios (include/eagle_hip.h section 1b''''viii; kernels in eagle_tdt.hip, the flips' product in
// eagle_maxt.hip).  The planes are GenoPlanes::build's; the trio pass and its finish give the counts and the observed key; with R >= 1 the
// int8 image of d is built in bands of whole 128-marker tiles and each band goes through k_maxt_tile against the sign operand.
// ---------------------------------------------------------------------------------------------------------------
static_assert(TDT_MAX_FLIP_TRIOS == EAGLE_MAXT_MAX_N, "a flip's trios are the tile's K dimension");
namespace {

// What a call holds beside the planes, and the rows of an image band.  `fixed`: the trio list, the per-trio and per-marker arrays and,
// with flips, the families, S, count1, the sign operand, the tile partials and the per-flip maxima; the band takes what is left of the
// budget, whole 128-marker tiles, at least one, at most 2 GiB.
struct TdtPlan { long ld = 0, band = 0, tiles = 0; size_t extra = 0; };
TdtPlan tdt_plan(size_t budget, size_t plane_bytes, long lp, long ntrios, long R) {
    TdtPlan p;
    const size_t T = (size_t)ntrios, Lp = (size_t)lp;
    size_t fixed = (size_t)36 * T + (size_t)44 * Lp;      // trios, trio_out; marker_out (5 int32), d_obs, V, key_obs
    if (R < 1) { p.extra = fixed; return p; }
    p.ld = (ntrios + 15) / 16 * 16;
    p.tiles = (lp + 127) / 128;
    fixed += (size_t)4 * T + (size_t)8 * Lp + (size_t)R * (size_t)p.ld + (size_t)12 * (size_t)R * (size_t)p.tiles + (size_t)12 * (size_t)R;
    const size_t used = plane_bytes + fixed, left = budget > used ? budget - used : 0;
    const long fit = (long)std::min<size_t>(left, (size_t)1 << 31) / p.ld / 128 * 128;
    p.band = std::min(p.tiles * 128, std::max(128L, fit));
    p.extra = fixed + (size_t)p.band * (size_t)p.ld;
    return p;
}

// Both entry points: the route's name, the checks that need no context, the planes, the kernels, the downloads.
int tdt_call(eagle_ctx* ctx, const char* who, bool is_bed, const char* path, const long dims[2], const uint8_t* include, const int32_t* trios,
             long ntrios, const int32_t* family, uint64_t seed, long first, long R, double mem_gb, int32_t* trio_out, int32_t* marker_out,
             double* key_obs, int32_t* count1, double* maxkey, int32_t* argmax) {
    char msg[200];
    auto fail = [&](const char* what) {
        snprintf(msg, sizeof msg, "%s: %s", who, what);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    };
    if (!path || !dims || !trios || !trio_out || !marker_out || !key_obs) return fail("NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return fail("dims must be positive");
    if (is_bed && n > 0x3fffffffL) return fail("2^30 individuals or more");
    const long lp = is_bed ? bedld_count(include, L) : L;
    if (lp < 1) return fail("include selects no marker");
    if (const char* bad = tdt_arg_error(lp, ntrios, family, first, R)) return fail(bad);
    if (R >= 1 && (!count1 || !maxkey || !argmax)) return fail("NULL argument (count1, maxkey and argmax are needed with R >= 1)");
    const long k = mendel_trios_check(trios, ntrios, n);
    if (k >= 0) {
        snprintf(msg, sizeof msg, "%s: trio %ld is not (c, f, m) with 0 <= c < n, -1 <= f, m < n, c != f, c != m, f != m", who, k);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    }
    if (!ctx) return fail("no context");

    GenoPlanes g;
    g.n = n;
    g.lp = lp;
    g.nplanes = is_bed ? 3 : 2;
    size_t budget = 0;
    if (int rc = GenoPlanes::budget_bytes(ctx, &budget)) return rc;
    const TdtPlan plan = tdt_plan(budget, g.bytes(), lp, ntrios, R);
    int rc = g.build(ctx, who, is_bed, path, n, L, include, lp, mem_gb, plan.extra,
                     "the per-trio and per-marker arrays, the image band, the sign operand and the tile partials");
    if (rc) return rc;

    hipStream_t st = ctx->stream;
    const size_t T = (size_t)ntrios, Lp = (size_t)lp;
    std::vector<int32_t> fam;
    DevBuf d_trios, d_out, d_marker, dD, dV, dK, d_fam, op, dS, dC, pkey, parg, dmax, darg, img;
    HIPCHK(ctx, d_trios.alloc(sizeof(int32_t) * 3 * T));
    HIPCHK(ctx, d_out.alloc(sizeof(int32_t) * 6 * T));
    HIPCHK(ctx, d_marker.alloc(sizeof(int32_t) * 5 * Lp));
    HIPCHK(ctx, dD.alloc(sizeof(int64_t) * Lp));
    HIPCHK(ctx, dV.alloc(sizeof(int64_t) * Lp));
    HIPCHK(ctx, dK.alloc(sizeof(double) * Lp));
    if (R >= 1) {
        HIPCHK(ctx, d_fam.alloc(sizeof(int32_t) * T));
        HIPCHK(ctx, op.alloc((size_t)R * (size_t)plan.ld));
        HIPCHK(ctx, dS.alloc(sizeof(int32_t) * Lp));
        HIPCHK(ctx, dC.alloc(sizeof(int32_t) * Lp));
        HIPCHK(ctx, pkey.alloc(sizeof(double) * (size_t)plan.tiles * (size_t)R));
        HIPCHK(ctx, parg.alloc(sizeof(int32_t) * (size_t)plan.tiles * (size_t)R));
        HIPCHK(ctx, dmax.alloc(sizeof(double) * (size_t)R));
        HIPCHK(ctx, darg.alloc(sizeof(int32_t) * (size_t)R));
        HIPCHK(ctx, img.alloc((size_t)plan.band * (size_t)plan.ld));
    }
    // every later error path drains the stream first: kernels and copies may be queued on this frame's buffers and on fam
    auto drain = [&](int code) { (void)hipStreamSynchronize(st); return code; };
    auto hip = [&](hipError_t e, const char* what) { return e == hipSuccess ? EAGLE_OK : drain(eagle_fail_hip(ctx, e, what)); };
    if ((rc = hip(hipMemcpyAsync(d_trios.p, trios, sizeof(int32_t) * 3 * T, hipMemcpyHostToDevice, st), "tdt: trio upload"))) return rc;
    if ((rc = hip(hipMemsetAsync(d_marker.p, 0, sizeof(int32_t) * 5 * Lp, st), "tdt: marker counts"))) return rc;
    rc = eagle_dev_tdt_trios(ctx, g.p(), g.nplanes, n, lp, d_trios.as<int32_t>(), ntrios, d_out.as<int32_t>(), d_marker.as<int32_t>(), st);
    if (!rc) rc = eagle_dev_tdt_finish(ctx, d_marker.as<int32_t>(), lp, dD.as<int64_t>(), dV.as<int64_t>(), dK.as<double>(), st);
    if (rc) return drain(rc);
    if (R >= 1) {
        fam.resize(T);
        if (family) std::copy(family, family + ntrios, fam.begin());
        else tdt_families(trios, ntrios, fam.data());
        if ((rc = hip(hipMemcpyAsync(d_fam.p, fam.data(), sizeof(int32_t) * T, hipMemcpyHostToDevice, st), "tdt: family upload"))) return rc;
        if ((rc = hip(hipMemsetAsync(dS.p, 0, sizeof(int32_t) * Lp, st), "tdt: S"))) return rc;
        if ((rc = hip(hipMemsetAsync(dC.p, 0, sizeof(int32_t) * Lp, st), "tdt: count1"))) return rc;
        rc = eagle_dev_tdt_signs(ctx, d_fam.as<int32_t>(), ntrios, seed, first, R, op.as<int8_t>(), plan.ld, st);
        long tile_base = 0;
        for (long m0 = 0; m0 < lp && !rc; m0 += plan.band) {   // stream order: a band's tile has read the image before the next band writes it
            const long rows = std::min(plan.band, lp - m0);
            rc = eagle_dev_tdt_image(ctx, g.p(), g.nplanes, n, lp, d_trios.as<int32_t>(), ntrios, m0, rows, img.as<int8_t>(), plan.ld, st);
            if (!rc) rc = eagle_dev_maxt_tile(ctx, 0, img.as<int8_t>(), rows, ntrios, plan.ld, op.as<int8_t>(), plan.ld, 1, R, R, 1, 0,
                                              dS.as<int32_t>() + m0, dV.as<int64_t>() + m0, dD.as<int64_t>() + m0, dK.as<double>() + m0,
                                              dC.as<int32_t>() + m0, pkey.as<double>(), parg.as<int32_t>(), tile_base, m0, st);
            tile_base += (rows + 127) / 128;
        }
        if (!rc) rc = eagle_dev_maxt_finish(ctx, pkey.as<double>(), parg.as<int32_t>(), tile_base, R, dmax.as<double>(), darg.as<int32_t>(), st);
        if (rc) return drain(rc);
        if ((rc = hip(hipMemcpyAsync(count1, dC.p, sizeof(int32_t) * Lp, hipMemcpyDeviceToHost, st), "tdt: download"))) return rc;
        if ((rc = hip(hipMemcpyAsync(maxkey, dmax.p, sizeof(double) * (size_t)R, hipMemcpyDeviceToHost, st), "tdt: download"))) return rc;
        if ((rc = hip(hipMemcpyAsync(argmax, darg.p, sizeof(int32_t) * (size_t)R, hipMemcpyDeviceToHost, st), "tdt: download"))) return rc;
    }
    if ((rc = hip(hipMemcpyAsync(trio_out, d_out.p, sizeof(int32_t) * 6 * T, hipMemcpyDeviceToHost, st), "tdt: download"))) return rc;
    if ((rc = hip(hipMemcpyAsync(marker_out, d_marker.p, sizeof(int32_t) * 5 * Lp, hipMemcpyDeviceToHost, st), "tdt: download"))) return rc;
    if ((rc = hip(hipMemcpyAsync(key_obs, dK.p, sizeof(double) * Lp, hipMemcpyDeviceToHost, st), "tdt: download"))) return rc;
    return hip(hipStreamSynchronize(st), "tdt: synchronize");
}

}  // namespace

extern "C" int eagle_tdt(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], const int32_t* trios, long ntrios, const int32_t* family,
                         uint64_t seed, long first, long R, double max_memory_in_Gbytes, int32_t* trio_out, int32_t* marker_out, double* key_obs,
                         int32_t* count1, double* maxkey, int32_t* argmax) {
    return tdt_call(ctx, "tdt", false, f_name_ascii_M, dims, nullptr, trios, ntrios, family, seed, first, R, max_memory_in_Gbytes, trio_out, marker_out,
                    key_obs, count1, maxkey, argmax);
}

extern "C" int eagle_bed_tdt(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, const int32_t* trios, long ntrios,
                             const int32_t* family, uint64_t seed, long first, long R, double max_memory_in_Gbytes, int32_t* trio_out,
                             int32_t* marker_out, double* key_obs, int32_t* count1, double* maxkey, int32_t* argmax) {
    return tdt_call(ctx, "bed_tdt", true, bed_path, dims, include, trios, ntrios, family, seed, first, R, max_memory_in_Gbytes, trio_out, marker_out,
                    key_obs, count1, maxkey, argmax);
}

// The loci's rows are gathered into a 64-row image first (k_gather_rows_i8: from the resident image, else from their own lines of
// the file, each distinct line read once), then every tile of Mt multiplies against it, where it lies or window by window.
extern "C" int eagle_ld_dots(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const long* loci, long nloci,
                             double max_memory_in_Gbytes, int32_t* dots_out) {
    if (!f_name_ascii_Mt || !dims || !loci || !dots_out) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_dots: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0 || L > 0x7fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_dots: bad dims");
    if (nloci < 1 || nloci > 64) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_dots: the number of loci must be in [1, 64]");
    for (long i = 0; i < nloci; i++)
        if (loci[i] < 0 || loci[i] >= L) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_dots: locus outside [0, L)");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "ld_dots: no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long k = nloci;
    ImageLines lines;
    int rc = lines.open(ctx, f_name_ascii_Mt, L, n, max_memory_in_Gbytes);
    if (rc) return rc;
    LociRows B;
    DevBuf dots;
    HIPCHK(ctx, dots.alloc(sizeof(int32_t) * (size_t)L * (size_t)k));
    rc = B.gather(lines, loci, k);
    if (rc) return rc;
    rc = lines.each(lines.disjoint(ld_stream_rows(lines)), [&](const int8_t* img, long r0, long nr, long, long) {
        return eagle_dev_ld_dots(ctx, img, nr, n, lines.ld(), B.rows(), k, dots.as<int32_t>() + r0 * k, ctx->stream);
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(dots_out, dots.p, sizeof(int32_t) * (size_t)L * (size_t)k, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Sample QC: per-individual counts, pairwise IBS counts, the Hardy-Weinberg exact test (no counterpart in the reference; kernels in
// eagle_qc.hip, Q's operand pass in eagle_i8mfma.hip, the two Gram products in eagle_api.cpp)
// ---------------------------------------------------------------------------------------------------------------

// A line of M.ascii is an individual: k_marker_counts on the individual-major image, where it lies or in bands of whole lines.
extern "C" int eagle_sample_counts(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], double max_memory_in_Gbytes,
                                   int32_t* counts_out) {
    if (!f_name_ascii_M || !dims || !counts_out) return qc_fail(ctx, EAGLE_ERR_ARG, "sample_counts: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "sample_counts: dims must be positive");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "sample_counts: no context");
    return line_counts(ctx, f_name_ascii_M, L, n, max_memory_in_Gbytes, counts_out);
}

// The windows of eagle_bed_marker_counts through the same staging ring; every window's counts are added to the n x 4 array in HBM.
extern "C" int eagle_bed_sample_counts(eagle_ctx* ctx, const char* bed_path, const long dims[2], double max_memory_in_Gbytes,
                                       int32_t* counts_out) {
    if (!bed_path || !dims || !counts_out) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_sample_counts: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0 || L > 0x7fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_sample_counts: bad dims");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_sample_counts: no context");
    BedRing ring;
    if (int orc = ring.open(ctx, bed_path, n, L)) return orc;
    const long w = std::min(std::min(L, 1L << 25), bed_stage_rows(ring.rb, max_memory_in_Gbytes));
    int rc = ring.ensure(w);
    if (rc) return rc;
    DevBuf counts;
    HIPCHK(ctx, counts.alloc(sizeof(int32_t) * 4 * (size_t)n));
    HIPCHK(ctx, hipMemsetAsync(counts.p, 0, sizeof(int32_t) * 4 * (size_t)n, ctx->stream));
    rc = ring.each(L, w, [&](long, long nr, const uint8_t* raw) {
        const int brc = eagle_dev_bed_sample_counts(ctx, raw, nr, n, counts.as<int32_t>(), ctx->stream);
        return brc ? brc : ring.release();
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(counts_out, counts.p, sizeof(int32_t) * 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

extern "C" int eagle_sample_ibs(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], double max_memory_in_Gbytes, int32_t* ibs0_out,
                                int32_t* hethet_out) {
    if (!f_name_ascii_M || !dims || !ibs0_out || !hethet_out) return qc_fail(ctx, EAGLE_ERR_ARG, "sample_ibs: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0 || L > 0x7fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "sample_ibs: bad dims");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "sample_ibs: no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return eagle_ibs_counts(ctx, f_name_ascii_M, n, L, max_memory_in_Gbytes, host_threads(), ibs0_out, hethet_out);
}

// Pairwise-complete counts from the .bed file itself (include/eagle_hip.h section 1b'''ii).  The windows of eagle_bed_marker_counts
// through the same staging ring -- cut further only where padding n to 256 rows would let one operand plane pass 128 MiB -- and per
// window ONE k_bed_pack_fp4 launch that writes the four operand planes side by side into the ctx-owned operand buffer (at most 512 MiB),
// then the four SYRKs into four accumulators that live for the whole call.  The window's marker count is padded to 256 with zero nibbles.
extern "C" int eagle_bed_sample_ibs(eagle_ctx* ctx, const char* bed_path, const long dims[2], const uint8_t* include, int min_overlap,
                                    double max_memory_in_Gbytes, int32_t* ncalled_out, int32_t* ibs0_out, int32_t* hethet_out,
                                    int32_t* hetsum_out, uint32_t* dist_out) {
    if (!bed_path || !dims || !ncalled_out || !ibs0_out || !hethet_out || !hetsum_out) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_sample_ibs: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_sample_ibs: dims must be positive");
    if (L >= (1L << 29)) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_sample_ibs: 2^29 markers or more");
    if (min_overlap < 1) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_sample_ibs: min_overlap must be at least 1");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "bed_sample_ibs: no context");
    BedRing ring;
    if (int orc = ring.open(ctx, bed_path, n, L)) return orc;
    const long np = eagle_pad(n);
    const long wplane = std::max(256L, (long)(((size_t)1 << 28) / (size_t)np) / 256 * 256);   // markers of a 128 MiB operand plane
    const long w = std::min(std::min(L, wplane), bed_stage_rows(ring.rb, max_memory_in_Gbytes));
    int rc = ring.ensure(w);
    if (rc) return rc;
    const long wp = eagle_pad(w), ld4 = wp / 2;
    const size_t plane = (size_t)np * (size_t)ld4, accn = (size_t)np * np;
    uint8_t* m4 = (uint8_t*)eagle_ctx_f4_buffer(ctx, 4 * plane);
    if (!m4) return EAGLE_ERR_HIP;
    DevBuf acc, dinc;
    HIPCHK(ctx, acc.alloc(sizeof(int32_t) * 4 * accn));
    HIPCHK(ctx, hipMemsetAsync(acc.p, 0, sizeof(int32_t) * 4 * accn, ctx->stream));
    long linc = L;
    if (include) {
        linc = 0;
        for (long m = 0; m < L; m++) linc += include[m] != 0;
        HIPCHK(ctx, dinc.alloc((size_t)L));
        HIPCHK(ctx, hipMemcpyAsync(dinc.p, include, (size_t)L, hipMemcpyHostToDevice, ctx->stream));
    }
    rc = ring.each(L, w, [&](long r0, long nr, const uint8_t* raw) {
        const long nrp = eagle_pad(nr);
        int brc = eagle_dev_bed_pack_fp4(ctx, raw, nr, n, include ? dinc.as<uint8_t>() + r0 : nullptr, np, nrp, m4, ld4, (long)plane, ctx->stream);
        if (!brc) brc = ring.release();     // the staging buffer is free once the pack has read it
        for (int p = 0; p < 4 && !brc; p++)
            brc = eagle_dev_mmt_accumulate_f4(ctx, m4 + (size_t)p * plane, np, nrp, ld4, acc.as<int32_t>() + (size_t)p * accn, ctx->stream);
        return brc;
    });
    if (rc) return rc;
    rc = eagle_bed_ibs_results(ctx, acc.as<int32_t>(), n, linc, min_overlap, ncalled_out, ibs0_out, hethet_out, hetsum_out, dist_out);
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

extern "C" int eagle_knn_rows_dist(eagle_ctx* ctx, const uint32_t* dist, long n, int K, int32_t* nbr_out) {
    if (!dist || !nbr_out) return qc_fail(ctx, EAGLE_ERR_ARG, "knn_rows_dist: NULL argument");
    if (n <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "knn_rows_dist: n must be positive");
    if (n > EAGLE_KNN_MAX_N) return qc_fail(ctx, EAGLE_ERR_ARG, "knn_rows_dist: more than EAGLE_KNN_MAX_N individuals");
    if (K < 1 || K > EAGLE_KNN_MAX_K) return qc_fail(ctx, EAGLE_ERR_ARG, "knn_rows_dist: K outside [1, 256]");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "knn_rows_dist: no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t mb = sizeof(uint32_t) * (size_t)n * (size_t)n, nb = sizeof(int32_t) * (size_t)n * (size_t)K;
    DevBuf dd, dn;
    HIPCHK(ctx, dd.alloc(mb));
    HIPCHK(ctx, dn.alloc(nb));
    HIPCHK(ctx, hipMemcpyAsync(dd.p, dist, mb, hipMemcpyHostToDevice, ctx->stream));
    int rc = eagle_dev_knn_rows_dist(ctx, dd.as<uint32_t>(), n, K, dn.as<int32_t>(), ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    HIPCHK(ctx, hipMemcpyAsync(nbr_out, dn.p, nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

extern "C" int eagle_hwe_exact(eagle_ctx* ctx, const int32_t* counts, long L, int stride, double* p_out) {
    if (!counts || !p_out) return qc_fail(ctx, EAGLE_ERR_ARG, "hwe_exact: NULL argument");
    if (L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "hwe_exact: the number of markers must be positive");
    if (stride != 3 && stride != 4) return qc_fail(ctx, EAGLE_ERR_ARG, "hwe_exact: stride must be 3 or 4");
    for (long i = 0; i < L; i++) {
        const int32_t* c = counts + i * stride;
        if (c[0] < 0 || c[1] < 0 || c[2] < 0 || (long)c[0] + c[1] + c[2] > (1L << 30))
            return qc_fail(ctx, EAGLE_ERR_ARG, "hwe_exact: a count is negative or a marker has more than 2^30 genotypes");
    }
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "hwe_exact: no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf dc, dp;
    const size_t cb = sizeof(int32_t) * (size_t)L * (size_t)stride;
    HIPCHK(ctx, dc.alloc(cb));
    HIPCHK(ctx, dp.alloc(sizeof(double) * (size_t)L));
    HIPCHK(ctx, hipMemcpyAsync(dc.p, counts, cb, hipMemcpyHostToDevice, ctx->stream));
    int rc = eagle_dev_hwe_exact(ctx, dc.as<int32_t>(), L, stride, dp.as<double>(), ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    HIPCHK(ctx, hipMemcpyAsync(p_out, dp.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// GRM: the per-marker weighted Gram product (no counterpart in the reference; kernels in eagle_grm.hip, the windows in eagle_api.cpp)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int eagle_weighted_gram(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], const uint32_t* q,
                                   double max_memory_in_Gbytes, int64_t* Q_out) {
    if (!f_name_ascii_M || !dims || !q || !Q_out) return qc_fail(ctx, EAGLE_ERR_ARG, "weighted_gram: NULL argument");
    const long n = dims[0], L = dims[1];
    if (n <= 0 || L <= 0) return qc_fail(ctx, EAGLE_ERR_ARG, "weighted_gram: dims must be positive");
    if (L > 0x7fffffffL) return qc_fail(ctx, EAGLE_ERR_ARG, "weighted_gram: 2^31 markers or more");
    if (L > EAGLE_WGRAM_MAX_MARKERS)
        return qc_fail(ctx, EAGLE_ERR_ARG, "weighted_gram: more than 16,909,320 markers (the int32 accumulator of a digit plane holds 127 L)");
    for (long m = 0; m < L; m++)
        if (q[m] >= (1u << 21)) return qc_fail(ctx, EAGLE_ERR_ARG, "weighted_gram: a weight is 2^21 or more");
    if (!ctx) return qc_fail(ctx, EAGLE_ERR_ARG, "weighted_gram: no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return eagle_wgram(ctx, f_name_ascii_M, n, L, q, max_memory_in_Gbytes, host_threads(), Q_out);
}

// ---------------------------------------------------------------------------------------------------------------
// Line scores (no counterpart in the reference; include/eagle_hip.h section 1b''''i, kernels in eagle_score.hip)
// ---------------------------------------------------------------------------------------------------------------
// out[r * T + t] = sum_c w[t * cols + c] g[r][c] for the `rows` lines of `cols` characters of a genotype file, read as line_counts reads
// it: the resident image where it lies, else bands of whole lines through eagle_dev_load_ascii.  The weights become one digit image per
// call; every band's rows are finished before the next band is read.
static int line_scores(eagle_ctx* ctx, const char* path, long rows, long cols, const int32_t* w, long T, int plane_mask,
                       double max_memory_in_Gbytes, int64_t* out) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t outb = sizeof(int64_t) * (size_t)rows * (size_t)T;
    if (!plane_mask) {   // every weight is zero: no product, and the file is not read
        memset(out, 0, outb);
        return EAGLE_OK;
    }
    // a resident image has 256-padded lines; the longest lines the engine addresses fit it only at the 128-padding of a band
    const bool narrow = (double)eagle_pad(cols) * 256.0 >= 2147483648.0;
    ImageLines lines;
    int rc = lines.open(ctx, path, rows, cols, max_memory_in_Gbytes, narrow, (cols + 127) / 128 * 128);
    if (rc) return rc;
    const long ld = lines.ld();
    const long band = lines.resident() ? rows : std::min(rows, lines.stream_rows());
    DevBuf dw, dB, c32, dout;
    HIPCHK(ctx, dout.alloc(outb));
    HIPCHK(ctx, dw.alloc(sizeof(int32_t) * (size_t)T * (size_t)cols));
    HIPCHK(ctx, dB.alloc((size_t)eagle_score_b_rows(T, plane_mask) * (size_t)ld));
    HIPCHK(ctx, c32.alloc(eagle_line_scores_ws_bytes(band, T, plane_mask)));
    HIPCHK(ctx, hipMemcpyAsync(dw.p, w, sizeof(int32_t) * (size_t)T * (size_t)cols, hipMemcpyHostToDevice, ctx->stream));
    rc = eagle_dev_score_digits(ctx, dw.as<int32_t>(), T, cols, ld, plane_mask, dB.as<int8_t>(), ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    rc = lines.each(row_windows_disjoint(rows, band), [&](const int8_t* img, long r0, long nr, long, long) {
        return eagle_dev_line_scores(ctx, img, nr, cols, ld, dB.as<int8_t>(), T, plane_mask, c32.as<int32_t>(), dout.as<int64_t>() + r0 * T, ctx->stream);
    }, eagle_pad(band));   // eagle_dev_line_scores wants the rows up to the next multiple of 256 allocated
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out, dout.p, outb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return EAGLE_OK;
}

static_assert(SCORES_MAX_COLUMNS == EAGLE_SCORES_MAX_COLUMNS && SCORES_MAX_WEIGHT == EAGLE_SCORES_MAX_WEIGHT && SCORES_MAX_LINE == EAGLE_SCORES_MAX_LINE,
              "eagle_host.h restates the limits of include/eagle_hip.h");
static int scores_entry(eagle_ctx* ctx, const char* who, const char* path, const long dims[2], bool by_marker, const int32_t* w, long T,
                        double max_memory_in_Gbytes, int64_t* out) {
    char msg[160];
    if (!path || !dims || !w || !out) { snprintf(msg, sizeof msg, "%s: NULL argument", who); return qc_fail(ctx, EAGLE_ERR_ARG, msg); }
    const long n = dims[0], L = dims[1];
    const long rows = by_marker ? L : n, cols = by_marker ? n : L;
    int plane_mask = 0;
    if (n <= 0 || L <= 0) { snprintf(msg, sizeof msg, "%s: dims must be positive", who); return qc_fail(ctx, EAGLE_ERR_ARG, msg); }
    if (const char* bad = scores_arg_error(rows, cols, T, w, &plane_mask)) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return qc_fail(ctx, EAGLE_ERR_ARG, msg);
    }
    if (!ctx) { snprintf(msg, sizeof msg, "%s: no context", who); return qc_fail(ctx, EAGLE_ERR_ARG, msg); }
    return line_scores(ctx, path, rows, cols, w, T, plane_mask, max_memory_in_Gbytes, out);
}

extern "C" int eagle_sample_scores(eagle_ctx* ctx, const char* f_name_ascii_M, const long dims[2], const int32_t* w, long T,
                                   double max_memory_in_Gbytes, int64_t* out) {
    return scores_entry(ctx, "sample_scores", f_name_ascii_M, dims, false, w, T, max_memory_in_Gbytes, out);
}

extern "C" int eagle_marker_scores(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const int32_t* v, long T,
                                   double max_memory_in_Gbytes, int64_t* out) {
    return scores_entry(ctx, "marker_scores", f_name_ascii_Mt, dims, true, v, T, max_memory_in_Gbytes, out);
}
