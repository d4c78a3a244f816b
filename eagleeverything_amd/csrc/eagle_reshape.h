// eagle_reshape.h -- the host side of eagle_reshape_m (E/src/ReshapeM_rcpp.cpp:17-120): the NA list check, the keep-list of
// individuals, and the FILES-mode rewrite of M.ascii / Mt.ascii.  HIP-free, so a CPU build can run it under ASan / UBSan
// (tests/test_reshape_host.py builds a small driver around it).
//
// The reference reads both files line by line and writes
//   <fnameM>tmp  : every line of M whose 0-based number is not in indxNA, followed by '\n'
//   <fnameMt>tmp : every line of Mt with the characters at the positions of indxNA erased, followed by '\n'
// and returns {lines written to M, length of the last line of M}.  Here both inputs are memory-mapped, their lines indexed by
// `threads` workers, and the output lines written with pwrite() at offsets known from the index, in parallel.  Unlike the
// reference, a duplicate index or one outside [0, dims[0]) is an argument error (its erase would drop the wrong column or
// throw), and a line of Mt too short to hold every NA column is a format error.
#ifndef EAGLE_RESHAPE_H
#define EAGLE_RESHAPE_H
#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <stdint.h>
#include <string>
#include <vector>

#include "eagle_host.h"

// 0 and `sorted` = the indices in increasing order, or the reason they are not a valid NA list of `n` individuals.
static inline const char* reshape_check_na(const long* idx, long nNA, long n, std::vector<long>& sorted) {
    if (nNA < 0 || (nNA > 0 && !idx)) return "ReshapeM: bad indxNA";
    if (n < 0) return "ReshapeM: bad dims";
    sorted.assign(idx, idx + nNA);
    std::sort(sorted.begin(), sorted.end());
    for (long i = 0; i < nNA; i++) {
        if (sorted[(size_t)i] < 0 || sorted[(size_t)i] >= n) return "ReshapeM: an index of indxNA lies outside [0, dims[0])";
        if (i > 0 && sorted[(size_t)i] == sorted[(size_t)i - 1]) return "ReshapeM: indxNA names an individual twice";
    }
    return nullptr;
}

// Positions 0 .. total-1 that are not in `sorted_na` (increasing), as int32 (the device keep-map).
static inline std::vector<int32_t> reshape_keep_list(long total, const std::vector<long>& sorted_na) {
    std::vector<int32_t> keep;
    keep.reserve((size_t)std::max(0L, total));
    size_t j = 0;
    for (long i = 0; i < total; i++) {
        while (j < sorted_na.size() && sorted_na[j] < i) j++;
        if (j < sorted_na.size() && sorted_na[j] == i) continue;
        keep.push_back((int32_t)i);
    }
    return keep;
}

struct ReshapeMap {
    int fd = -1;
    const char* p = nullptr;
    size_t size = 0;
    ~ReshapeMap() {
        if (p && size) munmap((void*)p, size);
        if (fd >= 0) close(fd);
    }
    bool open_ro(const char* path) {
        fd = open(path, O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0) return false;
        size = (size_t)st.st_size;
        if (size == 0) return true;
        void* q = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (q == MAP_FAILED) { size = 0; return false; }
        p = (const char*)q;
        (void)madvise(q, size, MADV_SEQUENTIAL);
        return true;
    }
};

// Writes the lines [0, nlines) of `in` to `out_path`; line i becomes out_len(i) bytes produced by emit(i, dst) plus '\n'.
template <class LenFn, class EmitFn>
static inline bool reshape_write(const char* out_path, long nlines, int threads, LenFn out_len, EmitFn emit) {
    std::vector<size_t> off((size_t)nlines + 1, 0);
    for (long i = 0; i < nlines; i++) off[(size_t)i + 1] = off[(size_t)i] + out_len(i) + 1;
    const int fd = open(out_path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fd < 0) return false;
    bool ok = ftruncate(fd, (off_t)off[(size_t)nlines]) == 0;
    std::atomic<bool> good{ok};
    if (ok) {
        // each worker fills a buffer of up to 8 MiB of whole lines and writes it at the lines' offset
        const long nt = off[(size_t)nlines] < ((size_t)8 << 20) ? 1 : threads;
        parallel_for(nlines, (int)nt, [&](long a, long b, int) {
            std::vector<char> buf;
            long i = a;
            while (i < b && good) {
                long j = i;
                size_t bytes = 0;
                while (j < b && (j == i || bytes + (off[(size_t)j + 1] - off[(size_t)j]) <= ((size_t)8 << 20))) {
                    bytes += off[(size_t)j + 1] - off[(size_t)j];
                    j++;
                }
                buf.resize(bytes);
                char* q = buf.data();
                for (long k = i; k < j; k++) {
                    emit(k, q);
                    q += off[(size_t)k + 1] - off[(size_t)k];
                    q[-1] = '\n';
                }
                size_t done = 0;
                while (done < bytes) {
                    ssize_t w = pwrite(fd, buf.data() + done, bytes - done, (off_t)(off[(size_t)i] + done));
                    if (w <= 0) { good = false; break; }
                    done += (size_t)w;
                }
                i = j;
            }
        });
        ok = good;
    }
    if (close(fd) != 0) ok = false;
    return ok;
}

// FILES mode.  0 and newdims, or an error code of eagle_hip.h with the reason in `msg`.
static inline int reshape_write_files(const char* fnameM, const char* fnameMt, const std::vector<long>& na, int threads,
                                      long newdims[2], std::string& msg) {
    newdims[0] = newdims[1] = 0;
    {
        ReshapeMap m;
        if (!m.open_ro(fnameM)) { msg = std::string("ERROR: Could not open  ") + fnameM; return -1; }
        LineIndex ix;
        index_lines_buf(m.p, m.size, threads, ix);
        const long nl = ix.nlines();
        std::vector<long> kept;
        kept.reserve((size_t)nl);
        size_t j = 0;
        for (long i = 0; i < nl; i++) {
            while (j < na.size() && na[j] < i) j++;
            if (!(j < na.size() && na[j] == i)) kept.push_back(i);
        }
        const std::string out = std::string(fnameM) + "tmp";
        if (!reshape_write(out.c_str(), (long)kept.size(), threads,
                           [&](long k) { return ix.end(kept[(size_t)k]) - ix.begin(kept[(size_t)k]); },
                           [&](long k, char* dst) {
                               const long r = kept[(size_t)k];
                               memcpy(dst, m.p + ix.begin(r), ix.end(r) - ix.begin(r));
                           })) {
            msg = "ERROR: Could not write  " + out;
            return -1;
        }
        newdims[0] = (long)kept.size();
        newdims[1] = nl > 0 ? (long)(ix.end(nl - 1) - ix.begin(nl - 1)) : 0;
    }
    ReshapeMap mt;
    if (!mt.open_ro(fnameMt)) { msg = std::string("ERROR: Could not open  ") + fnameMt; return -1; }
    LineIndex ix;
    index_lines_buf(mt.p, mt.size, threads, ix);
    const long nl = ix.nlines();
    const long need = na.empty() ? 0 : na.back() + 1;
    for (long i = 0; i < nl; i++)
        if ((long)(ix.end(i) - ix.begin(i)) < need) {
            msg = "ReshapeM: line " + std::to_string(i + 1) + " of " + fnameMt + " is shorter than the largest index of indxNA";
            return -2;
        }
    const std::string out = std::string(fnameMt) + "tmp";
    const long nna = (long)na.size();
    if (!reshape_write(out.c_str(), nl, threads, [&](long i) { return ix.end(i) - ix.begin(i) - (size_t)nna; },
                       [&](long i, char* dst) {
                           const char* src = mt.p + ix.begin(i);
                           const long len = (long)(ix.end(i) - ix.begin(i));
                           long from = 0;
                           for (long c : na) {  // the runs between the erased columns
                               memcpy(dst, src + from, (size_t)(c - from));
                               dst += c - from;
                               from = c + 1;
                           }
                           memcpy(dst, src + from, (size_t)(len - from));
                       })) {
        msg = "ERROR: Could not write  " + out;
        return -1;
    }
    return 0;
}
#endif
