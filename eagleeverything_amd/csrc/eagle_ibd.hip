// eagle_ibd.hip -- pairwise IBD-type segments (include/eagle_hip.h section 1b'''vii): shared-genotype runs between two individuals.
// Integer arithmetic only; plain HIP, nothing through LDS, no inline assembly.
//
//   Planes.  One uint64 word per individual per 64 panel markers, bit b of word w = panel marker 64 w + b.  A = hom A1, B = hom A2 and,
//   from the .bed file only, C = called.  WORD-MAJOR: word w of individual i lies at plane[w * np + i], np = n rounded up to 64, so a
//   wave whose lanes are 64 different individuals reads one word index as 512 consecutive bytes.  Bits past the last panel marker and
//   the words of the individuals n .. np - 1 are zero: a zero word holds no break, and the walk ends at the last marker whatever the
//   words say, so neither can start or extend a run.
//
//   k_ibd_planes_i8 ...... the individual-major int8 image (a line of M.ascii is an individual) -> A and B.  One wave per 64 individuals
//                          x one word: per individual the lanes read its 64 bytes of that word (one marker each) and two ballots are
//                          the words; lane t keeps those of the t-th individual, and the wave stores 512 consecutive bytes per plane.
//   k_ibd_planes_bed ..... raw SNP-major .bed rows -> A, B and C.  One wave per 256 individuals x one word: a lane owns one byte column
//                          (four individuals) and walks the 64 rows of the word, one bit per row into twelve registers -- the transpose
//                          happens in registers, a lane stores 32 consecutive bytes per plane and the wave 2 KiB.
//   The cut plane, shared by all pairs, has bit m set where a piece STARTS (rule 3); the host builds it (ibd_cut_plane, eagle_host.h).
//   k_ibd_walk<LIST,FILL>  one lane per pair.  All-pairs form: a wave takes one i and 64 consecutive j, so the words of i are one
//                          wave-uniform load and those of j one coalesced load; list form: 64 list entries, both sides gathered.  The
//                          lanes walk the words in order; per word the events are the bits of break | cut, taken by find-first-set, so
//                          a clean word costs its loads and one compare.  The run and chain state of rule 5 is five registers.  FILL =
//                          false writes the four totals of the pair (the first is its segment count); FILL = true writes the rows from
//                          the exclusive scan of those counts: sorted by (pair ordinal, s) with no sort.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

#define IBD_LAUNCH_CHECK(ctx)                                               \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

struct IbdRule { long min_snp, min_len, merge_min; int mode; };

// img: row 0 is individual r0, rows of ld bytes; the individuals [r0, r0 + nr) of n.  blockIdx.x = group * nwords + word; group g holds the
// individuals r0 + 64 g ...  When the band is the last one (r0 + nr == n) its last group also writes the zero words of n .. np - 1.
__global__ __launch_bounds__(64) void k_ibd_planes_i8(const int8_t* __restrict__ img, long ld, long r0, long nr, long n, long np, long L,
                                                      long nwords, uint64_t* __restrict__ A, uint64_t* __restrict__ B) {
    const long g = (long)blockIdx.x / nwords, w = (long)blockIdx.x - g * nwords;
    const int lane = threadIdx.x;
    const long m = 64 * w + lane;
    const bool live = m < L;
    const long left = nr - 64 * g;                       // individuals of this group inside the band
    const int cnt = left < 64 ? (int)left : 64;
    uint64_t a = 0, b = 0;
    for (int t0 = 0; t0 < cnt; t0 += 8) {
        int8_t v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            v[u] = 0;
            if (live && t0 + u < cnt) v[u] = img[(64 * g + t0 + u) * ld + m];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint64_t ba = __ballot(v[u] == -1), bb = __ballot(v[u] == 1);
            if (lane == t0 + u) { a = ba; b = bb; }
        }
    }
    const long i = r0 + 64 * g + lane;
    if (lane < cnt || (r0 + nr == n && i < np)) {
        A[w * np + i] = a;
        B[w * np + i] = b;
    }
}

// bed: row 0 is panel marker g0 (rows of rb = ceil(n / 4) bytes; the row of marker g0 + p at offs[p] when offs is given).  The words
// [w0, w1) of the planes; blockIdx.x = (word - w0) * groups + group, group g = the byte columns 64 g ...
__global__ __launch_bounds__(64) void k_ibd_planes_bed(const uint8_t* __restrict__ bed, long rb, const long* __restrict__ offs, long n, long np,
                                                       long g0, long w0, long L, long groups, uint64_t* __restrict__ A,
                                                       uint64_t* __restrict__ B, uint64_t* __restrict__ Cc) {
    const long w = w0 + (long)blockIdx.x / groups, g = (long)blockIdx.x % groups;
    const int lane = threadIdx.x;
    const long col = 64 * g + lane;
    const bool live = col < rb;
    const long left = L - 64 * w;
    const int rows = left < 64 ? (int)left : 64;
    uint64_t a[4], b[4], c[4];
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] = b[k] = c[k] = 0;
    for (int t0 = 0; t0 < rows; t0 += 8) {
        uint32_t x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            x[u] = 0x55u;                                // four not-called codes
            if (live && t0 + u < rows) {
                const long p = 64 * w + t0 + u - g0;
                x[u] = bed[(offs ? offs[p] : p) * rb + col];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t code = (x[u] >> (2 * k)) & 3u;
                a[k] |= (uint64_t)(code == 0u) << (t0 + u);
                b[k] |= (uint64_t)(code == 3u) << (t0 + u);
                c[k] |= (uint64_t)(code != 1u) << (t0 + u);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long i = 4 * col + k;
        if (i < np) {                                    // padding bits of a row's last byte and the individuals n .. np - 1: zero words
            const bool real = i < n;
            A[w * np + i] = real ? a[k] : 0ull;
            B[w * np + i] = real ? b[k] : 0ull;
            Cc[w * np + i] = real ? c[k] : 0ull;
        }
    }
}

// The state of rule 5 for one pair.  cur: where the open pure run would start (the piece's first marker or the last break + 1); a chain
// of k >= 1 closed pure runs cs .. ce is open iff have, and then ce + 2 == cur (one break lies between).
struct IbdWalk {
    long cur, cs, ce;
    int k;
    bool have, pe;     // pe: the chain's last run is eligible
};

// blk: nb + 1 block bounds (the block ordinal of a row).  pairs null (LIST false): grid (ceil((n - 1) / 64), n - 1), the wave of (x, y)
// takes i = y and j = i + 1 + 64 x ...  pairs given (LIST true): grid ceil(P / 64), lane = list entry.  tot: P x 4; offs: P; seg rows of six.
template <bool LIST, bool FILL>
__global__ __launch_bounds__(64) void k_ibd_walk(const uint64_t* __restrict__ A, const uint64_t* __restrict__ B, const uint64_t* __restrict__ Cc,
                                                 const uint64_t* __restrict__ cut, long np, long n, long L, long nwords,
                                                 const int32_t* __restrict__ pairs, long P, const int32_t* __restrict__ blk, int nb,
                                                 const int64_t* __restrict__ pos, IbdRule R, int64_t* __restrict__ tot,
                                                 const int64_t* __restrict__ offs, int32_t* __restrict__ seg) {
    const int lane = threadIdx.x;
    long i, j, ord;
    bool live;
    if (LIST) {
        ord = 64 * (long)blockIdx.x + lane;
        live = ord < P;
        i = live ? pairs[2 * ord] : 0;
        j = live ? pairs[2 * ord + 1] : 0;
    } else {
        i = blockIdx.y;
        if (i + 1 + 64 * (long)blockIdx.x >= n) return;  // an empty tile of the triangle (wave-uniform)
        j = i + 1 + 64 * (long)blockIdx.x + lane;
        live = j < n;
        if (!live) j = n - 1;
        ord = i * n - i * (i + 1) / 2 + (j - i - 1);
    }
    IbdWalk S = {0, 0, 0, 0, false, false};
    long count = 0, sum_snp = 0, sum_len = 0, longest = 0;
    long out = (FILL && live) ? offs[ord] : 0;

    auto emit = [&]() {                                  // the open chain is a candidate (rule 6)
        const long nsnp = S.ce - S.cs + 1;
        if (live && nsnp >= R.min_snp) {                  // a lane without a pair walks clean words: it must not report them
            const long len = pos ? pos[S.ce] - pos[S.cs] : S.ce - S.cs;
            if (len >= R.min_len) {
                if (FILL) {
                    int b = 0;                           // the last b with blk[b] <= cs
                    for (int hi = nb - 1; b < hi;) {
                        const int mid = (b + hi + 1) >> 1;
                        if ((long)blk[mid] <= S.cs) b = mid; else hi = mid - 1;
                    }
                    int32_t* row = seg + 6 * out;
                    row[0] = (int32_t)i; row[1] = (int32_t)j; row[2] = (int32_t)S.cs; row[3] = (int32_t)S.ce; row[4] = S.k - 1; row[5] = b;
                    out++;
                } else {
                    count++;
                    sum_snp += nsnp;
                    sum_len += len;
                    if (len > longest) longest = len;
                }
            }
        }
        S.have = false;
    };
    // the pure run cur .. m - 1 (when it has a marker) ends at m: at a break (brk) or at a cut / the end of the panel
    auto close_run = [&](long m, bool brk) {
        const long rl = m - S.cur;
        if (rl > 0) {
            const bool el = R.merge_min >= 1 && rl >= R.merge_min;
            if (S.have && S.pe && el) {
                S.ce = m - 1;
                S.k++;
            } else {
                if (S.have) emit();
                S.cs = S.cur; S.ce = m - 1; S.k = 1; S.have = true;
            }
            S.pe = el;
            if (!brk) emit();
        } else if (S.have) {
            emit();                                      // two breaks in a row, or a cut right after a break
        }
        S.cur = brk ? m + 1 : m;
    };

    uint64_t ai = A[i], bi = B[i], aj = A[j], bj = B[j], ci = Cc ? Cc[i] : 0, cj = Cc ? Cc[j] : 0;
    for (long w = 0; w < nwords; w++) {
        const uint64_t xai = ai, xbi = bi, xaj = aj, xbj = bj, xci = ci, xcj = cj;
        if (w + 1 < nwords) {                            // the next word's loads fly while this word's events are worked on
            const long o = (w + 1) * np;
            ai = A[o + i]; bi = B[o + i]; aj = A[o + j]; bj = B[o + j];
            if (Cc) { ci = Cc[o + i]; cj = Cc[o + j]; }
        }
        uint64_t brk = R.mode == 1 ? ((xai & xbj) | (xbi & xaj)) : ((xai ^ xaj) | (xbi ^ xbj));
        if (Cc) brk &= xci & xcj;
        if (!live) brk = 0;
        const uint64_t cw = cut[w];
        uint64_t ev = brk | cw;
        while (ev) {
            const int b = __ffsll((unsigned long long)ev) - 1;
            const uint64_t bit = 1ull << b;
            ev &= ev - 1;
            const long m = 64 * w + b;
            if (cw & bit) close_run(m, false);
            if (brk & bit) close_run(m, true);
        }
    }
    close_run(L, false);
    if (!FILL && live) {
        tot[4 * ord + 0] = count;
        tot[4 * ord + 1] = sum_snp;
        tot[4 * ord + 2] = sum_len;
        tot[4 * ord + 3] = longest;
    }
}

// The plane words of the individuals [r0, r0 + nr) from an individual-major int8 image whose row 0 is individual r0.  planes: A then B,
// each ceil(L / 64) x np uint64.
extern "C" int eagle_dev_ibd_planes_i8(eagle_ctx* ctx, const int8_t* img, long ld, long r0, long nr, long n, long L, uint64_t* planes,
                                       void* stream) {
    if (nr <= 0) return EAGLE_OK;
    if (n <= 0 || L <= 0 || L > 0x7fffffffL || r0 < 0 || r0 + nr > n || L > ld) return eagle_fail(ctx, EAGLE_ERR_ARG, "ibd_planes: bad shape");
    const long np = (n + 63) / 64 * 64, nwords = (L + 63) / 64;
    const long groups = r0 + nr == n ? (np - r0 + 63) / 64 : (nr + 63) / 64;
    if (groups * nwords > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "ibd_planes: too many individuals x markers for one launch");
    uint64_t* A = planes;
    uint64_t* B = planes + (size_t)nwords * (size_t)np;
    hipLaunchKernelGGL(k_ibd_planes_i8, dim3((unsigned)(groups * nwords)), dim3(64), 0, (hipStream_t)stream, img, ld, r0, nr, n, np, L, nwords, A, B);
    IBD_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// The plane words [w0, w1) from raw .bed rows: the row of panel marker g0 + p is row offsets[p] of `bed` (offsets null: row p), checked
// by the CALLER for the markers [64 w0, min(L, 64 w1)).  planes: A, B, C.
extern "C" int eagle_dev_ibd_planes_bed(eagle_ctx* ctx, const uint8_t* bed, const long* offsets, long n, long g0, long w0, long w1, long L,
                                        uint64_t* planes, void* stream) {
    if (w1 <= w0) return EAGLE_OK;
    const long nwords = (L + 63) / 64;
    if (n <= 0 || n > 0x3fffffffL || L <= 0 || L > 0x7fffffffL || w0 < 0 || w1 > nwords || g0 < 0 || g0 > 64 * w0)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "ibd_planes: bad shape");
    const long np = (n + 63) / 64 * 64, groups = np / 256 + (np % 256 != 0);
    if (groups * (w1 - w0) > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "ibd_planes: too many individuals x markers for one launch");
    const size_t plane = (size_t)nwords * (size_t)np;
    hipLaunchKernelGGL(k_ibd_planes_bed, dim3((unsigned)(groups * (w1 - w0))), dim3(64), 0, (hipStream_t)stream, bed, bed_row_bytes(n), offsets, n, np,
                       g0, w0, L, groups, planes, planes + plane, planes + 2 * plane);
    IBD_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// fill == 0: tot (P x 4) written; fill != 0: the rows of seg from offs (P).  nplanes 2 (A, B) or 3 (A, B, C).  pairs null: all pairs.
extern "C" int eagle_dev_ibd_walk(eagle_ctx* ctx, const uint64_t* planes, int nplanes, const uint64_t* cut, long n, long L, const int32_t* pairs,
                                  long P, const int32_t* blk, long nb, const int64_t* pos, const eagle_ibd_params* prm, int fill, int64_t* tot,
                                  const int64_t* offs, int32_t* seg, void* stream) {
    if (n < 2 || L <= 0 || L > 0x7fffffffL || P < 1 || P > EAGLE_IBD_MAX_PAIRS || nb < 1 || nb > 0x7fffffffL || (nplanes != 2 && nplanes != 3) ||
        (prm->mode != 1 && prm->mode != 2))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "ibd_walk: bad shape");
    const long np = (n + 63) / 64 * 64, nwords = (L + 63) / 64;
    const size_t plane = (size_t)nwords * (size_t)np;
    const uint64_t* A = planes;
    const uint64_t* B = planes + plane;
    const uint64_t* Cc = nplanes == 3 ? planes + 2 * plane : nullptr;
    const IbdRule R = {prm->min_snp, prm->min_len, prm->merge_min, (int)prm->mode};
    hipStream_t s = (hipStream_t)stream;
    const dim3 b(64);
    if (pairs) {
        const dim3 g((unsigned)((P + 63) / 64));
        if (fill) hipLaunchKernelGGL((k_ibd_walk<true, true>), g, b, 0, s, A, B, Cc, cut, np, n, L, nwords, pairs, P, blk, (int)nb, pos, R, tot, offs, seg);
        else hipLaunchKernelGGL((k_ibd_walk<true, false>), g, b, 0, s, A, B, Cc, cut, np, n, L, nwords, pairs, P, blk, (int)nb, pos, R, tot, offs, seg);
    } else {
        if (n - 1 > 65535 || P != n * (n - 1) / 2) return eagle_fail(ctx, EAGLE_ERR_ARG, "ibd_walk: bad shape");
        const dim3 g((unsigned)((n - 1 + 63) / 64), (unsigned)(n - 1));
        if (fill) hipLaunchKernelGGL((k_ibd_walk<false, true>), g, b, 0, s, A, B, Cc, cut, np, n, L, nwords, pairs, P, blk, (int)nb, pos, R, tot, offs, seg);
        else hipLaunchKernelGGL((k_ibd_walk<false, false>), g, b, 0, s, A, B, Cc, cut, np, n, L, nwords, pairs, P, blk, (int)nb, pos, R, tot, offs, seg);
    }
    IBD_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}
