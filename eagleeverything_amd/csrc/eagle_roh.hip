// eagle_roh.hip -- runs of homozygosity (include/eagle_hip.h section 1b'''vi): the window scan along the genome of every individual and
// the extraction of the reported segments.  Integer arithmetic only; plain HIP, nothing through LDS, no inline assembly.
//
//   k_roh_flags<SRC> ...... the genotypes of the panel markers [c0, c1) (SRC 0: the int8 marker-major image, SRC 1: raw SNP-major .bed
//                           rows) -> three marker-major bit planes, ceil(n / 64) uint64 words per marker each: FLAGGED (rule 4), HET and
//                           MISS (rule 1).  A lane owns FOUR consecutive individuals -- one dword of an image row, one byte of a .bed
//                           row, so that a wave reads 256 (64) consecutive bytes of a row -- and a wave walks one chunk of
//                           EAGLE_ROH_CHUNK markers from top to bottom, with a halo of w - 1 rows on either side, every row read once.
//                           Per individual the window state is three 64-bit shift registers, bit t = row r - t when row r has just
//                           been read: H (het), M (miss) and W (the window that ENDS at that row is valid and homozygous).  The window
//                           test is two popcounts under the mask of the low w bits.  Marker j is decided when row j + w - 1 has been
//                           read, or with all the markers still open at its block's last row: hom = popcount of the low r - j + 1
//                           bits of W (the windows that end in [j, r], all of which contain j), cover from the block's bounds, and the
//                           marker's het / miss bits are bit r - j of H / M.  Four ballots per plane, bit l = individual 4 l + k of the
//                           wave's 256, are interleaved into the four plane words (wave-uniform bit arithmetic) and stored by lanes
//                           0 .. 3.  Bits of individuals >= n are zero.
//   k_roh_segments<FILL> .. one lane per individual, one wave per 64 individuals x block: the lanes load the plane words (and positions)
//                           of 64 markers at once, one marker each, and walk them through lane broadcasts, so a marker costs no memory
//                           round trip of its own.  Rules 5 and 6.  FILL = false counts the reported segments of (individual, block)
//                           and adds the individual's totals to ind (integer atomics: integer sums and a maximum, order-free); FILL =
//                           true writes the rows from the exclusive scan of those counts: sorted by (individual, s) with no sort.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

#define ROH_LAUNCH_CHECK(ctx)                                               \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

#define ROH_IPL 4      // individuals per lane
#define ROH_BATCH 8    // rows loaded before they are worked on: that many loads in flight per lane

struct RohRule { int w, win_het, win_miss, thr16; };
struct RohSegRule { long min_snp, min_len, max_gap, max_density, max_het; };

__device__ __forceinline__ uint64_t roh_low_bits(int k) { return k >= 64 ? ~0ull : ((1ull << k) - 1ull); }
// bit i of the low 16 bits of x -> bit 4 i
__device__ __forceinline__ uint64_t roh_spread4(uint64_t x) {
    x &= 0xffffull;
    x = (x | (x << 24)) & 0x000000ff000000ffull;
    x = (x | (x << 12)) & 0x000f000f000f000full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}
// word q (individuals 64 q .. 64 q + 63 of the wave's 256) of the plane whose ballot for the lanes' k-th individuals is b[k]
__device__ __forceinline__ uint64_t roh_word(const uint64_t b[ROH_IPL], int q) {
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < ROH_IPL; k++) v |= roh_spread4(b[k] >> (16 * q)) << k;
    return v;
}

// src: row 0 is panel marker g0 (SRC 0: rows of `stride` = ld bytes, ld % 16 == 0; SRC 1: rows of `stride` = ceil(n / 4) bytes, row of
// the marker g0 + p at offs[p] when offs is given).  blk: nb + 1 block bounds.  The rows held reach from max(0, c0 - (w - 1)) to
// min(markers, c1 + w - 1) at least (the CALLER's contract).  groups = ceil(n / 256); block = chunk * groups + group.
template <int SRC>
__global__ __launch_bounds__(64) void k_roh_flags(const uint8_t* __restrict__ src, long stride, const long* __restrict__ offs, long n, long g0,
                                                  long c0, long c1, const int32_t* __restrict__ blk, int nb, RohRule R, long nw, long groups,
                                                  uint64_t* __restrict__ flagged, uint64_t* __restrict__ het, uint64_t* __restrict__ miss) {
    const long chunk = (long)blockIdx.x / groups, g = (long)blockIdx.x - chunk * groups;
    const int lane = threadIdx.x;
    const long m0 = c0 + chunk * EAGLE_ROH_CHUNK, m1 = m0 + EAGLE_ROH_CHUNK < c1 ? m0 + EAGLE_ROH_CHUNK : c1;
    const long col = SRC == 0 ? 256 * g + 4 * lane : 64 * g + lane;   // byte of a row this lane reads
    const bool live = col < stride;
    const int w = R.w;
    const uint64_t wm = roh_low_bits(w);
    // the block of marker m0: the last b with blk[b] <= m0
    int b = 0;
    for (int hi = nb - 1; b < hi;) {
        const int mid = (b + hi + 1) >> 1;
        if ((long)blk[mid] <= m0) b = mid; else hi = mid - 1;
    }
    // the words these lanes store, and the individuals < n among their 64
    const long wq = 4 * g + lane;
    const bool storer = lane < 4 && wq < nw;
    const long left = n - 64 * wq;
    const uint64_t keep = storer ? (left >= 64 ? ~0ull : roh_low_bits((int)left)) : 0ull;

    for (; b < nb && (long)blk[b] < m1; b++) {
        const long a = blk[b], e = blk[b + 1];
        const long rs = a > m0 - (w - 1) ? a : m0 - (w - 1);
        const long re = e < m1 + (w - 1) ? e : m1 + (w - 1);
        uint64_t H[ROH_IPL], M[ROH_IPL], W[ROH_IPL];
#pragma unroll
        for (int k = 0; k < ROH_IPL; k++) H[k] = M[k] = W[k] = 0;
        for (long rb0 = rs; rb0 < re; rb0 += ROH_BATCH) {
            uint32_t x[ROH_BATCH];
#pragma unroll
            for (int u = 0; u < ROH_BATCH; u++) {
                x[u] = 0;
                const long r = rb0 + u;
                if (live && r < re) {
                    const long row = (SRC == 1 && offs) ? offs[r - g0] : r - g0;
                    const uint8_t* p = src + row * stride + col;
                    x[u] = SRC == 0 ? __builtin_nontemporal_load((const uint32_t*)p) : (uint32_t)__builtin_nontemporal_load(p);
                }
            }
#pragma unroll
            for (int u = 0; u < ROH_BATCH; u++) {
                const long r = rb0 + u;
                if (r >= re) break;
                const bool full = r - (w - 1) >= rs;       // the window that ends at r lies inside the rows read of this block
#pragma unroll
                for (int k = 0; k < ROH_IPL; k++) {
                    uint64_t hb, mb;
                    if (SRC == 0) {
                        hb = ((x[u] >> (8 * k)) & 0xffu) == 0u;
                        mb = 0;
                    } else {
                        const uint32_t c = (x[u] >> (2 * k)) & 3u;
                        hb = c == 2u;
                        mb = c == 1u;
                    }
                    H[k] = (H[k] << 1) | hb;
                    M[k] = (M[k] << 1) | mb;
                    const bool homw = full && __popcll(H[k] & wm) <= R.win_het && __popcll(M[k] & wm) <= R.win_miss;
                    W[k] = (W[k] << 1) | (uint64_t)homw;
                }
                // markers decided by this row: j = r - (w - 1), and at the block's last row every marker from there on
                long jlo = r - (w - 1), jhi = r == e - 1 ? r : jlo;
                if (jlo < a) jlo = a;
                if (jlo < m0) jlo = m0;
                if (jhi >= m1) jhi = m1 - 1;
                for (long j = jlo; j <= jhi; j++) {
                    const int t = (int)(r - j);
                    const uint64_t bm = roh_low_bits(t + 1);
                    const long s_lo = a > j - (w - 1) ? a : j - (w - 1), s_hi = j < e - w ? j : e - w;
                    const int cover = s_hi >= s_lo ? (int)(s_hi - s_lo + 1) : 0;
                    uint64_t bf[ROH_IPL], bh[ROH_IPL], bmi[ROH_IPL];
#pragma unroll
                    for (int k = 0; k < ROH_IPL; k++) {
                        const int hom = __popcll(W[k] & bm);
                        bf[k] = __ballot(hom >= 1 && hom * 65536 >= R.thr16 * cover);
                        bh[k] = __ballot((int)((H[k] >> t) & 1ull));
                        bmi[k] = SRC == 1 ? __ballot((int)((M[k] >> t) & 1ull)) : 0ull;
                    }
                    if (storer) {
                        uint64_t vf = 0, vh = 0, vm = 0;
#pragma unroll
                        for (int q = 0; q < 4; q++)
                            if (lane == q) {
                                vf = roh_word(bf, q);
                                vh = roh_word(bh, q);
                                vm = SRC == 1 ? roh_word(bmi, q) : 0ull;
                            }
                        flagged[j * nw + wq] = vf & keep;
                        het[j * nw + wq] = vh & keep;
                        miss[j * nw + wq] = vm & keep;
                    }
                }
            }
        }
    }
}

__device__ __forceinline__ uint64_t roh_bcast64(uint64_t v, int t) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, t), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), t);
    return ((uint64_t)hi << 32) | lo;
}

// blockIdx.x = block ordinal * nw + word.  cnt / offs: n x nb by (individual, block).  ind: n x 4 (zeroed by the caller before the count
// pass).  seg: rows of six int32.
template <bool FILL>
__global__ __launch_bounds__(64) void k_roh_segments(const uint64_t* __restrict__ flagged, const uint64_t* __restrict__ het,
                                                     const uint64_t* __restrict__ miss, long nw, long n, const int32_t* __restrict__ blk, int nb,
                                                     const int64_t* __restrict__ pos, RohSegRule P, int32_t* __restrict__ cnt,
                                                     unsigned long long* __restrict__ ind, const int64_t* __restrict__ offs,
                                                     int32_t* __restrict__ seg) {
    const long b = (long)blockIdx.x / nw, wq = (long)blockIdx.x - b * nw;
    const int lane = threadIdx.x;
    const long i = 64 * wq + lane;
    const long a = blk[b], e = blk[b + 1];
    bool in_run = false;
    long s = 0, pos_s = 0, prev_pos = 0;
    int nhet = 0, nmiss = 0;
    int count = 0;
    long sum_snp = 0, sum_len = 0, longest = 0;
    long out = (FILL && i < n) ? offs[i * nb + b] : 0;

    auto close_run = [&](long last, long pos_last) {   // the run s .. last ends
        const long nsnp = last - s + 1, len = pos_last - pos_s;
        const bool ok = nsnp >= P.min_snp && len >= P.min_len && (P.max_density == 0 || len <= P.max_density * nsnp) &&
                        (P.max_het < 0 || (long)nhet <= P.max_het);
        if (ok) {
            if (FILL) {
                int32_t* row = seg + 6 * out;
                row[0] = (int32_t)i; row[1] = (int32_t)s; row[2] = (int32_t)last; row[3] = nhet; row[4] = nmiss; row[5] = (int32_t)b;
                out++;
            } else {
                count++;
                sum_snp += nsnp;
                sum_len += len;
                if (len > longest) longest = len;
            }
        }
        in_run = false;
    };

    for (long mb = a; mb < e; mb += 64) {
        const long mine = mb + lane;
        uint64_t fw = 0, hw = 0, mw = 0;
        long pw = mine;
        if (mine < e) {
            fw = flagged[mine * nw + wq];
            hw = het[mine * nw + wq];
            mw = miss[mine * nw + wq];
            if (pos) pw = pos[mine];
        }
        const int cntm = e - mb < 64 ? (int)(e - mb) : 64;
        for (int t = 0; t < cntm; t++) {
            const long m = mb + t;
            const bool f = (roh_bcast64(fw, t) >> lane) & 1ull;
            const int hb = (int)((roh_bcast64(hw, t) >> lane) & 1ull), mbit = (int)((roh_bcast64(mw, t) >> lane) & 1ull);
            const long p = (long)roh_bcast64((uint64_t)pw, t);
            const bool gap = P.max_gap > 0 && m > a && p - prev_pos > P.max_gap;
            if (in_run && (gap || !f)) close_run(m - 1, prev_pos);
            if (f) {
                if (!in_run) { in_run = true; s = m; pos_s = p; nhet = 0; nmiss = 0; }
                nhet += hb;
                nmiss += mbit;
            }
            prev_pos = p;
        }
    }
    if (in_run) close_run(e - 1, prev_pos);
    if (!FILL && i < n) {
        cnt[i * nb + b] = count;
        if (count) {
            atomicAdd(ind + 4 * i + 0, (unsigned long long)count);
            atomicAdd(ind + 4 * i + 1, (unsigned long long)sum_snp);
            atomicAdd(ind + 4 * i + 2, (unsigned long long)sum_len);
            atomicMax(ind + 4 * i + 3, (unsigned long long)longest);
        }
    }
}

static int roh_rule(eagle_ctx* ctx, const eagle_roh_params* p, RohRule* r) {
    if (p->w < 1 || p->w > 64 || p->thr16 < 0 || p->thr16 > 65536 || p->win_het < 0 || p->win_miss < 0)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "roh_flags: bad window rule");
    r->w = (int)p->w;
    r->win_het = (int)(p->win_het > 64 ? 64 : p->win_het);
    r->win_miss = (int)(p->win_miss > 64 ? 64 : p->win_miss);
    r->thr16 = (int)p->thr16;
    return EAGLE_OK;
}

static int roh_flags_launch(eagle_ctx* ctx, int src_kind, const uint8_t* src, long stride, const long* offs, long n, long g0, long c0, long c1,
                            const int32_t* blk, long nb, const RohRule& R, uint64_t* planes, long markers, void* stream) {
    if (c1 <= c0) return EAGLE_OK;
    if (n <= 0 || c0 < 0 || c1 > markers || nb < 1 || nb > 0x7fffffffL || markers > 0x7fffffffL)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "roh_flags: bad shape");
    const long nw = (n + 63) / 64, groups = (n + 255) / 256, chunks = (c1 - c0 + EAGLE_ROH_CHUNK - 1) / EAGLE_ROH_CHUNK;
    if (groups * chunks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "roh_flags: too many individuals x markers for one launch");
    uint64_t* pf = planes;
    uint64_t* ph = planes + (size_t)markers * (size_t)nw;
    uint64_t* pm = ph + (size_t)markers * (size_t)nw;
    const dim3 grid((unsigned)(groups * chunks)), blkdim(64);
    hipStream_t s = (hipStream_t)stream;
    if (src_kind == 0)
        hipLaunchKernelGGL(k_roh_flags<0>, grid, blkdim, 0, s, src, stride, offs, n, g0, c0, c1, blk, (int)nb, R, nw, groups, pf, ph, pm);
    else
        hipLaunchKernelGGL(k_roh_flags<1>, grid, blkdim, 0, s, src, stride, offs, n, g0, c0, c1, blk, (int)nb, R, nw, groups, pf, ph, pm);
    ROH_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// The planes' rows of the panel markers [c0, c1) from an int8 Mt image whose row 0 is panel marker g0 and which holds the markers
// [max(0, c0 - (w - 1)), min(markers, c1 + w - 1)) at least.  planes: 3 x markers x ceil(n / 64) uint64 (flagged, het, miss).
extern "C" int eagle_dev_roh_flags_i8(eagle_ctx* ctx, const int8_t* Mt8, long ld, long n, long g0, long c0, long c1, const int32_t* blk, long nb,
                                      const eagle_roh_params* prm, uint64_t* planes, long markers, void* stream) {
    RohRule R;
    if (int rc = roh_rule(ctx, prm, &R)) return rc;
    if (n > ld || ld % 16 || ((uintptr_t)Mt8 & 15)) return eagle_fail(ctx, EAGLE_ERR_ARG, "roh_flags: bad image shape");
    return roh_flags_launch(ctx, 0, (const uint8_t*)Mt8, ld, nullptr, n, g0, c0, c1, blk, nb, R, planes, markers, stream);
}

// The same from raw .bed rows: the row of panel marker g0 + p is row offsets[p] of `bed` (offsets null: row p), checked by the CALLER.
extern "C" int eagle_dev_roh_flags_bed(eagle_ctx* ctx, const uint8_t* bed, const long* offsets, long n, long g0, long c0, long c1,
                                       const int32_t* blk, long nb, const eagle_roh_params* prm, uint64_t* planes, long markers, void* stream) {
    RohRule R;
    if (int rc = roh_rule(ctx, prm, &R)) return rc;
    if (n > 0x3fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "roh_flags: bad shape");
    return roh_flags_launch(ctx, 1, bed, bed_row_bytes(n), offsets, n, g0, c0, c1, blk, nb, R, planes, markers, stream);
}

// fill == 0: cnt (n x nb) written, ind (n x 4, zeroed by the caller) added to; fill != 0: the rows of seg from offs (n x nb).
extern "C" int eagle_dev_roh_segments(eagle_ctx* ctx, const uint64_t* planes, long markers, long n, const int32_t* blk, long nb, const int64_t* pos,
                                      const eagle_roh_params* prm, int fill, int32_t* cnt, int64_t* ind, const int64_t* offs, int32_t* seg,
                                      void* stream) {
    if (n <= 0 || markers <= 0 || nb < 1) return eagle_fail(ctx, EAGLE_ERR_ARG, "roh_segments: bad shape");
    const long nw = (n + 63) / 64;
    if (nw * nb > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "roh_segments: too many individuals x blocks for one launch");
    const RohSegRule P = {prm->min_snp, prm->min_len, prm->max_gap, prm->max_density, prm->max_het};
    const uint64_t* pf = planes;
    const uint64_t* ph = planes + (size_t)markers * (size_t)nw;
    const uint64_t* pm = ph + (size_t)markers * (size_t)nw;
    const dim3 grid((unsigned)(nw * nb)), blkdim(64);
    hipStream_t s = (hipStream_t)stream;
    if (fill)
        hipLaunchKernelGGL(k_roh_segments<true>, grid, blkdim, 0, s, pf, ph, pm, nw, n, blk, (int)nb, pos, P, cnt, (unsigned long long*)ind, offs, seg);
    else
        hipLaunchKernelGGL(k_roh_segments<false>, grid, blkdim, 0, s, pf, ph, pm, nw, n, blk, (int)nb, pos, P, cnt, (unsigned long long*)ind, offs, seg);
    ROH_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}
