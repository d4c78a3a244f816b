// eagle_ld.hip -- linkage disequilibrium between markers: integer dot products between rows of the int8 marker-major image on the int8
// MFMA (v_mfma_i32_32x32x32_i8), in three modes of one tile kernel.  Every number below is an exact integer until the one fp64 test.
//
//   s_i = sum g, q_i = sum g^2 (from k_marker_counts: s = n2 - n0, q = n2 + n0), d_ij = sum g_i g_j (int32, the MFMA),
//   c_ij = n d_ij - s_i s_j, v_i = n q_i - s_i^2 (int64);  r^2_ij = c^2 / (v_i v_j).
//   i, j are IN LD AT t  iff  v_i > 0, v_j > 0 and (double)c * (double)c > t * ((double)v_i * (double)v_j), evaluated in that order:
//   products only, so nothing contracts to an FMA and the host restatement gives the same bits.
//
//   band mode (k_ld_tile<NB, false>) ... bit o - 1 of mask[i] is set iff markers i and i + o (1 <= o <= window <= 256, i + o < rows) are
//                                        in LD at t; mask is rows x ceil(window / 64) uint64 words.
//   picks mode (k_ld_tile<2, true>) .... dots[i][j] = d between marker i and row j of a gathered image B8 of k <= 64 rows (64 x ld, zero rows
//                                        beyond k; k_gather_rows_i8 makes it), int32 rows x k.
//
//   r2 mode (k_ld_tile<NB, false, true>) band[i * window + o - 1] = r^2 between markers i and i + o as an fp64 number,
//                                        fl(fl((double)c * (double)c) / fl((double)v_i * (double)v_j)), or -1.0 where i + o >= rows or one of
//                                        the two is monomorphic: the band mode's tile with another epilogue.  k_ld_partners then ranks, per
//                                        marker, its forward entries and the backward entries of the `window` markers before it (include/
//                                        eagle_hip.h section 1b'''iii); k_ld_reduce sums them all, quantised to integers, per marker and
//                                        per distance bin (section 1b'''v).
//
// Tile.  A workgroup (256 threads, 4 waves) owns TM = 128 consecutive markers.  Per K chunk of 128 individuals it stages TB rows x 128 B
// in LDS once: in band mode TB = 128 + 32 (NB - 1) rows of the SAME image from the tile's first row on, NB - 1 = pad32(window) / 32, so that
// the A operand is simply the first 128 rows of what was staged for B; in picks mode rows 128 .. 191 are B8.  Wave w multiplies the 32-row
// block w of A against NB blocks of B: blocks w .. w + NB - 1 in band mode -- block pairs (a, b) hold offsets j - i in
// [32 (b - a) - 31, 32 (b - a) + 31], which meet (0, window] exactly for 0 <= b - a <= floor((window + 31) / 32) = NB - 1 -- and blocks
// 4, 5 in picks mode.  Accumulators: NB blocks of 16 int32 registers per lane, at most 9 x 16 = 144 for window 225 .. 256 (36 blocks of the
// 4 x 12 block grid, 9 per wave); the staging registers of the next chunk add TB / 32 <= 12 x 4.  One wave per SIMD has 512 registers.
//
// Loads: plain 16-byte global loads into registers, issued for chunk c + 1 before the MFMAs of chunk c and written to LDS after them
// (the staged reader of eagle_t8.h moves fixed 256-row tiles of images whose ld is a multiple of 128; this tile has 160 .. 384 rows, rows
// beyond the image that must not be read, and a second source in picks mode).  LDS rows are 128 B = 8 chunks of 16 B, logical chunk c of
// row r at physical chunk c ^ ((r >> 1) & 7): the swizzle of the tile engine, under which the ds_read_b128 operand reads of 32 rows x one
// logical chunk are free of bank conflicts.  Rows at or beyond `rows` and bytes at or beyond ceil16(n) are staged as zeros, never read.
//
// Epilogue (band): s and v of the TB markers go to LDS (over the dead tile), every accumulator element inside the band takes the test and
// ORs its bit into the tile's mask words in LDS; after a barrier the words leave by plain 8-byte vector stores.  Every word of `mask` has
// one owning workgroup: no global atomics, a deterministic result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

typedef int ld_i32x4 __attribute__((ext_vector_type(4)));
typedef int ld_i32x16 __attribute__((ext_vector_type(16)));

#define LD_TM 128   /* markers per workgroup */
#define LD_BK 128   /* individuals (bytes of a row) per staged chunk */

#define LD_LAUNCH_CHECK(ctx)                                                \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

// sq[r] = (s, q) of marker r from counts[r] = (n0, n1, n2)
__global__ __launch_bounds__(256) void k_ld_sq(const int32_t* __restrict__ counts, long rows, int32_t* __restrict__ sq) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int n0 = counts[3 * r], n2 = counts[3 * r + 2];
    sq[2 * r] = n2 - n0;
    sq[2 * r + 1] = n2 + n0;
}

// kbytes = ceil16(n): the bytes of a row that hold individuals (the image is zero from n on).  B8 / ldB / k / dots: picks mode only;
// sq / window: band and r2 mode; t / mask / wpr: band mode only; band: r2 mode only (rows x window fp64).
template <int NB, bool PICKS, bool R2 = false>
__global__ __launch_bounds__(256) void k_ld_tile(const int8_t* __restrict__ Mt8, long rows, long n, long ld, long kbytes,
                                                 const int8_t* __restrict__ B8, long ldB, int k, const int32_t* __restrict__ sq, int window,
                                                 double t, uint64_t* __restrict__ mask, int wpr, int32_t* __restrict__ dots,
                                                 double* __restrict__ band) {
    constexpr int TB = PICKS ? LD_TM + 32 * NB : LD_TM + 32 * (NB - 1);
    constexpr int NCH = TB / 32;   // 16-byte pieces per thread and chunk: TB * 8 / 256
    __shared__ __attribute__((aligned(16))) int8_t tile[TB * LD_BK];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const long row0 = (long)blockIdx.x * LD_TM;

    ld_i32x4 pre[NCH];
    auto fetch = [&](long k0) {
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int idx = tid + 256 * i, rr = idx >> 3;
            const long kb = k0 + 16 * (idx & 7);
            ld_i32x4 v = {0, 0, 0, 0};
            if (kb < kbytes) {
                if (PICKS && rr >= LD_TM) v = *(const ld_i32x4*)(B8 + (long)(rr - LD_TM) * ldB + kb);
                else if (row0 + rr < rows) v = *(const ld_i32x4*)(Mt8 + (row0 + rr) * ld + kb);
            }
            pre[i] = v;
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int idx = tid + 256 * i, rr = idx >> 3, c = idx & 7;
            *(ld_i32x4*)(tile + rr * LD_BK + ((c ^ ((rr >> 1) & 7)) << 4)) = pre[i];
        }
    };

    ld_i32x16 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[b][e] = 0;

    const int8_t* pa = tile + (32 * w + r) * LD_BK;
    const int8_t* pb = tile + ((PICKS ? LD_TM : 32 * w) + r) * LD_BK;
    const int swz = (r >> 1) & 7;

    fetch(0);
    for (long k0 = 0; k0 < kbytes; k0 += LD_BK) {
        put();
        __syncthreads();
        if (k0 + LD_BK < kbytes) fetch(k0 + LD_BK);
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
            const int ch = ((2 * ks + h) ^ swz) << 4;
            const ld_i32x4 a = *(const ld_i32x4*)(pa + ch);
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const ld_i32x4 bb = *(const ld_i32x4*)(pb + b * (32 * LD_BK) + ch);
                acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bb, acc[b], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // accumulator element e of block b: marker i = 32 w + (e & 3) + 8 (e >> 2) + 4 h of the tile (the A row), j = lane & 31 of the B block
    if (PICKS) {
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const int j = 32 * b + r;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const long gi = row0 + 32 * w + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (j < k && gi < rows) dots[gi * k + j] = acc[b][e];
            }
        }
        return;
    }

    int* sS = (int*)tile;                              // TB x int32 s
    long long* sV = (long long*)(tile + TB * 4);       // TB x int64 v (TB * 4 is a multiple of 8)
    unsigned* sM = (unsigned*)(tile + TB * 12);        // 128 rows x 8 half words of the mask
    for (int x = tid; x < TB; x += 256) {
        const long g = row0 + x;
        int s = 0;
        long long v = 0;
        if (g < rows) {
            s = sq[2 * g];
            v = (long long)n * sq[2 * g + 1] - (long long)s * s;
        }
        sS[x] = s;
        sV[x] = v;
    }
    if (!R2)
        for (int x = tid; x < LD_TM * 8; x += 256) sM[x] = 0u;
    __syncthreads();
    if (R2) {
        // every (i, o), i < rows, 1 <= o <= window, lies in exactly one block pair: each entry of the band is written once, by the 32
        // lanes of a half wave as 32 consecutive doubles (o = jl - il runs with the lane)
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const int jl = 32 * (w + b) + r;
            const int sj = sS[jl];
            const long long vj = sV[jl];
            const bool jok = row0 + jl < rows && vj > 0;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int il = 32 * w + (e & 3) + 8 * (e >> 2) + 4 * h, o = jl - il;
                const long gi = row0 + il;
                if (o < 1 || o > window || gi >= rows) continue;
                const long long vi = sV[il];
                double val = -1.0;
                if (jok && vi > 0) {
                    const long long c = (long long)n * acc[b][e] - (long long)sS[il] * sj;
                    const double dc = (double)c;
                    val = (dc * dc) / ((double)vi * (double)vj);
                }
                band[gi * window + (o - 1)] = val;
            }
        }
        return;
    }
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const int jl = 32 * (w + b) + r;
        const int sj = sS[jl];
        const long long vj = sV[jl];
        const bool jok = row0 + jl < rows && vj > 0;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int il = 32 * w + (e & 3) + 8 * (e >> 2) + 4 * h, o = jl - il;
            if (!jok || o < 1 || o > window) continue;
            const long long vi = sV[il];
            if (vi <= 0) continue;
            const long long c = (long long)n * acc[b][e] - (long long)sS[il] * sj;
            const double dc = (double)c;
            if (dc * dc > t * ((double)vi * (double)vj)) atomicOr(&sM[il * 8 + ((o - 1) >> 5)], 1u << ((o - 1) & 31));
        }
    }
    __syncthreads();
    for (int x = tid; x < LD_TM * wpr; x += 256) {
        const int il = x / wpr, wd = x - il * wpr;
        const long gi = row0 + il;
        if (gi < rows) mask[gi * wpr + wd] = (uint64_t)sM[il * 8 + 2 * wd] | ((uint64_t)sM[il * 8 + 2 * wd + 1] << 32);
    }
}

static bool ld_bad_image(const int8_t* Mt8, long n, long ld) {
    return n <= 0 || n > ld || ld % 16 || ((uintptr_t)Mt8 & 15) || n > 0x3fffffffL;
}

extern "C" int eagle_dev_ld_sq(eagle_ctx* ctx, const int32_t* counts, long rows, int32_t* sq, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    const long blocks = (rows + 255) / 256;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "ld_sq: too many rows");
    hipLaunchKernelGGL(k_ld_sq, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, counts, rows, sq);
    LD_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

extern "C" int eagle_dev_ld_band(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, const int32_t* sq, long window, double t,
                                 uint64_t* mask, long words_per_row, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (ld_bad_image(Mt8, n, ld)) return eagle_fail(ctx, EAGLE_ERR_ARG, "ld_band: bad image shape");
    if (window < 1 || window > 256 || words_per_row != (window + 63) / 64 || !(t >= 0.0 && t <= 1.0))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "ld_band: bad window, threshold or mask width");
    const long blocks = (rows + LD_TM - 1) / LD_TM;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "ld_band: too many rows");
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t s = (hipStream_t)stream;
    const long kbytes = (n + 15) / 16 * 16;
    const int nb = (int)((window + 31) / 32) + 1;
#define LD_BAND_CASE(NB)                                                                                                              \
    case NB:                                                                                                                          \
        hipLaunchKernelGGL((k_ld_tile<NB, false>), grid, blk, 0, s, Mt8, rows, n, ld, kbytes, (const int8_t*)nullptr, 0L, 0, sq, (int)window, \
                           t, mask, (int)words_per_row, (int32_t*)nullptr, (double*)nullptr);                                         \
        break;
    switch (nb) {
        LD_BAND_CASE(2) LD_BAND_CASE(3) LD_BAND_CASE(4) LD_BAND_CASE(5) LD_BAND_CASE(6) LD_BAND_CASE(7) LD_BAND_CASE(8) LD_BAND_CASE(9)
    }
#undef LD_BAND_CASE
    LD_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// B8: 64 rows x ld (the leading dimension of Mt8), rows k .. 63 zero
extern "C" int eagle_dev_ld_dots(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, const int8_t* B8, long k, int32_t* dots,
                                 void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (ld_bad_image(Mt8, n, ld) || ((uintptr_t)B8 & 15)) return eagle_fail(ctx, EAGLE_ERR_ARG, "ld_dots: bad image shape");
    if (k < 1 || k > 64) return eagle_fail(ctx, EAGLE_ERR_ARG, "ld_dots: 1 to 64 loci");
    const long blocks = (rows + LD_TM - 1) / LD_TM;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "ld_dots: too many rows");
    hipLaunchKernelGGL((k_ld_tile<2, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, Mt8, rows, n, ld, (n + 15) / 16 * 16,
                       B8, ld, (int)k, (const int32_t*)nullptr, 0, 0.0, (uint64_t*)nullptr, 0, dots, (double*)nullptr);
    LD_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// ranked partner lists (include/eagle_hip.h section 1b'''iii)
// ------------------------------------------------------------------------------------------------------------------------------
// One wave per marker i of [c_lo, c_hi) (rows of `band`, whose row 0 is marker g0 of the panel).  Candidate t = 2 (|o| - 1) + (o > 0),
// 0 <= t < 2 window, is marker j = i + o: t is the rank of a tie in r^2 (the smaller |j - i|, then the smaller j).  Lane x holds the
// candidates t = x, x + 64, ... (at most 8) in registers: the forward entry band[i][o - 1], or the backward entry band[j][|o| - 1] of
// the marker before it.  l rounds of a wave-wide maximum of (r^2, then the smaller t) write the list in order; the winner's owner
// retires it.  Lane 0 stores: every word of partners / r2 has one owner.
__global__ __launch_bounds__(256) void k_ld_partners(const double* __restrict__ band, long rows, int window, long c_lo, long c_hi, long g0,
                                                     const int32_t* __restrict__ chrom, double min_r2, int l, int32_t* __restrict__ partners,
                                                     double* __restrict__ r2) {
    const int lane = threadIdx.x & 63;
    const long i = c_lo + (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= c_hi) return;                                          // a whole wave: the shuffles below see all 64 lanes or none
    const long gi = g0 + i;
    const int ci = chrom ? chrom[gi] : 0;
    double val[8];
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const int t = lane + 64 * s, o = (t >> 1) + 1;
        val[s] = -1.0;
        if (t < 2 * window) {
            const long j = (t & 1) ? i + o : i - o;
            if (j >= 0 && j < rows) {
                const double v = (t & 1) ? band[i * window + (o - 1)] : band[j * window + (o - 1)];
                if (v >= min_r2 && (!chrom || chrom[g0 + j] == ci)) val[s] = v;      // -1.0 (no pair, monomorphic) is below every min_r2
            }
        }
    }
    int32_t* prow = partners + gi * l;
    double* rrow = r2 + gi * l;
    int t = 0;
    for (; t < l; t++) {
        double best = -1.0;
        int bt = 0x7fffffff;
#pragma unroll
        for (int s = 0; s < 8; s++)
            if (val[s] > best) { best = val[s]; bt = lane + 64 * s; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ob = __shfl_xor(best, off);
            const int ot = __shfl_xor(bt, off);
            if (ob > best || (ob == best && ot < bt)) { best = ob; bt = ot; }
        }
        if (best < 0.0) break;                                      // the same value in every lane
        if (lane == 0) {
            const int o = (bt >> 1) + 1;
            prow[t] = (int32_t)(gi + ((bt & 1) ? o : -o));
            rrow[t] = best;
        }
#pragma unroll
        for (int s = 0; s < 8; s++)
            if (bt == lane + 64 * s) val[s] = -1.0;
    }
    for (int x = t + lane; x < l; x += 64) {
        prow[x] = -1;
        rrow[x] = 0.0;
    }
}

// band: rows x window fp64, every entry written
extern "C" int eagle_dev_ld_r2band(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, const int32_t* sq, long window, double* band,
                                   void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (ld_bad_image(Mt8, n, ld)) return eagle_fail(ctx, EAGLE_ERR_ARG, "ld_r2band: bad image shape");
    if (window < 1 || window > 256) return eagle_fail(ctx, EAGLE_ERR_ARG, "ld_r2band: bad window");
    const long blocks = (rows + LD_TM - 1) / LD_TM;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "ld_r2band: too many rows");
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t s = (hipStream_t)stream;
    const long kbytes = (n + 15) / 16 * 16;
    const int nb = (int)((window + 31) / 32) + 1;
#define LD_R2_CASE(NB)                                                                                                                \
    case NB:                                                                                                                          \
        hipLaunchKernelGGL((k_ld_tile<NB, false, true>), grid, blk, 0, s, Mt8, rows, n, ld, kbytes, (const int8_t*)nullptr, 0L, 0, sq, \
                           (int)window, 0.0, (uint64_t*)nullptr, 0, (int32_t*)nullptr, band);                                          \
        break;
    switch (nb) {
        LD_R2_CASE(2) LD_R2_CASE(3) LD_R2_CASE(4) LD_R2_CASE(5) LD_R2_CASE(6) LD_R2_CASE(7) LD_R2_CASE(8) LD_R2_CASE(9)
    }
#undef LD_R2_CASE
    LD_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// partners / r2: rows of l entries indexed by the PANEL's marker, of which the rows g0 + [c_lo, c_hi) are written; chrom: by the panel's
// marker, or null
extern "C" int eagle_dev_ld_partners(eagle_ctx* ctx, const double* band, long rows, long window, long c_lo, long c_hi, long g0, const int32_t* chrom,
                                     double min_r2, int l, int32_t* partners, double* r2, void* stream) {
    if (c_hi <= c_lo) return EAGLE_OK;
    if (c_lo < 0 || c_hi > rows || window < 1 || window > 256 || l < 1 || l > EAGLE_LDKNN_MAX_PARTNERS || !(min_r2 >= 0.0 && min_r2 <= 1.0))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "ld_partners: bad shape");
    const long blocks = (c_hi - c_lo + 3) / 4;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "ld_partners: too many rows");
    hipLaunchKernelGGL(k_ld_partners, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, band, rows, (int)window, c_lo, c_hi, g0, chrom, min_r2,
                       l, partners, r2);
    LD_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// LD scores and the LD decay curve (include/eagle_hip.h section 1b'''v)
// ------------------------------------------------------------------------------------------------------------------------------
#define LD_REDUCE_MAX_BINS 512
#define LD_REDUCE_MAX_BLOCKS 2048   /* 8 workgroups of 4 waves on each of 256 compute units: what bounds the flush below */

// k_ld_partners' shape: one wave per marker i of [c_lo, c_hi), lane x holds the candidates t = x, x + 64, ... (at most 8), the forward
// entry band[i][o - 1] or the backward entry band[j][|o| - 1].  Every eligible candidate adds u = (uint64)(r2 * 2^30) and 1 to the lane's
// totals; a wave-wide integer sum gives U and cnt, lane 0 stores them: every word has one owner.  FORWARD candidates alone (the pair
// belongs to its smaller marker, and that marker to one core) also add u and 1 to the bin of their distance in the workgroup's
// histogram in LDS (64-bit integer LDS atomics; the edges sit in LDS too, the bin is found by binary search).  A workgroup walks its
// markers with the grid's stride -- at most LD_REDUCE_MAX_BLOCKS workgroups, however long the core -- and adds its non-zero bins to the
// global histogram once, after a barrier, with 64-bit vector atomic adds: consecutive lanes add consecutive words, at most 2,048 x 512
// x 2 adds of 8 bytes per launch (16 MiB of added bytes whatever L is; every workgroup adds into the same two arrays of at most 4 KB,
// and the rate of 64-bit integer adds under that contention has not been measured), and integer adds in any order give one result.
// A wave without a marker skips the work and still meets the barrier.
__global__ __launch_bounds__(256) void k_ld_reduce(const double* __restrict__ band, long rows, int window, long c_lo, long c_hi, long g0,
                                                   const int32_t* __restrict__ chrom, const int64_t* __restrict__ pos, long max_dist,
                                                   const int64_t* __restrict__ edges, int nbins, unsigned long long* __restrict__ U,
                                                   int32_t* __restrict__ cnt, unsigned long long* __restrict__ bin_sum,
                                                   unsigned long long* __restrict__ bin_pairs) {
    __shared__ unsigned long long hS[LD_REDUCE_MAX_BINS], hP[LD_REDUCE_MAX_BINS];
    __shared__ long long eS[LD_REDUCE_MAX_BINS + 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int x = tid; x < nbins; x += 256) hS[x] = hP[x] = 0ull;
    for (int x = tid; x <= nbins && nbins > 0; x += 256) eS[x] = edges[x];
    __syncthreads();
    const long groups = (c_hi - c_lo + 3) / 4;
    for (long g = blockIdx.x; g < groups; g += gridDim.x) {         // the same trip count in every wave of the workgroup
        const long i = c_lo + 4 * g + w;
        if (i >= c_hi) continue;                                    // a whole wave: the shuffles below see all 64 lanes or none
        const long gi = g0 + i;
        const int ci = chrom ? chrom[gi] : 0;
        const long long pi = pos ? pos[gi] : 0;
        unsigned long long usum = 0ull;
        int c = 0;
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const int t = lane + 64 * s, o = (t >> 1) + 1;
            if (t >= 2 * window) continue;
            const long j = (t & 1) ? i + o : i - o;
            if (j < 0 || j >= rows) continue;
            const double v = (t & 1) ? band[i * window + (o - 1)] : band[j * window + (o - 1)];
            if (!(v >= 0.0) || (chrom && chrom[g0 + j] != ci)) continue;         // -1.0: no pair
            long long d = o;
            if (pos) {
                const long long pj = pos[g0 + j];
                d = pj > pi ? pj - pi : pi - pj;
                if (max_dist > 0 && d > max_dist) continue;
            }
            const unsigned long long u = (unsigned long long)(v * 1073741824.0);   // exact product, truncating conversion
            usum += u;
            c++;
            if ((t & 1) && nbins > 0 && d >= eS[0] && d < eS[nbins]) {
                int lo = 0, hi = nbins;                             // eS[lo] <= d < eS[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (d >= eS[mid]) lo = mid;
                    else hi = mid;
                }
                atomicAdd(&hS[lo], u);
                atomicAdd(&hP[lo], 1ull);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            usum += __shfl_xor(usum, off);
            c += __shfl_xor(c, off);
        }
        if (lane == 0) {
            U[gi] = usum;
            cnt[gi] = c;
        }
    }
    __syncthreads();
    for (int x = tid; x < nbins; x += 256) {
        if (!hP[x]) continue;                                       // no pair, no sum
        atomicAdd(&bin_pairs[x], hP[x]);
        if (hS[x]) atomicAdd(&bin_sum[x], hS[x]);
    }
}

// U / cnt: by the PANEL's marker, of which the entries g0 + [c_lo, c_hi) are written; chrom / pos: by the panel's marker, or null;
// edges (nbins + 1 int64, increasing) / bin_sum / bin_pairs (nbins words each, ADDED to): device memory, unused when nbins == 0
extern "C" int eagle_dev_ld_reduce(eagle_ctx* ctx, const double* band, long rows, long window, long c_lo, long c_hi, long g0, const int32_t* chrom,
                                   const int64_t* pos, long max_dist, const int64_t* edges, int nbins, uint64_t* U, int32_t* cnt,
                                   uint64_t* bin_sum, int64_t* bin_pairs, void* stream) {
    if (c_hi <= c_lo) return EAGLE_OK;
    if (c_lo < 0 || c_hi > rows || window < 1 || window > 256 || nbins < 0 || nbins > LD_REDUCE_MAX_BINS || !band || !U || !cnt ||
        (nbins > 0 && (!edges || !bin_sum || !bin_pairs)) || (max_dist > 0 && !pos))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "ld_reduce: bad shape");
    const long groups = (c_hi - c_lo + 3) / 4;
    const long blocks = groups < LD_REDUCE_MAX_BLOCKS ? groups : LD_REDUCE_MAX_BLOCKS;
    hipLaunchKernelGGL(k_ld_reduce, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, band, rows, (int)window, c_lo, c_hi, g0, chrom, pos,
                       max_dist, edges, nbins, (unsigned long long*)U, cnt, (unsigned long long*)bin_sum, (unsigned long long*)bin_pairs);
    LD_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}
