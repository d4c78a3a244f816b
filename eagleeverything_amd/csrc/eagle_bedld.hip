// eagle_bedld.hip -- pairwise-complete linkage disequilibrium between markers from the rows of a PLINK .bed file (include/eagle_hip.h
// section 1b'''iv): eagle_ld.hip's band tile for a file in which the missing code is still known.  Every number is an exact integer
// until the one fp64 test or quotient.
//
//   Per genotype x = -1, 0, 0, +1 for the codes 0, 1, 2, 3, c = [code != 1], u = |x|.  For markers i != j six int32 sums over the
//   individuals:  N = sum c_i c_j,  D = sum x_i x_j,  Si = sum x_i c_j,  Sj = sum c_i x_j,  Qi = sum u_i c_j,  Qj = sum c_i u_j;  in
//   int64 cov = N D - Si Sj, vi = N Qi - Si^2, vj = N Qj - Sj^2.  COMPARABLE iff N >= min_overlap, vi > 0, vj > 0; then IN LD AT t iff
//   (double)cov * (double)cov > t * ((double)vi * (double)vj), and r2 = fl(fl(dc * dc) / fl(dvi * dvj)): products and one quotient, so
//   nothing contracts to an FMA and the host restatement gives the same bits.
//
// k_bed_ld_pack.  The included rows of a staged window of .bed rows become three marker-major int8 images X, C, U (one row per panel
// marker of the window, rows compacted in panel order, leading dimension a multiple of 16, zero at and beyond individual n: the pad bit
// pairs of a row's last byte are masked by the individual's index, whatever they hold).  One thread per 16 individuals of a marker: four
// bytes of the row in, three 16-byte stores out.
//
// k_bedld_tile<NB, R2>.  k_ld_tile's geometry: a workgroup (256 threads, 4 waves) owns TM = 128 consecutive panel markers, K chunks of 128
// individuals, LDS rows of 128 B with logical 16-byte chunk c of row r at physical chunk c ^ ((r >> 1) & 7), v_mfma_i32_32x32x32_i8.
// Wave w multiplies the 32-row block w of the tile (A) against the blocks w + o, 0 <= o < NB = floor((window + 31) / 32) + 1 (B), and per
// block pair six of the nine products of the three images: X.X (D), X.C (Si), C.X (Sj), C.C (N), U.C (Qi), C.U (Qj).
//   Registers set the shape.  Six products x 16 int32 x NB = 864 accumulator registers per lane at NB = 9; one wave per SIMD has 512.
//   The block offsets are therefore walked in GROUPS of at most 2 (192 accumulator registers; the 27 x 4 staging registers of the next
//   chunk and the operands come on top: about 400 in all, no scratch -- groups of 3 need 288 + 120 and spill), and the K loop runs once per
//   group INSIDE the workgroup: the mask words of neighbouring block offsets overlap, so a group per workgroup would need global
//   atomics.  The later passes read A and B from L2.
//   LDS per group: the 128 A rows and the 32 (G + 3) B rows the four waves need for G offsets, of three images: 3 x 288 x 128 B = 108 KiB
//   at G = 2 (dynamic; one workgroup per compute unit), plus 4 KiB of mask half words that live across the groups.
//   Loads are k_ld_tile's: plain 16-byte global loads into registers for chunk c + 1 before the MFMAs of chunk c, written to LDS after
//   them.  Rows at or beyond `rows` and bytes at or beyond ceil16(n) are staged as zeros and never read: a pair with such a row has N = 0
//   and is not comparable.
//   Epilogues are k_ld_tile's two with the pair's own sums taken from the accumulators: the mask bit under the strict >, ORed into the
//   tile's words in LDS and stored once after the last group by plain 8-byte stores; or the fp64 r2, -1.0 where the pair is not
//   comparable (i + o >= rows included), every entry of the band written once by the one block pair that holds it.  Every word of `mask`
//   and every entry of `band` has one owning workgroup: no global atomics, a deterministic result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

typedef int bl_i32x4 __attribute__((ext_vector_type(4)));
typedef int bl_i32x16 __attribute__((ext_vector_type(16)));

#define BL_TM 128   /* panel markers per workgroup */
#define BL_BK 128   /* individuals (bytes of a row) per staged chunk */
#define BL_G 2      /* block offsets per pass over K */

#define BL_LAUNCH_CHECK(ctx)                                                \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

// bed: staged rows of rb = ceil(n / 4) bytes; panel marker p of the window is staged row offsets[p] (p itself when offsets is null).
// X, C, U: P x ld int8.  pieces = ld / 16.
__global__ __launch_bounds__(256) void k_bed_ld_pack(const uint8_t* __restrict__ bed, long staged, long rb, const long* __restrict__ offsets,
                                                     long P, long n, long ld, long pieces, int8_t* __restrict__ X, int8_t* __restrict__ C,
                                                     int8_t* __restrict__ U) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= P * pieces) return;
    const long p = gid / pieces, t = gid - p * pieces;
    const long src = offsets ? offsets[p] : p;
    uint32_t bits = 0;                                  // 16 codes, individual 16 t + q at bits 2 q
    if (src >= 0 && src < staged) {
        const uint8_t* row = bed + src * rb;
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (4 * t + b < rb) bits |= (uint32_t)row[4 * t + b] << (8 * b);
    }
    bl_i32x4 vx = {0, 0, 0, 0}, vc = {0, 0, 0, 0}, vu = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const uint32_t code = (bits >> (2 * q)) & 3u;
        const bool in = 16 * t + q < n;                 // the pad pairs of the last byte, and the bytes beyond it, belong to nobody
        const uint32_t c = (in && code != 1u) ? 1u : 0u;
        const uint32_t u = (in && (code == 0u || code == 3u)) ? 1u : 0u;
        const uint32_t x = (in && code == 0u) ? 0xffu : u;      // -1 as a byte, else u: 0 or +1
        const int sh = 8 * (q & 3);
        vx[q >> 2] |= (int)(x << sh);
        vc[q >> 2] |= (int)(c << sh);
        vu[q >> 2] |= (int)(u << sh);
    }
    const long at = p * ld + 16 * t;
    *(bl_i32x4*)(X + at) = vx;
    *(bl_i32x4*)(C + at) = vc;
    *(bl_i32x4*)(U + at) = vu;
}

// One pass over K for the G block offsets g0 .. g0 + G - 1 of the tile at row0, and their epilogue.  tile: 3 images x R rows x 128 B with
// R = 128 + 32 (GMAX + 3); rows [0, 128) of an image are the A rows, row 128 + x is tile row 32 g0 + x.  sM: 128 x 8 mask half words.
template <int G, int R, bool R2>
__device__ __forceinline__ void bedld_group(int8_t* tile, unsigned* sM, const int8_t* __restrict__ X8, const int8_t* __restrict__ C8,
                                            const int8_t* __restrict__ U8, long rows, long ld, long kbytes, long row0, int g0, int window,
                                            double t, long min_overlap, double* __restrict__ band) {
    constexpr int RU = BL_TM + 32 * (G + 3);     // rows of an image this group stages
    constexpr int PER = RU / 32;                 // 16-byte pieces per thread, image and chunk: RU * 8 / 256
    constexpr int NCH = 3 * PER;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;

    bl_i32x4 pre[NCH];
    auto fetch = [&](long k0) {
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int m = i / PER, idx = tid + 256 * (i - m * PER), rr = idx >> 3;
            const long kb = k0 + 16 * (idx & 7);
            const long g = row0 + (rr < BL_TM ? rr : 32 * g0 + rr - BL_TM);
            const int8_t* img = m == 0 ? X8 : (m == 1 ? C8 : U8);
            bl_i32x4 v = {0, 0, 0, 0};
            if (kb < kbytes && g < rows) v = *(const bl_i32x4*)(img + g * ld + kb);
            pre[i] = v;
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int m = i / PER, idx = tid + 256 * (i - m * PER), rr = idx >> 3, c = idx & 7;
            *(bl_i32x4*)(tile + (m * R + rr) * BL_BK + ((c ^ ((rr >> 1) & 7)) << 4)) = pre[i];
        }
    };

    // products: 0 X.X = D, 1 X.C = Si, 2 C.X = Sj, 3 C.C = N, 4 U.C = Qi, 5 C.U = Qj  (first factor: the A marker i)
    bl_i32x16 acc[G][6];
#pragma unroll
    for (int b = 0; b < G; b++)
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[b][p][e] = 0;

    const int8_t* pa = tile + (32 * w + r) * BL_BK;
    const int8_t* pb = tile + (BL_TM + 32 * w + r) * BL_BK;
    const int swz = (r >> 1) & 7;

    fetch(0);
    for (long k0 = 0; k0 < kbytes; k0 += BL_BK) {
        put();
        __syncthreads();
        if (k0 + BL_BK < kbytes) fetch(k0 + BL_BK);
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
            const int ch = ((2 * ks + h) ^ swz) << 4;
            const bl_i32x4 ax = *(const bl_i32x4*)(pa + ch);
            const bl_i32x4 ac = *(const bl_i32x4*)(pa + R * BL_BK + ch);
            const bl_i32x4 au = *(const bl_i32x4*)(pa + 2 * R * BL_BK + ch);
#pragma unroll
            for (int b = 0; b < G; b++) {
                const bl_i32x4 bx = *(const bl_i32x4*)(pb + b * (32 * BL_BK) + ch);
                const bl_i32x4 bc = *(const bl_i32x4*)(pb + R * BL_BK + b * (32 * BL_BK) + ch);
                const bl_i32x4 bu = *(const bl_i32x4*)(pb + 2 * R * BL_BK + b * (32 * BL_BK) + ch);
                acc[b][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ax, bx, acc[b][0], 0, 0, 0);
                acc[b][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ax, bc, acc[b][1], 0, 0, 0);
                acc[b][2] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ac, bx, acc[b][2], 0, 0, 0);
                acc[b][3] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ac, bc, acc[b][3], 0, 0, 0);
                acc[b][4] = __builtin_amdgcn_mfma_i32_32x32x32_i8(au, bc, acc[b][4], 0, 0, 0);
                acc[b][5] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ac, bu, acc[b][5], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // accumulator element e of offset b: marker i = 32 w + (e & 3) + 8 (e >> 2) + 4 h of the tile (the A row), j = 32 (g0 + w + b) + r
#pragma unroll
    for (int b = 0; b < G; b++) {
        const int jl = 32 * (g0 + w + b) + r;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int il = 32 * w + (e & 3) + 8 * (e >> 2) + 4 * h, o = jl - il;
            const long gi = row0 + il;
            if (o < 1 || o > window || gi >= rows) continue;
            const long long N = acc[b][3][e], D = acc[b][0][e], Si = acc[b][1][e], Sj = acc[b][2][e], Qi = acc[b][4][e], Qj = acc[b][5][e];
            const long long vi = N * Qi - Si * Si, vj = N * Qj - Sj * Sj;
            const bool ok = N >= min_overlap && vi > 0 && vj > 0;       // a row at or beyond `rows` was staged as zeros: N = 0
            const double dc = (double)(N * D - Si * Sj);
            if (R2) {
                band[gi * window + (o - 1)] = ok ? (dc * dc) / ((double)vi * (double)vj) : -1.0;
            } else if (ok && dc * dc > t * ((double)vi * (double)vj)) {
                atomicOr(&sM[il * 8 + ((o - 1) >> 5)], 1u << ((o - 1) & 31));
            }
        }
    }
}

// kbytes = ceil16(n).  t / mask / wpr: band mode; band: r2 mode (rows x window fp64).  Dynamic LDS: 3 * R * 128 + 4096 bytes.
template <int NB, bool R2>
__global__ __launch_bounds__(256) void k_bedld_tile(const int8_t* __restrict__ X8, const int8_t* __restrict__ C8, const int8_t* __restrict__ U8,
                                                    long rows, long ld, long kbytes, int window, double t, long min_overlap,
                                                    uint64_t* __restrict__ mask, int wpr, double* __restrict__ band) {
    constexpr int GMAX = NB < BL_G ? NB : BL_G;
    constexpr int R = BL_TM + 32 * (GMAX + 3);
    extern __shared__ __attribute__((aligned(16))) int8_t bl_lds[];
    int8_t* tile = bl_lds;
    unsigned* sM = (unsigned*)(bl_lds + 3 * R * BL_BK);
    const int tid = threadIdx.x;
    const long row0 = (long)blockIdx.x * BL_TM;
    if (!R2) {
        for (int x = tid; x < BL_TM * 8; x += 256) sM[x] = 0u;
        __syncthreads();
    }
    // the NB block offsets in groups of BL_G = 2, the last one shorter
#define BL_GROUP(G0)                                                                                                      \
    if constexpr (NB > G0)                                                                                                \
        bedld_group<(NB - G0 < BL_G ? NB - G0 : BL_G), R, R2>(tile, sM, X8, C8, U8, rows, ld, kbytes, row0, G0, window, t, \
                                                              min_overlap, band);
    BL_GROUP(0) BL_GROUP(2) BL_GROUP(4) BL_GROUP(6) BL_GROUP(8)
#undef BL_GROUP
    if (R2) return;
    __syncthreads();
    for (int x = tid; x < BL_TM * wpr; x += 256) {
        const int il = x / wpr, wd = x - il * wpr;
        const long gi = row0 + il;
        if (gi < rows) mask[gi * wpr + wd] = (uint64_t)sM[il * 8 + 2 * wd] | ((uint64_t)sM[il * 8 + 2 * wd + 1] << 32);
    }
}

static bool bedld_bad_images(const int8_t* X, const int8_t* C, const int8_t* U, long n, long ld) {
    return !X || !C || !U || n <= 0 || n > ld || ld % 16 || (((uintptr_t)X | (uintptr_t)C | (uintptr_t)U) & 15) || n > 0x3fffffffL;
}

static size_t bedld_lds_bytes(int nb) { return (size_t)3 * (BL_TM + 32 * ((nb < BL_G ? nb : BL_G) + 3)) * BL_BK + 4096; }

// offsets: P device longs, each in [0, staged), or null (panel marker p is staged row p; then P <= staged)
extern "C" int eagle_dev_bed_ld_pack(eagle_ctx* ctx, const uint8_t* bed, long staged, const long* offsets, long P, long n, long ld, int8_t* X,
                                     int8_t* C, int8_t* U, void* stream) {
    if (P <= 0) return EAGLE_OK;
    if (!bed || staged <= 0 || bedld_bad_images(X, C, U, n, ld) || (!offsets && P > staged))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_ld_pack: bad image shape");
    const long pieces = ld / 16;
    if (P > 0x7fffffffffffL / pieces) return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_ld_pack: too many rows");
    const long blocks = (P * pieces + 255) / 256;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_ld_pack: too many rows");
    hipLaunchKernelGGL(k_bed_ld_pack, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, bed, staged, (n + 3) / 4, offsets, P, n, ld, pieces,
                       X, C, U);
    BL_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

template <bool R2>
static int bedld_launch(eagle_ctx* ctx, const char* who, const int8_t* X, const int8_t* C, const int8_t* U, long rows, long n, long ld, long window,
                        double t, long min_overlap, uint64_t* mask, long wpr, double* band, hipStream_t s) {
    const long blocks = (rows + BL_TM - 1) / BL_TM;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "bedld: too many rows");
    const dim3 grid((unsigned)blocks), blk(256);
    const long kbytes = (n + 15) / 16 * 16;
    const int nb = (int)((window + 31) / 32) + 1;
    const size_t lds = bedld_lds_bytes(nb);
#define BL_CASE(NB)                                                                                                                      \
    case NB: {                                                                                                                           \
        const uint32_t bit = 1u << (2 * (NB - 2) + (R2 ? 1 : 0)); /* per device */                                                       \
        if (!(ctx->attr_bedld & bit)) {                                                                                                  \
            hipError_t e = hipFuncSetAttribute((const void*)k_bedld_tile<NB, R2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) return eagle_fail_hip(ctx, e, "hipFuncSetAttribute(k_bedld_tile)");                                     \
            ctx->attr_bedld |= bit;                                                                                                      \
        }                                                                                                                                \
        hipLaunchKernelGGL((k_bedld_tile<NB, R2>), grid, blk, lds, s, X, C, U, rows, ld, kbytes, (int)window, t, min_overlap, mask,      \
                           (int)wpr, band);                                                                                              \
    } break;
    switch (nb) {
        BL_CASE(2) BL_CASE(3) BL_CASE(4) BL_CASE(5) BL_CASE(6) BL_CASE(7) BL_CASE(8) BL_CASE(9)
    }
#undef BL_CASE
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return eagle_fail_hip(ctx, e, who);
    return EAGLE_OK;
}

extern "C" int eagle_dev_bedld_band(eagle_ctx* ctx, const int8_t* X, const int8_t* C, const int8_t* U, long rows, long n, long ld, long window,
                                    double t, long min_overlap, uint64_t* mask, long words_per_row, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (bedld_bad_images(X, C, U, n, ld)) return eagle_fail(ctx, EAGLE_ERR_ARG, "bedld_band: bad image shape");
    if (window < 1 || window > 256 || words_per_row != (window + 63) / 64 || !(t >= 0.0 && t <= 1.0) || min_overlap < 1 || !mask)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "bedld_band: bad window, threshold, overlap or mask width");
    return bedld_launch<false>(ctx, "eagle_dev_bedld_band", X, C, U, rows, n, ld, window, t, min_overlap, mask, words_per_row, nullptr,
                               (hipStream_t)stream);
}

// band: rows x window fp64, every entry written
extern "C" int eagle_dev_bedld_r2band(eagle_ctx* ctx, const int8_t* X, const int8_t* C, const int8_t* U, long rows, long n, long ld, long window,
                                      long min_overlap, double* band, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (bedld_bad_images(X, C, U, n, ld)) return eagle_fail(ctx, EAGLE_ERR_ARG, "bedld_r2band: bad image shape");
    if (window < 1 || window > 256 || min_overlap < 1 || !band) return eagle_fail(ctx, EAGLE_ERR_ARG, "bedld_r2band: bad window or overlap");
    return bedld_launch<true>(ctx, "eagle_dev_bedld_r2band", X, C, U, rows, n, ld, window, 0.0, min_overlap, nullptr, 0, band, (hipStream_t)stream);
}
