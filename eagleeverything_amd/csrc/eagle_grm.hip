// eagle_grm.hip -- the per-marker weighted Gram product of include/eagle_hip.h section 1b'''' (eagle_weighted_gram):
//     Q_ij = sum_m q_m g_im g_jm,   q_m < 2^21 = d0 + 128 d1 + 128^2 d2,  d in [0, 127],   g in {-1, 0, +1}
// as three exact int8 x int8 products on the tile engine of k_syrk_i8 (eagle_t8.h), one per base-128 digit plane:
//
//   k_scale_cols_i8 ... B_d[j][m] = d_m g_jm for a window of the individual-major int8 image and one digit plane (HBM-bound: 16-byte
//                       loads and stores, one read and one write of the window); the operand of the product is materialised once
//                       per window and plane, because a scaling fused into the operand staging would be redone by every row tile
//   k_gram_i8ab ....... C32[i][j] += sum_k A[i][k] B[j][k]: t8_gram_tiles, the body of k_syrk_i8, with two operand images.  The
//                       result is symmetric although the operands differ (sum_m g_im d_m g_jm), so only the upper-triangular tile
//                       pairs run and a tile on the diagonal is computed in full, exactly as in the SYRK
//   k_wgram_finish .... Q = C0 + 128 C1 + 128^2 C2 in int64 from the live upper 256-tiles, mirrored to the full n x n matrix
//
// The int32 accumulators hold |sum| <= 127 L per plane: eagle_weighted_gram refuses L > 16,909,320 = floor((2^31 - 1) / 127).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

#include "eagle_t8.h"

#define GRM_LAUNCH_CHECK(ctx)                                               \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

typedef unsigned grm_u32x4 __attribute__((ext_vector_type(4)));

// Four packed genotypes g (bytes 0xff, 0x00, 0x01) times four packed digits d (bytes 0 .. 127) -> four packed int8 products, without a
// carry between the bytes: a byte of `nz` is 0xff where g != 0 and a byte of `ng` where g = -1 (a 0 / 1 byte times 0xff fills its own
// byte only); -d per byte is (0x80 - d) ^ 0x80 (0x80 - d lies in [1, 0x80]: no borrow; the flip of the top bit maps 0x80 to 0 and
// 0x80 - d to 0x100 - d).  The product is a selection between d, 0 and -d, nothing is negated in place.
__device__ __forceinline__ unsigned grm_scale4(unsigned g, unsigned d) {
    const unsigned nz = (g & 0x01010101u) * 0xffu;
    const unsigned ng = ((g >> 7) & 0x01010101u) * 0xffu;
    const unsigned negd = (0x80808080u - d) ^ 0x80808080u;
    return (d & nz & ~ng) | (negd & ng);
}

#define GRM_SCALE_ROWS 16   /* rows per block: the digits of a 16-byte column group are loaded once for them */
// grid.x = 16-byte column groups / 256, grid.y = rows / GRM_SCALE_ROWS; consecutive threads take consecutive groups of one row.
__global__ __launch_bounds__(256) void k_scale_cols_i8(const int8_t* __restrict__ A, long ldA, long n, long rows, long groups,
                                                       const uint8_t* __restrict__ digit, int8_t* __restrict__ B, long ldB) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= groups) return;
    const grm_u32x4 d = *(const grm_u32x4*)(digit + c * 16);
    const long r0 = (long)blockIdx.y * GRM_SCALE_ROWS;
#pragma unroll 4
    for (int k = 0; k < GRM_SCALE_ROWS; k++) {
        const long r = r0 + k;
        if (r >= rows) break;
        grm_u32x4 o = {0u, 0u, 0u, 0u};
        if (r < n) {
            const grm_u32x4 g = *(const grm_u32x4*)(A + r * ldA + c * 16);
#pragma unroll
            for (int b = 0; b < 4; b++) o[b] = grm_scale4(g[b], d[b]);
        }
        *(grm_u32x4*)(B + r * ldB + c * 16) = o;
    }
}

extern "C" int eagle_dev_scale_cols_i8(eagle_ctx* ctx, const int8_t* A, long ldA, long n, long rows, long cols, const uint8_t* digit, int8_t* B,
                                       long ldB, void* stream) {
    if (n < 0 || n > rows || rows <= 0 || cols <= 0 || cols % 16 || ldA % 16 || ldB % 16 || cols > ldA || cols > ldB ||
        ((uintptr_t)A | (uintptr_t)B | (uintptr_t)digit) % 16)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "scale_cols_i8: layout contract violated (16-byte column groups and leading dimensions)");
    const long groups = cols / 16, gy = (rows + GRM_SCALE_ROWS - 1) / GRM_SCALE_ROWS;
    if (gy > 65535 || (groups + 255) / 256 > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "scale_cols_i8: window too large");
    hipLaunchKernelGGL(k_scale_cols_i8, dim3((unsigned)((groups + 255) / 256), (unsigned)gy), dim3(256), 0, (hipStream_t)stream, A, ldA, n, rows,
                       groups, digit, B, ldB);
    GRM_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// k_syrk_i8 with two operand images: grid.x = upper-triangular 256-tile pairs x K splits, XCD-aware order, integer atomics.
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 2) void k_gram_i8ab(const int8_t* __restrict__ A, long ldA, const int8_t* __restrict__ B, long ldB,
                                                      const int* __restrict__ pairs, int npairs, int nblocks, long nstages,
                                                      long stages_per_split, int32_t* __restrict__ C, long ldc) {
    __shared__ __attribute__((aligned(1024))) int8_t lds[2][2][TILE_BYTES];
    t8_gram_tiles(lds, A, ldA, B, ldB, pairs, npairs, nblocks, nstages, stages_per_split, C, ldc);
}

// The launch rules of eagle_dev_mmt_accumulate_i8 (tile pairs, K splits of at least 16 stages, about 10 waves of 256 workgroups).
extern "C" int eagle_dev_gram_i8ab(eagle_ctx* ctx, const int8_t* A, long ldA, const int8_t* B, long ldB, long n_pad, long K_pad, int32_t* C32,
                                   void* stream) {
    if (n_pad % T8 || K_pad % BK8 || ldA % 128 || ldB % 128 || K_pad > ldA || K_pad > ldB || n_pad <= 0 || (double)ldA * T8 >= 2147483648.0 ||
        (double)ldB * T8 >= 2147483648.0 || ((uintptr_t)A | (uintptr_t)B) % 16)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "gram_i8ab: layout contract violated (n_pad % 256, K_pad % 128, ld % 128, ld < 2^23)");
    if (K_pad == 0) return EAGLE_OK;
    const int nt = (int)(n_pad / T8);
    const long npairs = (long)nt * (nt + 1) / 2;
    const long nstages = K_pad / BK8;
    long want = (10L * 256 + npairs - 1) / npairs;
    long maxsplit = nstages / 16 > 0 ? nstages / 16 : 1;
    long nsplit = want < maxsplit ? want : maxsplit;
    if (nsplit < 1) nsplit = 1;
    long per = (nstages + nsplit - 1) / nsplit;
    nsplit = (nstages + per - 1) / per;
    const long nblocks = npairs * nsplit;
    if (nt >= 65536 || nblocks >= (1L << 30)) return eagle_fail(ctx, EAGLE_ERR_ARG, "gram_i8ab: too many workgroups");
    const int* pairs = nullptr;
    int rc = syrk_pair_table(ctx, nt, &pairs, (hipStream_t)stream);
    if (rc) return rc;
    dim3 grid((unsigned)((nblocks + 7) / 8 * 8));
    hipLaunchKernelGGL(k_gram_i8ab, grid, dim3(512), 0, (hipStream_t)stream, A, ldA, B, ldB, pairs, (int)npairs, (int)nblocks, nstages, per, C32,
                       n_pad);
    GRM_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// One block per 32 x 32 tile on or above the diagonal (the tiling of k_mmt_finish and k_ibs_finish): coalesced reads of the live
// accumulators, coalesced writes of Q and, through LDS, of its mirror image.  Every element of Q has one owner.
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_wgram_finish(const int32_t* __restrict__ C0, const int32_t* __restrict__ C1,
                                                      const int32_t* __restrict__ C2, long n, long ldc, int64_t* __restrict__ Q) {
    const long bi = (long)blockIdx.y * 32, bj = (long)blockIdx.x * 32;
    if (bj < bi) return;
    __shared__ int64_t tq[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long j = bj + tx;
    for (int r = ty; r < 32; r += 8) {
        const long i = bi + r;
        int64_t v = 0;
        if (i < n && j < n) {
            const long at = i * ldc + j;
            if (C0) v += (int64_t)C0[at];
            if (C1) v += (int64_t)C1[at] * 128;
            if (C2) v += (int64_t)C2[at] * 16384;
            Q[i * n + j] = v;
        }
        tq[r][tx] = v;
    }
    __syncthreads();
    if (bj > bi)
        for (int r = ty; r < 32; r += 8) {
            const long jj = bj + r, ii = bi + tx;   // Q[jj][ii] = the value at (ii, jj)
            if (ii < n && jj < n) Q[jj * n + ii] = tq[tx][r];
        }
}

extern "C" int eagle_dev_wgram_finish(eagle_ctx* ctx, const int32_t* C0, const int32_t* C1, const int32_t* C2, long n, long n_pad, int64_t* Q,
                                      void* stream) {
    if (n <= 0 || n > n_pad || n_pad % 256) return eagle_fail(ctx, EAGLE_ERR_ARG, "wgram_finish: bad shape");
    const unsigned nb = (unsigned)((n + 31) / 32);
    if (nb > 65535) return eagle_fail(ctx, EAGLE_ERR_ARG, "wgram_finish: too many individuals");
    hipLaunchKernelGGL(k_wgram_finish, dim3(nb, nb), dim3(256), 0, (hipStream_t)stream, C0, C1, C2, n, n_pad, Q);
    GRM_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}
