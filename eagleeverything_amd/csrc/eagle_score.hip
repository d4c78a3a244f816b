// eagle_score.hip -- the exact int8 line-score pass of include/eagle_hip.h section 1b''''i (eagle_sample_scores, eagle_marker_scores):
//     out[r][t] = sum_c w[t][c] g[r][c],   |w| <= 2^30 = d0 + 256 d1 + 256^2 d2 + 256^3 d3,  d in [-128, 127],   g in {-1, 0, +1}
// for the lines r of a genotype image and T <= 64 weight columns, as one int8 x int8 product on the tile engine of k_syrk_i8
// (eagle_t8.h) whose second operand holds one row per weight column and live digit plane:
//
//   k_score_digits ..... B[col(t, p)][c] = digit p of w[t][c], zero from character `cols` on and in the rows up to the next multiple
//                        of 64.  Only the planes that are not zero over the whole call get rows (the caller's plane mask); the live
//                        planes are ranked in increasing p and col(t, p) = rank(p) T + t, so the live columns are a prefix
//   k_line_scores_i8 ... C32[r][col] += sum_k A[r][k] B[col][k]: the stage loop of t8_gram_tiles (LDS-DMA staging, 256 x 256 tile, K
//                        splits, XCD-aware order, integer atomics) over the rectangular work list (row tile, 0) x K splits.  A wave
//                        whose 64 columns lie beyond the live ones still issues its share of the staging and skips its MFMAs
//   k_scores_finish .... out[r][t] = sum over the live planes of 256^p C32[r][col(t, p)] in int64, rows x T, unpadded
//
// The int32 accumulators hold |sum| <= 128 cols < 2^31 (cols <= EAGLE_SCORES_MAX_LINE); the image is read once and never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

#include "eagle_t8.h"

#define SCORE_LAUNCH_CHECK(ctx)                                             \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

typedef unsigned score_u32x4 __attribute__((ext_vector_type(4)));

// Live planes of a mask in increasing order; the number of them.
struct ScorePlanes { int n, p[4]; };
static inline ScorePlanes score_planes(int mask) {
    ScorePlanes s = {0, {0, 0, 0, 0}};
    for (int p = 0; p < 4; p++) if (mask >> p & 1) s.p[s.n++] = p;
    return s;
}

// One thread per 16 bytes of a row of B: grid.x = 16-byte groups of ld / 256, grid.y = rows of B (a multiple of 64).
__global__ __launch_bounds__(256) void k_score_digits(const int32_t* __restrict__ w, long T, long cols, long ld, ScorePlanes pl,
                                                      int8_t* __restrict__ B) {
    const long grp = (long)blockIdx.x * 256 + threadIdx.x;
    if (grp * 16 >= ld) return;
    const long row = blockIdx.y;
    score_u32x4 o = {0u, 0u, 0u, 0u};
    if (row < pl.n * T) {
        const int p = pl.p[row / T];
        const int32_t* wt = w + (row % T) * cols;
#pragma unroll
        for (int b = 0; b < 16; b++) {
            const long c = grp * 16 + b;
            if (c < cols) o[b >> 2] |= (unsigned)(uint8_t)score_digit(wt[c], p) << (8 * (b & 3));
        }
    }
    *(score_u32x4*)(B + row * ld + grp * 16) = o;
}

extern "C" int eagle_dev_score_digits(eagle_ctx* ctx, const int32_t* w, long T, long cols, long ld, int plane_mask, int8_t* B, void* stream) {
    const ScorePlanes pl = score_planes(plane_mask);
    if (!w || !B || T < 1 || T > EAGLE_SCORES_MAX_COLUMNS || cols <= 0 || cols > ld || ld % 128 || plane_mask < 0 || plane_mask > 15 ||
        (uintptr_t)B % 16)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "score_digits: layout contract violated (1 <= T <= 64, cols <= ld, ld % 128)");
    const long rowsB = eagle_score_b_rows(T, plane_mask);
    if (rowsB == 0) return EAGLE_OK;
    hipLaunchKernelGGL(k_score_digits, dim3((unsigned)((ld / 16 + 255) / 256), (unsigned)rowsB), dim3(256), 0, (hipStream_t)stream, w, T, cols, ld,
                       pl, B);
    SCORE_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// The stage loop of t8_gram_tiles with a rectangular work list: logical block lid = split * ntiles + row tile, column tile 0 always.
// B's descriptor ends behind its rowsB rows (a multiple of 64): the staging of the rows beyond them fetches nothing, and the waves
// that would read them (wc * 64 >= rowsB) run no MFMA and add nothing.
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 2) void k_line_scores_i8(const int8_t* __restrict__ A, const int8_t* __restrict__ B, long ld_, int rowsB,
                                                           int ntiles, int nblocks, long nstages, long stages_per_split,
                                                           int32_t* __restrict__ C, long ldc) {
    __shared__ __attribute__((aligned(1024))) int8_t lds[2][2][TILE_BYTES];
    const int cpx = (gridDim.x + 7) / 8;
    const int lid = (blockIdx.x & 7) * cpx + (blockIdx.x >> 3);
    if (lid >= nblocks) return;
    const int split = lid / ntiles;
    const int ti = lid - split * ntiles;
    const long s0 = (long)split * stages_per_split;
    long s1 = s0 + stages_per_split;
    if (s1 > nstages) s1 = nstages;
    if (s0 >= s1) return;
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = w >> 2, wc = w & 3;
    const bool active = wc * 64 < rowsB;
    const int ld = (int)ld_;
    const T8Lane ln = t8_lane(lane, ld);
    const __amdgpu_buffer_rsrc_t rsA = t8_rsrc(A + (long)ti * T8 * ld_, ld);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)B, 0, rowsB * ld, 0x00020000);
    i32x16 acc[4][2];
    t8_zero(acc);
    t8_stage(rsA, ln, ld, (int)(s0 * BK8), lds[0][0], w);
    t8_stage(rsB, ln, ld, (int)(s0 * BK8), lds[0][1], w);
    __syncthreads();
    int cur = 0;
    const T8Read rd = t8_read_init(wr, wc, lane);
    for (long s = s0; s < s1; s++) {
        const int kn = (int)((s + 1) * BK8);
        const bool more = s + 1 < s1;
        if (active) {
            t8_stage_compute(acc, lds[cur][0], lds[cur][1], rd, more, rsA, ln, ld, kn, lds[cur ^ 1][0], rsB, ln, ld, kn, lds[cur ^ 1][1], w);
        } else if (more) {
            t8_stage(rsA, ln, ld, kn, lds[cur ^ 1][0], w);
            t8_stage(rsB, ln, ld, kn, lds[cur ^ 1][1], w);
        }
        __syncthreads();
        cur ^= 1;
    }
    if (!active) return;
    // C/D map of the 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
    const int col = lane & 31, rq = 4 * (lane >> 5);
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int q = 0; q < 16; q++) {
                const long i = (long)ti * T8 + wr * 128 + m * 32 + (q & 3) + 8 * (q >> 2) + rq;
                const long j = wc * 64 + n * 32 + col;   // < rowsB <= ldc: the wave is active
                const int v = acc[m][n][q];
                if (v) atomicAdd(&C[i * ldc + j], v);
            }
}

// One thread per output element.
__global__ __launch_bounds__(256) void k_scores_finish(const int32_t* __restrict__ C, long ldc, long rows, long T, ScorePlanes pl,
                                                       int64_t* __restrict__ out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * T) return;
    const long r = e / T, t = e - r * T;
    int64_t v = 0;
    for (int k = 0; k < pl.n; k++) v += (int64_t)C[r * ldc + k * T + t] * ((int64_t)1 << (8 * pl.p[k]));
    out[e] = v;
}

// Row tiles per launch: the accumulators of one launch, 256 rows x rowsB int32 per tile, stay below 256 MiB.
#define SCORE_CHUNK_TILES 1024L

extern "C" long eagle_score_b_rows(long T, int plane_mask) { return (score_planes(plane_mask).n * T + 63) / 64 * 64; }
extern "C" size_t eagle_line_scores_ws_bytes(long rows, long T, int plane_mask) {
    const long tiles = std::min((rows + T8 - 1) / T8, SCORE_CHUNK_TILES);
    return sizeof(int32_t) * (size_t)tiles * T8 * (size_t)eagle_score_b_rows(T, plane_mask);
}

// out (rows x T int64, device) from the image (the rows up to the next multiple of 256 allocated, ld bytes each) and the digit image B
// of eagle_dev_score_digits for the same T, plane_mask and ld; c32: eagle_line_scores_ws_bytes(rows, T, plane_mask) bytes.
extern "C" int eagle_dev_line_scores(eagle_ctx* ctx, const int8_t* img, long rows, long cols, long ld, const int8_t* B, long T, int plane_mask,
                                     int32_t* c32, int64_t* out, void* stream) {
    if (!img || !out || rows <= 0 || cols <= 0 || cols > EAGLE_SCORES_MAX_LINE || T < 1 || T > EAGLE_SCORES_MAX_COLUMNS || plane_mask < 0 ||
        plane_mask > 15 || ld % 128 || (cols + BK8 - 1) / BK8 * BK8 > ld || (double)ld * T8 >= 2147483648.0 || ((uintptr_t)img | (uintptr_t)B) % 16)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "line_scores: layout contract violated (ld % 128, pad128(cols) <= ld < 2^23, 1 <= T <= 64)");
    const ScorePlanes pl = score_planes(plane_mask);
    const long rowsB = eagle_score_b_rows(T, plane_mask);
    if (rowsB == 0) {   // every weight is zero
        HIPCHK(ctx, hipMemsetAsync(out, 0, sizeof(int64_t) * (size_t)rows * (size_t)T, (hipStream_t)stream));
        return EAGLE_OK;
    }
    if (!B || !c32) return eagle_fail(ctx, EAGLE_ERR_ARG, "line_scores: NULL operand");
    const long nstages = (cols + BK8 - 1) / BK8;
    const long tiles_all = (rows + T8 - 1) / T8;
    for (long t0 = 0; t0 < tiles_all; t0 += SCORE_CHUNK_TILES) {
        const long ntiles = std::min(SCORE_CHUNK_TILES, tiles_all - t0);
        const long r0 = t0 * T8, nr = std::min(rows - r0, ntiles * T8);
        // the launch rules of eagle_dev_gram_i8ab: K splits of at least 16 stages, about 10 waves of 256 workgroups
        long want = (10L * 256 + ntiles - 1) / ntiles;
        long maxsplit = nstages / 16 > 0 ? nstages / 16 : 1;
        long nsplit = want < maxsplit ? want : maxsplit;
        if (nsplit < 1) nsplit = 1;
        const long per = (nstages + nsplit - 1) / nsplit;
        nsplit = (nstages + per - 1) / per;
        const long nblocks = ntiles * nsplit;
        if (nblocks >= (1L << 30)) return eagle_fail(ctx, EAGLE_ERR_ARG, "line_scores: too many workgroups");
        HIPCHK(ctx, hipMemsetAsync(c32, 0, sizeof(int32_t) * (size_t)ntiles * T8 * (size_t)rowsB, (hipStream_t)stream));
        hipLaunchKernelGGL(k_line_scores_i8, dim3((unsigned)((nblocks + 7) / 8 * 8)), dim3(512), 0, (hipStream_t)stream, img + r0 * ld, B, ld,
                           (int)rowsB, (int)ntiles, (int)nblocks, nstages, per, c32, rowsB);
        SCORE_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(k_scores_finish, dim3((unsigned)((nr * T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c32, rowsB, nr, T, pl,
                           out + r0 * T);
        SCORE_LAUNCH_CHECK(ctx);
    }
    return EAGLE_OK;
}
