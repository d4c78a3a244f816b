// eagle_bedibs.hip -- pairwise-complete IBS counts straight from a SNP-major PLINK .bed file (include/eagle_hip.h section 1b'''ii): the
// operand pass and the finish of four exact Gram products on the fp4 SYRK (eagle_dev_mmt_accumulate_f4).  Integer arithmetic only.
//
//   k_bed_pack_fp4 ..... a window of raw .bed rows (ceil(n/4) bytes per marker, individual 4b+q at bits 2q of byte b; codes 0 hom A1,
//                        1 missing, 2 het, 3 hom A2) -> FOUR individual-major fp4 operand images M4[plane][individual][marker / 2], the
//                        layout, nibble order and e2m1 codes of k_transpose_pack_fp4:  g = -1, 0, 0, +1 (0xA, 0, 0, 0x2),  u = |g|,
//                        h = [code == 2],  c = [code != 1]  (0x2 where the indicator holds).  One read of the window feeds all four
//                        planes.  A block owns 256 markers x 128 individuals: 32 bytes of each of 256 rows, 8 KiB, staged in LDS with
//                        byte loads (rows have no alignment and lie back to back); whatever lies outside the window, outside the row
//                        or at an excluded marker is staged as 0x55, four missing codes, which is zero in every plane.  A thread then
//                        gathers 128 markers of one individual -- a wave reads 16 consecutive bytes of one staged row, four lanes to
//                        a byte: one bank row, same-dword lanes broadcast, conflict free -- as sixteen dwords of eight 2-bit codes
//                        spread to nibbles; an individual >= n gets the all-missing pattern.  Every plane is a few bit operations on
//                        those dwords; its 128 x 128 bytes go through an LDS stage of pitch 144 (the 16-byte writes of 8 neighbouring
//                        rows on different banks) and out as whole 128-byte lines, as in k_transpose_pack_fp4.  Consecutive blocks
//                        take consecutive byte columns of the same 256 rows, so a 128-byte line of the window is fetched once.
//   k_bed_ibs_finish ... the four int32 accumulators D = g g^T, Q = u u^T, H = h h^T, N = c c^T (upper 256-tiles live) -> the full
//                        symmetric int32 matrices ncalled = N, ibs0 = (Q - D) / 2, hethet = H, hetsum = H + N - Q and, when asked,
//                        the uint32 distance.  k_ibs_finish's shape: one block per 32 x 32 tile on or above the diagonal, coalesced
//                        reads and writes, the mirror image through LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_host.h"
#include "eagle_internal.h"

typedef int bi_i32x4 __attribute__((ext_vector_type(4)));

#define BI_LAUNCH_CHECK(ctx)                                                \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

#define BI_PITCH 144   // bytes between the rows of the output stage

// plane p of eight nibble-spread codes: lo / hi = the codes' two bits at bit 0 of every nibble
__device__ __forceinline__ uint32_t bi_plane(uint32_t x, int p) {
    const uint32_t lo = x & 0x11111111u, hi = (x >> 1) & 0x11111111u;
    const uint32_t u = ~(lo ^ hi) & 0x11111111u;                      // codes 0 and 3: homozygous
    if (p == 0) return (u << 1) | ((~(lo | hi) & 0x11111111u) << 3);  // g: 1.0 with the sign bit where the code is 0
    if (p == 1) return u << 1;                                        // u = |g|
    if (p == 2) return (hi & ~lo) << 1;                               // h: code 2
    return (~(lo & ~hi) & 0x11111111u) << 1;                          // c: every code but 1
}

__global__ __launch_bounds__(256) void k_bed_pack_fp4(const uint8_t* __restrict__ bed, long rb, long rows, long n,
                                                      const uint8_t* __restrict__ include, uint8_t* __restrict__ out, long ld4,
                                                      long plane_bytes) {
    __shared__ uint8_t in[256][32];
    __shared__ __attribute__((aligned(16))) uint8_t stage[128 * BI_PITCH];
    const int t = threadIdx.x;
    const long c0 = (long)blockIdx.x * 128, b0 = (long)blockIdx.x * 32, r0 = (long)blockIdx.y * 256;
#pragma unroll 8
    for (int i = 0; i < 32; i++) {
        const int idx = t + 256 * i, row = idx >> 5, byte = idx & 31;
        const long r = r0 + row, b = b0 + byte;
        uint8_t v = 0x55;
        if (r < rows && b < rb && (!include || include[r])) v = bed[r * rb + b];
        in[row][byte] = v;
    }
    __syncthreads();
    const int c = t & 127, part = t >> 7;
    const uint8_t* col = &in[part * 128][c >> 2];
    const int sh = 2 * (c & 3);
    uint32_t x[16];
    const bool live = c0 + c < n;      // the pad bit pairs of a row's last byte and the rows n .. n_pad: nobody's
#pragma unroll
    for (int v = 0; v < 16; v++) {
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) w |= (((uint32_t)col[(v * 8 + j) * 32] >> sh) & 3u) << (4 * j);
        x[v] = live ? w : 0x11111111u;
    }
#pragma unroll
    for (int p = 0; p < 4; p++) {
        if (p) __syncthreads();        // the stage's previous plane has gone out
#pragma unroll
        for (int v4 = 0; v4 < 4; v4++)
            *(bi_i32x4*)(stage + c * BI_PITCH + part * 64 + 16 * v4) =
                bi_i32x4{(int)bi_plane(x[4 * v4], p), (int)bi_plane(x[4 * v4 + 1], p), (int)bi_plane(x[4 * v4 + 2], p), (int)bi_plane(x[4 * v4 + 3], p)};
        __syncthreads();
        uint8_t* o = out + (long)p * plane_bytes;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int chunk = t + 256 * i, row = chunk >> 3, piece = chunk & 7;
            *(bi_i32x4*)(o + (c0 + row) * ld4 + r0 / 2 + piece * 16) = *(const bi_i32x4*)(stage + row * BI_PITCH + piece * 16);
        }
    }
}

// M4 + p * plane_bytes, p = 0 .. 3: the images of g, u, h, c (n_pad rows of ld4 bytes; L_pad markers written, the rows [n, n_pad) and
// the markers [rows, L_pad) zero) of `rows` raw .bed rows of n individuals; include (device, one byte per row, or null): rows with a
// zero byte are zero in every plane.
extern "C" int eagle_dev_bed_pack_fp4(eagle_ctx* ctx, const uint8_t* bed, long rows, long n, const uint8_t* include, long n_pad, long L_pad,
                                      void* M4, long ld4, long plane_bytes, void* stream) {
    if (rows <= 0 || n <= 0 || n > n_pad || n_pad % 128 || L_pad % 256 || rows > L_pad || ld4 % 128 || ld4 < L_pad / 2 ||
        plane_bytes % 128 || plane_bytes < n_pad * ld4 || ((uintptr_t)M4 & 127) || L_pad / 256 > 65535)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_pack_fp4: layout contract violated (n_pad % 128, L_pad % 256, ld4 % 128, L_pad < 2^24)");
    hipLaunchKernelGGL(k_bed_pack_fp4, dim3((unsigned)(n_pad / 128), (unsigned)(L_pad / 256)), dim3(256), 0, (hipStream_t)stream, bed,
                       bed_row_bytes(n), rows, n, include, (uint8_t*)M4, ld4, plane_bytes);
    BI_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

__global__ __launch_bounds__(256) void k_bed_ibs_finish(const int32_t* __restrict__ D, const int32_t* __restrict__ Q, const int32_t* __restrict__ H,
                                                        const int32_t* __restrict__ N, long n, long ldc, long linc, int min_overlap,
                                                        int32_t* __restrict__ ncalled, int32_t* __restrict__ ibs0, int32_t* __restrict__ hethet,
                                                        int32_t* __restrict__ hetsum, uint32_t* __restrict__ dist) {
    const long bi = (long)blockIdx.y * 32, bj = (long)blockIdx.x * 32;
    if (bj < bi) return;
    __shared__ int32_t tl[5][32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long j = bj + tx;
    for (int r = ty; r < 32; r += 8) {
        const long i = bi + r;
        int nc = 0, a = 0, h = 0, hs = 0;
        uint32_t dd = 0;
        if (i < n && j < n) {
            const long at = i * ldc + j;
            const int q = Q[at];
            nc = N[at];
            h = H[at];
            a = (q - D[at]) >> 1;                   // opposite homozygotes: the difference is even and not negative
            hs = h + nc - q;                        // both called, at least one heterozygous: one count per heterozygous genotype
            const long o = i * n + j;
            ncalled[o] = nc;
            ibs0[o] = a;
            hethet[o] = h;
            hetsum[o] = hs;
            if (dist) {
                const long d = 4L * a + hs - 2L * h;   // sum of (g_i - g_j)^2 over the both-called markers, <= 4 nc
                dd = nc < min_overlap ? 0xFFFFFFFEu : (uint32_t)((unsigned long long)(d * linc) / (unsigned long long)nc);
                dist[o] = dd;
            }
        }
        tl[0][r][tx] = nc;
        tl[1][r][tx] = a;
        tl[2][r][tx] = h;
        tl[3][r][tx] = hs;
        tl[4][r][tx] = (int32_t)dd;
    }
    __syncthreads();
    if (bj > bi)
        for (int r = ty; r < 32; r += 8) {
            const long jj = bj + r, ii = bi + tx;   // out[jj][ii] = the value at (ii, jj)
            if (ii < n && jj < n) {
                const long o = jj * n + ii;
                ncalled[o] = tl[0][tx][r];
                ibs0[o] = tl[1][tx][r];
                hethet[o] = tl[2][tx][r];
                hetsum[o] = tl[3][tx][r];
                if (dist) dist[o] = (uint32_t)tl[4][tx][r];
            }
        }
}

// The four n x n int32 results (and dist, or null) from the accumulators (n_pad x n_pad, upper 256-tiles live); linc = the number of
// included markers (< 2^29, so that d * linc < 2^62), min_overlap >= 1 (so that the division has a divisor).
extern "C" int eagle_dev_bed_ibs_finish(eagle_ctx* ctx, const int32_t* D32, const int32_t* Q32, const int32_t* H32, const int32_t* N32, long n,
                                        long n_pad, long linc, int min_overlap, int32_t* ncalled, int32_t* ibs0, int32_t* hethet, int32_t* hetsum,
                                        uint32_t* dist, void* stream) {
    if (n <= 0 || n > n_pad || n_pad % 256 || linc < 0 || linc >= (1L << 29) || min_overlap < 1)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_ibs_finish: bad shape");
    const unsigned nb = (unsigned)((n + 31) / 32);
    hipLaunchKernelGGL(k_bed_ibs_finish, dim3(nb, nb), dim3(256), 0, (hipStream_t)stream, D32, Q32, H32, N32, n, n_pad, linc, min_overlap, ncalled,
                       ibs0, hethet, hetsum, dist);
    BI_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}
