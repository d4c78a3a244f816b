// eagle_groups.hip -- genotype counts of every marker WITHIN each of K <= 64 groups of individuals (include/eagle_hip.h section
// 1b''''iii), and Fisher's exact test of 2 x 2 tables.  The counts are exact integers; the statistics made of them (allele frequencies
// per population, Fst, the case/control tests) are the caller's fp64 arithmetic (r_api.GroupCounts / Fst / CaseControl).
//
//   k_group_onehot ....... labels[n] (int32 in [-1, K)) -> the label operand: a 64 x ld int8 image, byte (k, i) = 1 iff labels[i] == k,
//                          zero from column n on and in the rows >= K (no label names them).
//   k_group_tile<NB> ..... the int8 marker-major image Mt8 (rows x ld, values -1/0/+1, zero padding) x the label operand -> int32
//                          counts[rows][K][3] = (n0, n1, n2) of every marker among every group.  NB = 1 for K <= 32, 2 up to 64.
//   k_group_bedmask ...... labels[n] -> K bit-mask planes of nd = ceil(ceil(n/4) / 4) dwords: bit 2q of byte b of plane k is set iff
//                          individual 4b + q is in group k (so every bit of a plane lies in 0x55555555 and none beyond individual n - 1).
//   k_bed_group_counts ... raw SNP-major .bed rows x the planes -> int32 counts[rows][K][4] = (hom A1, het, hom A2, missing).
//   k_fisher_2x2 ......... int32 tables[L][4] -> the two-sided exact p-value of every table, one table per thread.
//
// k_group_tile is the sibling of the picks mode k_ld_tile<2, true> of eagle_ld.hip and takes its tile from there: a workgroup (256
// threads, 4 waves) owns 128 consecutive markers over ALL n (no K split); per chunk of 128 individuals it stages 128 marker rows and the
// 32 NB rows of the label operand, 128 B each, in LDS -- logical 16-byte chunk c of row r at physical chunk c ^ ((r >> 1) & 7), plain
// 16-byte global loads issued for chunk c + 1 before the MFMAs of chunk c, rows at or beyond `rows` and bytes at or beyond ceil16(n)
// staged as zeros and never read.  Wave w multiplies the 32-marker block w against the NB label blocks on v_mfma_i32_32x32x32_i8, and it
// uses every A fragment TWICE: as it is, which accumulates s = sum_{i in k} g, and as a & 0x01010101 per dword -- g^2 of -1 / 0 / +1 (0xff,
// 0x00, 0x01), made in registers -- which accumulates q = sum_{i in k} g^2 in a second accumulator set.  2 NB 16 <= 64 accumulator
// registers per lane; the image is read once and no squared image exists anywhere.  Epilogue: accumulator element e of block b is marker
// 32 w + (e & 3) + 8 (e >> 2) + 4 h of the tile and group 32 b + (lane & 31); n2 = (q + s) / 2, n0 = (q - s) / 2, n1 = size_k - q leave by
// plain 4-byte vector stores, every word of `counts` having one owner: no atomics, a deterministic result.
//
// Why the MFMA and not v_dot4 against per-group byte masks: at K = 32 the masks cost 16 dot instructions per genotype dword and group
// pair, which is VALU-bound well above the HBM time of the image; the two one-hot products are a fraction of the matrix pipe under the
// same read (DESIGN.md section 4.8o has the measured numbers).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

typedef int gr_i32x4 __attribute__((ext_vector_type(4)));
typedef int gr_i32x16 __attribute__((ext_vector_type(16)));

#define GR_TM 128   /* markers per workgroup */
#define GR_BK 128   /* individuals (bytes of a row) per staged chunk */
#define GR_ROWS 64  /* rows of the label operand = EAGLE_GROUPS_MAX */

#define GR_LAUNCH_CHECK(ctx)                                                \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

// one thread = 16 bytes of one row of the operand; lanes16 = ld / 16
__global__ __launch_bounds__(256) void k_group_onehot(const int32_t* __restrict__ labels, long n, long ld, long lanes16, int8_t* __restrict__ out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= GR_ROWS * lanes16) return;
    const int k = (int)(t / lanes16);
    const long i0 = (t - k * lanes16) * 16;
    gr_i32x4 v = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++)
        if (i0 + j < n && labels[i0 + j] == k) v[j >> 2] |= 1 << (8 * (j & 3));
    *(gr_i32x4*)(out + (long)k * ld + i0) = v;
}

// kbytes = ceil16(n): the bytes of a row that hold individuals.  H: GR_ROWS x ldH, the label operand.  sizes[k] = individuals of group k.
template <int NB>
__global__ __launch_bounds__(256) void k_group_tile(const int8_t* __restrict__ Mt8, long rows, long ld, long kbytes, const int8_t* __restrict__ H,
                                                    long ldH, int K, const int32_t* __restrict__ sizes, int32_t* __restrict__ counts) {
    constexpr int TB = GR_TM + 32 * NB;
    constexpr int NCH = TB / 32;   // 16-byte pieces per thread and chunk: TB * 8 / 256
    __shared__ __attribute__((aligned(16))) int8_t tile[TB * GR_BK];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const long row0 = (long)blockIdx.x * GR_TM;

    gr_i32x4 pre[NCH];
    auto fetch = [&](long k0) {
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int idx = tid + 256 * i, rr = idx >> 3;
            const long kb = k0 + 16 * (idx & 7);
            gr_i32x4 v = {0, 0, 0, 0};
            if (kb < kbytes) {
                if (rr >= GR_TM) v = *(const gr_i32x4*)(H + (long)(rr - GR_TM) * ldH + kb);
                else if (row0 + rr < rows) v = *(const gr_i32x4*)(Mt8 + (row0 + rr) * ld + kb);
            }
            pre[i] = v;
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int idx = tid + 256 * i, rr = idx >> 3, c = idx & 7;
            *(gr_i32x4*)(tile + rr * GR_BK + ((c ^ ((rr >> 1) & 7)) << 4)) = pre[i];
        }
    };

    gr_i32x16 accS[NB], accQ[NB];
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int e = 0; e < 16; e++) accS[b][e] = accQ[b][e] = 0;

    const int8_t* pa = tile + (32 * w + r) * GR_BK;
    const int8_t* pb = tile + (GR_TM + r) * GR_BK;
    const int swz = (r >> 1) & 7;

    fetch(0);
    for (long k0 = 0; k0 < kbytes; k0 += GR_BK) {
        put();
        __syncthreads();
        if (k0 + GR_BK < kbytes) fetch(k0 + GR_BK);
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
            const int ch = ((2 * ks + h) ^ swz) << 4;
            const gr_i32x4 a = *(const gr_i32x4*)(pa + ch);
            const gr_i32x4 a2 = a & 0x01010101;                     // g^2 of -1 / 0 / +1
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const gr_i32x4 bb = *(const gr_i32x4*)(pb + b * (32 * GR_BK) + ch);
                accS[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bb, accS[b], 0, 0, 0);
                accQ[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a2, bb, accQ[b], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // accumulator element e of block b: marker i = 32 w + (e & 3) + 8 (e >> 2) + 4 h of the tile (the A row), group 32 b + (lane & 31)
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const int k = 32 * b + r;
        if (k >= K) continue;
        const int size = sizes[k];
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const long gi = row0 + 32 * w + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (gi >= rows) continue;
            const int s = accS[b][e], q = accQ[b][e];
            int32_t* c = counts + (gi * K + k) * 3;
            c[0] = (q - s) >> 1;
            c[1] = size - q;
            c[2] = (q + s) >> 1;
        }
    }
}

// one thread = one dword of one plane
__global__ __launch_bounds__(256) void k_group_bedmask(const int32_t* __restrict__ labels, long n, long nd, int K, uint32_t* __restrict__ planes) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)K * nd) return;
    const int k = (int)(t / nd);
    const long i0 = (t - k * nd) * 16;
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 16; j++)
        if (i0 + j < n && labels[i0 + j] == k) m |= 1u << (2 * j);
    planes[t] = m;
}

template <int G>
__device__ __forceinline__ int gr_group_sum(int v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The rows are byte-loaded like k_bed_marker_counts' (rb = ceil(n/4) has no alignment, the rows lie back to back as in the file), G
// lanes per row.  The groups are walked in chunks of GR_BCH, 3 GR_BCH accumulators per lane; every chunk reads the row's dwords again,
// from cache, and the planes stay in L2.  The planes hold no bit beyond individual n - 1: they are the mask of the row's last byte.
#define GR_BCH 8
template <int G>
__global__ __launch_bounds__(256) void k_bed_group_counts(const uint8_t* __restrict__ bed, long rb, long rows, long nd, int K,
                                                          const uint32_t* __restrict__ planes, const int32_t* __restrict__ sizes,
                                                          int32_t* __restrict__ counts) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long row = t / G;
    const int lane = (int)(t % G);
    const uint8_t* s = bed + (row < rows ? row : 0) * rb;
    for (int k0 = 0; k0 < K; k0 += GR_BCH) {              // the same trip count in every lane: the shuffles below see whole groups
        int het[GR_BCH], hom2[GR_BCH], miss[GR_BCH];
#pragma unroll
        for (int kk = 0; kk < GR_BCH; kk++) het[kk] = hom2[kk] = miss[kk] = 0;
        if (row < rows)
            for (long d = lane; d < nd; d += G) {
                const long b0 = 4 * d;
                uint32_t x = 0;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (b0 + j < rb) x |= (uint32_t)s[b0 + j] << (8 * j);
                const uint32_t lo = x & 0x55555555u, hi = (x >> 1) & 0x55555555u;
                const uint32_t pm = lo & ~hi, ph = hi & ~lo, p2 = lo & hi;   // 01, 10, 11
#pragma unroll
                for (int kk = 0; kk < GR_BCH; kk++) {
                    const uint32_t m = k0 + kk < K ? planes[(long)(k0 + kk) * nd + d] : 0u;
                    miss[kk] += __popc(pm & m);
                    het[kk] += __popc(ph & m);
                    hom2[kk] += __popc(p2 & m);
                }
            }
#pragma unroll
        for (int kk = 0; kk < GR_BCH; kk++) {
            const int a = gr_group_sum<G>(het[kk]), b = gr_group_sum<G>(hom2[kk]), c = gr_group_sum<G>(miss[kk]);
            if (row < rows && lane < 4 && k0 + kk < K) {
                const int hom1 = sizes[k0 + kk] - a - b - c;         // 00 among the group's individuals
                counts[(row * K + k0 + kk) * 4 + lane] = lane == 0 ? hom1 : (lane == 1 ? a : (lane == 2 ? b : c));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Fisher's exact test of (a, b; c, d), in the order section 1b''''iii of eagle_hip.h fixes (modelled on hwe_walk of eagle_qc.hip): every
// product, quotient and sum is one correctly rounded fp64 operation, the integer factors are exact int64 products converted once.
// fisher_walk visits the mode x0 first, then the leg below it (x0 - 1, ..., lo), then the leg above (x0 + 1, ..., hi); a leg ends at
// its first term that is exactly 0.0 (every later term is 0.0 too and adds nothing).  With cut < 0 it returns the total and leaves P(a)
// in *p_obs (0.0 where the leg ended before a); with cut >= 0 it returns the sum of the terms <= cut, in the same order.
// ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double fisher_walk(long x0, long lo, long hi, long r1, long r2, long c1, long a, double cut, double* p_obs) {
    const bool tail = cut >= 0.0;
    double sum = (!tail || 1.0 <= cut) ? 1.0 : 0.0;
    double pobs = a == x0 ? 1.0 : 0.0;
    double p = 1.0;
    for (long x = x0; x > lo; x--) {                     // P(x - 1) = P(x) x (r2 - c1 + x) / ((r1 - x + 1) (c1 - x + 1))
        p = __ddiv_rn(__dmul_rn(p, (double)(x * (r2 - c1 + x))), (double)((r1 - x + 1) * (c1 - x + 1)));
        if (p == 0.0) break;
        if (x - 1 == a) pobs = p;
        if (!tail || p <= cut) sum = __dadd_rn(sum, p);
    }
    p = 1.0;
    for (long x = x0; x < hi; x++) {                     // P(x + 1) = P(x) (r1 - x) (c1 - x) / ((x + 1) (r2 - c1 + x + 1))
        p = __ddiv_rn(__dmul_rn(p, (double)((r1 - x) * (c1 - x))), (double)((x + 1) * (r2 - c1 + x + 1)));
        if (p == 0.0) break;
        if (x + 1 == a) pobs = p;
        if (!tail || p <= cut) sum = __dadd_rn(sum, p);
    }
    if (p_obs) *p_obs = pobs;
    return sum;
}

__global__ __launch_bounds__(256) void k_fisher_2x2(const int32_t* __restrict__ tables, long L, double* __restrict__ pout) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= L) return;
    const long a = tables[4 * m], b = tables[4 * m + 1], c = tables[4 * m + 2], d = tables[4 * m + 3];
    const long r1 = a + b, r2 = c + d, c1 = a + c, N = r1 + r2;
    if (N == 0) { pout[m] = 1.0; return; }
    const long lo = c1 - r2 > 0 ? c1 - r2 : 0, hi = r1 < c1 ? r1 : c1;
    long x0 = (r1 + 1) * (c1 + 1) / (N + 2);
    x0 = x0 < lo ? lo : (x0 > hi ? hi : x0);
    double pobs;
    const double total = fisher_walk(x0, lo, hi, r1, r2, c1, a, -1.0, &pobs);
    const double tail = fisher_walk(x0, lo, hi, r1, r2, c1, a, __dmul_rn(pobs, 1.0000001), nullptr);
    const double pv = __ddiv_rn(tail, total);
    pout[m] = pv > 1.0 ? 1.0 : pv;
}

// ------------------------------------------------------------------------------------------------------------------------------
// launchers (device pointers throughout)
// ------------------------------------------------------------------------------------------------------------------------------
static bool gr_bad_image(const int8_t* p, long n, long ld) { return n <= 0 || n > ld || ld % 16 || ((uintptr_t)p & 15) || n > 0x3fffffffL; }

// onehot: GR_ROWS x ld int8, every byte written
extern "C" int eagle_dev_group_onehot(eagle_ctx* ctx, const int32_t* labels, long n, int8_t* onehot, long ld, void* stream) {
    if (gr_bad_image(onehot, n, ld)) return eagle_fail(ctx, EAGLE_ERR_ARG, "group_onehot: bad operand shape");
    const long lanes16 = ld / 16, blocks = (GR_ROWS * lanes16 + 255) / 256;
    hipLaunchKernelGGL(k_group_onehot, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, labels, n, ld, lanes16, onehot);
    GR_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

extern "C" int eagle_dev_group_counts(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, const int8_t* onehot, long ld_onehot, int K,
                                      const int32_t* sizes, int32_t* counts, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (gr_bad_image(Mt8, n, ld) || gr_bad_image(onehot, n, ld_onehot)) return eagle_fail(ctx, EAGLE_ERR_ARG, "group_counts: bad image shape");
    if (K < 1 || K > EAGLE_GROUPS_MAX) return eagle_fail(ctx, EAGLE_ERR_ARG, "group_counts: 1 to 64 groups");
    const long blocks = (rows + GR_TM - 1) / GR_TM;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "group_counts: too many rows");
    const dim3 grid((unsigned)blocks), blk(256);
    const long kbytes = (n + 15) / 16 * 16;
    if (K <= 32) hipLaunchKernelGGL(k_group_tile<1>, grid, blk, 0, (hipStream_t)stream, Mt8, rows, ld, kbytes, onehot, ld_onehot, K, sizes, counts);
    else hipLaunchKernelGGL(k_group_tile<2>, grid, blk, 0, (hipStream_t)stream, Mt8, rows, ld, kbytes, onehot, ld_onehot, K, sizes, counts);
    GR_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// planes: K x ceil(ceil(n/4) / 4) dwords, every one written
extern "C" int eagle_dev_group_bedmask(eagle_ctx* ctx, const int32_t* labels, long n, int K, uint32_t* planes, void* stream) {
    if (n <= 0 || n > 0x3fffffffL || K < 1 || K > EAGLE_GROUPS_MAX) return eagle_fail(ctx, EAGLE_ERR_ARG, "group_bedmask: bad shape");
    const long nd = (bed_row_bytes(n) + 3) / 4, blocks = ((long)K * nd + 255) / 256;
    hipLaunchKernelGGL(k_group_bedmask, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, labels, n, nd, K, planes);
    GR_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

extern "C" int eagle_dev_bed_group_counts(eagle_ctx* ctx, const uint8_t* bed, long rows, long n, int K, const uint32_t* planes, const int32_t* sizes,
                                          int32_t* counts, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (n <= 0 || n > 0x3fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_group_counts: bad shape");
    if (K < 1 || K > EAGLE_GROUPS_MAX) return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_group_counts: 1 to 64 groups");
    const long rb = bed_row_bytes(n), nd = (rb + 3) / 4;
    const int G = nd <= 16 ? 16 : (nd <= 32 ? 32 : 64);
    const long blocks = (rows * G + 255) / 256;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_group_counts: too many rows");
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t s = (hipStream_t)stream;
    if (G == 16) hipLaunchKernelGGL(k_bed_group_counts<16>, grid, blk, 0, s, bed, rb, rows, nd, K, planes, sizes, counts);
    else if (G == 32) hipLaunchKernelGGL(k_bed_group_counts<32>, grid, blk, 0, s, bed, rb, rows, nd, K, planes, sizes, counts);
    else hipLaunchKernelGGL(k_bed_group_counts<64>, grid, blk, 0, s, bed, rb, rows, nd, K, planes, sizes, counts);
    GR_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// tables: device int32 [L][4], every entry >= 0 and every table sum <= 2^30 (the caller's check)
extern "C" int eagle_dev_fisher_2x2(eagle_ctx* ctx, const int32_t* tables, long L, double* p, void* stream) {
    if (L <= 0) return EAGLE_OK;
    const long blocks = (L + 255) / 256;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "fisher_2x2: too many tables");
    hipLaunchKernelGGL(k_fisher_2x2, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tables, L, p);
    GR_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}
