// eagle_impute.hip -- k-nearest-neighbour imputation of the missing genotypes of a SNP-major PLINK .bed file (include/eagle_hip.h
// section 1b'''i).  Integer arithmetic in a fixed order only: a scalar restatement gives the same bytes (r_api.knn_rows_host,
// r_api.impute_knn_host).
//
//   k_knn_rows ..... ibs0, hethet (n x n int32, eagle_sample_ibs) -> nbr[n][K] int32.  One block per individual i.  The block writes
//                    d_ij = 4 ibs0_ij + h_i + h_j - 2 hethet_ij of its row into LDS, one dword per individual j (the key of j is
//                    (uint64)d_ij << 32 | j, so the dword at position j is the whole key), the entry of i itself as the sentinel
//                    0xffffffff.  Thread t owns the entries j = t, t + 256, ... and keeps the smallest key among them in registers;
//                    K_eff = min(K, n - 1) rounds of a block-wide minimum (a 64-bit butterfly in the wave, four wave minima through
//                    LDS) pick the neighbours in increasing key order.  Only the owner of a round's winner marks it taken and scans
//                    its entries again: a thread touches no other thread's entries, so a round needs one barrier, the reduction's (the
//                    wave minima alternate between two LDS slots).  k_knn_rows_dist is the same selection on a uint32 matrix whose
//                    dwords are the keys' high halves as they stand (eagle_bed_sample_ibs' dist, section 1b'''ii).
//   k_bed_impute ... raw .bed rows + nbr + the rows' counts (k_bed_marker_counts) -> patched rows and (by vote, by fallback) per row.
//                    A block owns a group of whole rows: their original bytes are staged in LDS with byte loads (rb = ceil(n/4) has no
//                    alignment and the rows lie back to back), every vote reads original codes from that copy, so the result does
//                    not depend on the order in which genotypes are filled.  A thread owns one byte column (four individuals) and
//                    walks down the block's rows, so the neighbour lists it reads are the same for every row (they stay in L1/L2);
//                    rows shorter than the block are worked on 256 / rb at a time.  The missing fields of a byte are the set bits of
//                    the plane lo & ~hi; each is filled by the walk over nbr[i][0 .. K) defined in the header.  The patched byte
//                    goes out with a plain byte store.  LDS bank behaviour: staging writes and the walk's reads are byte accesses at
//                    consecutive (staging) or data-dependent (neighbours) addresses -- the first conflict-free, the second a gather
//                    that no layout of whole rows orders; a neighbour shared by the four fields of a byte or by a lane group is
//                    one broadcast.  The rows' two counts are added in LDS (ds_add, integer: order-free) and stored by the block
//                    as the rows' sole owner: no global atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_host.h"
#include "eagle_internal.h"

#define IMP_LAUNCH_CHECK(ctx)                                               \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

// ------------------------------------------------------------------------------------------------------------------------------
// neighbour table
// ------------------------------------------------------------------------------------------------------------------------------
#define KNN_TAKEN 0xffffffffu
#define KNN_NONE 0xffffffffffffffffull

__device__ __forceinline__ unsigned long long knn_min64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

__device__ __forceinline__ unsigned long long knn_wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
        v = knn_min64(v, (unsigned long long)hi << 32 | lo);
    }
    return v;
}

// the smallest key among the entries j = tid, tid + 256, ... of the row that are not taken
__device__ __forceinline__ unsigned long long knn_scan(const uint32_t* d, int n, int tid) {
    unsigned long long best = KNN_NONE;
    for (int j = tid; j < n; j += 256) {
        const uint32_t v = d[j];
        if (v != KNN_TAKEN) best = knn_min64(best, (unsigned long long)v << 32 | (unsigned)j);
    }
    return best;
}

// DIST: the row's dwords are read as they are from a uint32 matrix (`ibs0` is that matrix, `hethet` is not used): k_knn_rows_dist
template <bool DIST>
__device__ __forceinline__ void knn_rows_body(const int32_t* __restrict__ ibs0, const int32_t* __restrict__ hethet, int n, int K, int keff,
                                              int32_t* __restrict__ nbr) {
    extern __shared__ uint32_t knn_d[];          // n dwords: d of the row; KNN_TAKEN for i itself and for the neighbours picked so far
    __shared__ unsigned long long wmin[2][4];    // by the round's parity: one barrier per round
    const int i = blockIdx.x, tid = threadIdx.x;
    const long row = (long)i * n;
    if constexpr (DIST) {
        for (int j = tid; j < n; j += 256) knn_d[j] = j == i ? KNN_TAKEN : (uint32_t)ibs0[row + j];
    } else {
        const uint32_t hi = (uint32_t)hethet[row + i];
        for (int j = tid; j < n; j += 256) {
            const uint32_t hj = (uint32_t)hethet[(long)j * n + j];
            // int32 arithmetic (unsigned, so that it is defined): exact while 4 L < 2^31
            const uint32_t dij = 4u * (uint32_t)ibs0[row + j] + hi + hj - 2u * (uint32_t)hethet[row + j];
            knn_d[j] = j == i ? KNN_TAKEN : dij;
        }
    }
    // every thread reads back only what it wrote: no barrier before the scan
    unsigned long long best = knn_scan(knn_d, n, tid);
    for (int t = 0; t < keff; t++) {
        const unsigned long long w = knn_wave_min(best);
        unsigned long long* wm = wmin[t & 1];
        if ((tid & 63) == 0) wm[tid >> 6] = w;
        __syncthreads();
        const unsigned long long win = knn_min64(knn_min64(wm[0], wm[1]), knn_min64(wm[2], wm[3]));
        // keff <= n - 1, so there is a winner -- unless a wrapped d (4 L >= 2^31) equals KNN_TAKEN: then -1, and nothing is marked
        const int j = win == KNN_NONE ? -1 : (int)(unsigned)win;
        if (tid == 0) nbr[(long)i * K + t] = j;
        if (j >= 0 && (j & 255) == tid) {
            knn_d[j] = KNN_TAKEN;
            best = knn_scan(knn_d, n, tid);
        }
    }
    for (int t = keff + tid; t < K; t += 256) nbr[(long)i * K + t] = -1;
}

__global__ __launch_bounds__(256) void k_knn_rows(const int32_t* __restrict__ ibs0, const int32_t* __restrict__ hethet, int n, int K, int keff,
                                                  int32_t* __restrict__ nbr) {
    knn_rows_body<false>(ibs0, hethet, n, K, keff, nbr);
}
// the same selection with the key's high dword read from dist (n x n uint32): a distance of 0xffffffff would read as taken, and
// eagle_bed_sample_ibs writes none above 0xfffffffe
__global__ __launch_bounds__(256) void k_knn_rows_dist(const uint32_t* __restrict__ dist, int n, int K, int keff, int32_t* __restrict__ nbr) {
    knn_rows_body<true>((const int32_t*)dist, nullptr, n, K, keff, nbr);
}

extern "C" int eagle_dev_knn_rows(eagle_ctx* ctx, const int32_t* ibs0, const int32_t* hethet, long n, int K, int32_t* nbr, void* stream) {
    if (n <= 0 || n > EAGLE_KNN_MAX_N || K < 1 || K > EAGLE_KNN_MAX_K) return eagle_fail(ctx, EAGLE_ERR_ARG, "knn_rows: bad shape");
    if (!ctx->attr_knn_rows) {  // per device
        hipError_t e = hipFuncSetAttribute((const void*)k_knn_rows, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * (int)EAGLE_KNN_MAX_N);
        if (e != hipSuccess) return eagle_fail_hip(ctx, e, "hipFuncSetAttribute(k_knn_rows)");
        ctx->attr_knn_rows = true;
    }
    const int keff = (int)std::min((long)K, n - 1);
    hipLaunchKernelGGL(k_knn_rows, dim3((unsigned)n), dim3(256), (size_t)(4 * n), (hipStream_t)stream, ibs0, hethet, (int)n, K, keff, nbr);
    IMP_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

extern "C" int eagle_dev_knn_rows_dist(eagle_ctx* ctx, const uint32_t* dist, long n, int K, int32_t* nbr, void* stream) {
    if (n <= 0 || n > EAGLE_KNN_MAX_N || K < 1 || K > EAGLE_KNN_MAX_K) return eagle_fail(ctx, EAGLE_ERR_ARG, "knn_rows_dist: bad shape");
    if (!ctx->attr_knn_rows_dist) {  // per device
        hipError_t e = hipFuncSetAttribute((const void*)k_knn_rows_dist, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * (int)EAGLE_KNN_MAX_N);
        if (e != hipSuccess) return eagle_fail_hip(ctx, e, "hipFuncSetAttribute(k_knn_rows_dist)");
        ctx->attr_knn_rows_dist = true;
    }
    const int keff = (int)std::min((long)K, n - 1);
    hipLaunchKernelGGL(k_knn_rows_dist, dim3((unsigned)n), dim3(256), (size_t)(4 * n), (hipStream_t)stream, dist, (int)n, K, keff, nbr);
    IMP_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// imputation of staged .bed rows
// ------------------------------------------------------------------------------------------------------------------------------
#define IMP_STAGE_BYTES (EAGLE_IMPUTE_MAX_N / 4)             // the longest row; two blocks' stages fit a CU's 160 KiB
#define IMP_MAX_ROWS 256                                     // rows of a block (the size of its count arrays)
static_assert(EAGLE_IMPUTE_MAX_N % 4 == 0 && 2 * (IMP_STAGE_BYTES + 9 * IMP_MAX_ROWS) <= 160 * 1024, "two blocks per CU");

// rows of a block: whole rows within the stage, about 16 KiB of them when rows are short (more blocks per CU, and blocks enough for
// every CU on windows of a few thousand rows), never more than the count arrays hold
static inline long imp_rows_per_block(long rb) {
    return std::max(1L, std::min(std::min((long)IMP_STAGE_BYTES / rb, (long)IMP_MAX_ROWS), std::max(1L, 16384L / rb)));
}

// 2-bit code of dosage g = 0, 1, 2: 00, 10, 11
__device__ __forceinline__ uint32_t imp_code(int g) { return g == 0 ? 0u : (g == 1 ? 2u : 3u); }

__global__ __launch_bounds__(256) void k_bed_impute(const uint8_t* __restrict__ bed, long rb, long rows, int n, int R,
                                                    const int32_t* __restrict__ nbr, int K, int k, int min_votes,
                                                    const int32_t* __restrict__ mcounts, uint8_t* __restrict__ out,
                                                    int32_t* __restrict__ counts) {
    __shared__ uint8_t stage[IMP_STAGE_BYTES];
    __shared__ int cnt[IMP_MAX_ROWS][2];
    __shared__ uint8_t fb[IMP_MAX_ROWS];         // the rows' fallback codes
    const int tid = threadIdx.x;
    const long row0 = (long)blockIdx.x * R;
    const int nr = (int)(rows - row0 < R ? rows - row0 : R);     // > 0: the grid is ceil(rows / R)
    const long bytes = (long)nr * rb;
    const uint8_t* src = bed + row0 * rb;
    for (long o = tid; o < bytes; o += 256) stage[o] = src[o];
    for (int r = tid; r < nr; r += 256) {
        cnt[r][0] = 0;
        cnt[r][1] = 0;
        const int32_t* mc = mcounts + (row0 + r) * 4;            // hom A1, het, hom A2, missing
        const int c = mc[0] + mc[1] + mc[2], s = mc[1] + 2 * mc[2];
        fb[r] = (uint8_t)(c > 0 ? imp_code((2 * s + c) / (2 * c)) : 2u);   // no call at all: het, the ingestion's rule
    }
    __syncthreads();
    // byte column b of rows sub, sub + rpp, ...: rb >= 256 -> every thread its columns b = tid, tid + 256, ... of every row;
    // rb < 256 -> rpp = 256 / rb rows at a time, thread = (row sub, column b), the threads beyond rpp * rb idle
    const int rpp = rb >= 256 ? 1 : (int)(256 / rb);
    const int sub = rb >= 256 ? 0 : (int)(tid / rb);
    if (sub < rpp) {
        for (long b = rb >= 256 ? tid : tid - sub * rb; b < rb; b += 256) {
            const int left = n - (int)(4 * b);                                  // individuals of the file among this byte's four fields (> 0)
            const uint32_t keep = left < 4 ? (1u << (2 * left)) - 1u : 0xffu;   // the pad bit pairs of a row's last byte go out as 00
            for (int r = sub; r < nr; r += rpp) {
                const uint8_t* rowp = stage + (long)r * rb;
                uint32_t x = (uint32_t)rowp[b] & keep;
                uint32_t miss = x & ~(x >> 1) & 0x55u;                          // lo & ~hi: bit 2q set iff field q is 01
                int votes = 0, fallbacks = 0;
                while (miss) {
                    const int q2 = __ffs(miss) - 1;                             // = 2 q
                    miss &= miss - 1;
                    const int32_t* list = nbr + ((long)(4 * b) + (q2 >> 1)) * K;
                    int c = 0, s = 0;
                    for (int t = 0; t < K && c < k; t++) {
                        const int j = list[t];
                        if (j < 0) continue;                                    // the tail beyond K_eff
                        const uint32_t code = ((uint32_t)rowp[j >> 2] >> (2 * (j & 3))) & 3u;
                        if (code != 1u) {
                            c++;
                            s += (int)(code - (code >> 1));                     // dosage: 0 -> 0, 2 -> 1, 3 -> 2
                        }
                    }
                    uint32_t code;
                    if (c >= min_votes) { code = imp_code((2 * s + c) / (2 * c)); votes++; }
                    else { code = fb[r]; fallbacks++; }
                    x = (x & ~(3u << q2)) | (code << q2);
                }
                out[(row0 + r) * rb + b] = (uint8_t)x;
                if (votes) atomicAdd(&cnt[r][0], votes);
                if (fallbacks) atomicAdd(&cnt[r][1], fallbacks);
            }
        }
    }
    __syncthreads();
    for (int r = tid; r < nr; r += 256) {
        counts[(row0 + r) * 2] = cnt[r][0];
        counts[(row0 + r) * 2 + 1] = cnt[r][1];
    }
}

// out = the `rows` raw .bed rows at `bed` with every missing genotype filled; counts[rows][2] = (by vote, by fallback); mcounts[rows][4]
// = the rows' counts from eagle_dev_bed_marker_counts; nbr = n x K int32 on the device, every entry in [-1, n) (checked by the caller:
// the kernel indexes the staged row with them).
extern "C" int eagle_dev_bed_impute(eagle_ctx* ctx, const uint8_t* bed, long rows, long n, const int32_t* nbr, int K, int k, int min_votes,
                                    const int32_t* mcounts, uint8_t* out, int32_t* counts, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (n <= 0 || n > EAGLE_IMPUTE_MAX_N || K < 1 || K > EAGLE_KNN_MAX_K || k < 1 || k > K || min_votes < 1)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_impute: bad shape");
    const long rb = bed_row_bytes(n), R = imp_rows_per_block(rb), blocks = (rows + R - 1) / R;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_impute: too many rows");
    hipLaunchKernelGGL(k_bed_impute, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, bed, rb, rows, (int)n, (int)R, nbr, K, k, min_votes,
                       mcounts, out, counts);
    IMP_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}
