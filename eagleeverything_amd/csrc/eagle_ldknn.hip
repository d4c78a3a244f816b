// eagle_ldknn.hip -- LD-kNNi: imputation of the missing genotypes of a SNP-major PLINK .bed file from neighbours that are ranked PER
// MARKER, over the marker's partners in local LD (include/eagle_hip.h section 1b'''iii).  Integer arithmetic only: a scalar restatement
// gives the same bytes (r_api.impute_ldknn_host).
//
//   k_bed_impute_ldknn ... raw .bed rows (a window with its halo) + partners + the window rows' counts (k_bed_marker_counts) -> patched
//                          rows and (by vote, by fallback) per row.  One workgroup of 8 waves per target marker; a marker without a
//                          missing call is a row copy.
//     1. gather: thread = byte column b (four individuals).  It reads byte b of the <= 32 partner rows and transposes their bit pairs
//        into three words per individual, bit p = partner p:  called (code != 01), hom (code 00 or 11), homA2 (code 11).  They go to LDS
//        as three arrays of pad4(n) dwords, written 16 bytes per thread and array, read one dword per lane at consecutive addresses:
//        free of bank conflicts both ways.  12 bytes per individual: EAGLE_LDKNN_MAX_N comes from the 160 KiB of a CU.
//     2. a wave per missing individual i of the marker (the waves walk the staged target row 16 individuals at a time and take the
//        words' missing fields in turn).  With B = called_i & called_j:  ov = popc(B),  d = popc(B & (hom_i ^ hom_j)) + 4 popc(hom_i &
//        hom_j & (homA2_i ^ homA2_j)),  key = (uint64)(d * 4096 / ov) << 32 | j for the j that are called at the marker and have
//        ov >= min_overlap.  Lane x keeps the smallest key among j = x, x + 64, ...; k rounds of the 64-bit wave minimum pick the voters in
//        increasing key order.  Keys are distinct, so the round's winner is retired by its value: only the lane that owned it scans its
//        entries again, for its smallest key above the winner's.  No list of taken entries, no barrier inside a wave's work.
//     3. the vote reads the codes of the staged target row; lane 0 XORs the field from 01 to its new code in a second copy of the row in
//        LDS (an LDS atomic on the dword: every field is patched once, so the result has no order), and adds to the row's two counts
//        in LDS.  After a barrier the patched row leaves by plain byte stores and the counts by their one owner: no global atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_host.h"
#include "eagle_internal.h"

#define LDK_THREADS 512
#define LDK_WAVES (LDK_THREADS / 64)
#define LDK_NONE 0xffffffffffffffffull

// dynamic LDS of a block: three word arrays of pad4(n) dwords, two copies of the target row in whole dwords
static inline size_t ldk_lds_bytes(long n) { return (size_t)(3 * ((n + 3) / 4 * 4) + 2 * ((bed_row_bytes(n) + 3) / 4)) * 4; }
// 160 KiB of LDS per CU, 1 KiB kept for the kernel's static arrays
static_assert(12 * EAGLE_LDKNN_MAX_N + 2 * (EAGLE_LDKNN_MAX_N / 4) + 1024 <= 160 * 1024 && EAGLE_LDKNN_MAX_N % 16 == 0, "one block per CU at the largest n");

__device__ __forceinline__ unsigned long long ldk_wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
        const unsigned long long u = (unsigned long long)hi << 32 | lo;
        v = u < v ? u : v;
    }
    return v;
}

// 2-bit code of dosage g = 0, 1, 2: 00, 10, 11
__device__ __forceinline__ uint32_t ldk_code(int g) { return g == 0 ? 0u : (g == 1 ? 2u : 3u); }

// bed: the staged rows, row 0 = marker h_lo of the file; the window's rows start at row `first` of them and at marker m0 of the file.
// partners: L x l by the file's marker, every entry -1 or a marker among the staged rows (the caller's check).  mcounts / out / counts: by
// the window's row.
__global__ __launch_bounds__(LDK_THREADS) void k_bed_impute_ldknn(const uint8_t* __restrict__ bed, long rb, int n, long first, long m0, long h_lo,
                                                                  const int32_t* __restrict__ partners, int l, int k, int min_votes,
                                                                  int min_overlap, const int32_t* __restrict__ mcounts,
                                                                  uint8_t* __restrict__ out, int32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ldk_lds[];
    __shared__ int sPart[EAGLE_LDKNN_MAX_PARTNERS];
    __shared__ int sCnt[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long r = blockIdx.x;
    const int np = (n + 3) & ~3, rbw = (int)((rb + 3) >> 2);
    uint32_t* sC = ldk_lds;
    uint32_t* sH = sC + np;
    uint32_t* sA = sH + np;
    uint32_t* tgt = sA + np;                  // the target row as it is in the file (pad fields 00): what the votes read
    uint32_t* outw = tgt + rbw;               // the row that leaves
    const uint8_t* trow = bed + (first + r) * rb;
    uint8_t* orow = out + r * rb;
    const int32_t* mc = mcounts + r * 4;      // hom A1, het, hom A2, missing
    const int left = n - (int)(4 * (rb - 1)); // individuals in the row's last byte (1 .. 4)
    const uint32_t keep = left < 4 ? (1u << (2 * left)) - 1u : 0xffu;   // the pad bit pairs of a row's last byte go out as 00
    if (mc[3] == 0) {                         // the same for every thread of the block: a row copy
        for (long b = tid; b < rb; b += LDK_THREADS) orow[b] = (uint8_t)(b == rb - 1 ? trow[b] & keep : trow[b]);
        if (tid == 0) { counts[r * 2] = 0; counts[r * 2 + 1] = 0; }
        return;
    }
    const int fc = mc[0] + mc[1] + mc[2], fs = mc[1] + 2 * mc[2];
    const uint32_t fb = fc > 0 ? ldk_code((2 * fs + fc) / (2 * fc)) : 2u;   // no call at all: het, the ingestion's rule

    for (int b = tid; b < 4 * rbw; b += LDK_THREADS) {
        const uint32_t x = b < rb ? (b == rb - 1 ? trow[b] & keep : trow[b]) : 0u;
        ((uint8_t*)tgt)[b] = (uint8_t)x;
        ((uint8_t*)outw)[b] = (uint8_t)x;
    }
    if (tid < EAGLE_LDKNN_MAX_PARTNERS) {
        const int p = tid < l ? partners[(m0 + r) * l + tid] : -1;
        sPart[tid] = p < 0 ? -1 : (int)(p - h_lo);
    }
    if (tid < 2) sCnt[tid] = 0;
    __syncthreads();

    // 1. gather
    for (int b = tid; b < (int)rb; b += LDK_THREADS) {
        uint32_t c[4] = {0u, 0u, 0u, 0u}, h[4] = {0u, 0u, 0u, 0u}, a[4] = {0u, 0u, 0u, 0u};
        for (int p = 0; p < l; p++) {
            const int pr = sPart[p];
            if (pr < 0) continue;
            const uint32_t x = bed[(long)pr * rb + b];
            const uint32_t lo = x & 0x55u, hi = (x >> 1) & 0x55u;
            const uint32_t cl = ~(lo & ~hi) & 0x55u, hm = ~(lo ^ hi) & 0x55u, a2 = lo & hi;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                c[q] |= ((cl >> (2 * q)) & 1u) << p;
                h[q] |= ((hm >> (2 * q)) & 1u) << p;
                a[q] |= ((a2 >> (2 * q)) & 1u) << p;
            }
        }
        // 4 b + 3 < pad4(n): the words of the pad fields are written and never read
        *(uint4*)(sC + 4 * b) = make_uint4(c[0], c[1], c[2], c[3]);
        *(uint4*)(sH + 4 * b) = make_uint4(h[0], h[1], h[2], h[3]);
        *(uint4*)(sA + 4 * b) = make_uint4(a[0], a[1], a[2], a[3]);
    }
    __syncthreads();

    // 2. and 3.
    const uint8_t* tb = (const uint8_t*)tgt;
    for (int wd = wv; wd < rbw; wd += LDK_WAVES) {
        const uint32_t x = tgt[wd];
        uint32_t miss = x & ~(x >> 1) & 0x55555555u;                  // lo & ~hi: bit 2q set iff field q is 01
        while (miss) {
            const int q2 = __ffs(miss) - 1;                           // = 2 q
            miss &= miss - 1;
            const int i = 16 * wd + (q2 >> 1);                        // < n: the pad fields are 00
            const uint32_t ci = sC[i], hi_ = sH[i], ai = sA[i];
            // the lane's smallest key that is at least `from`
            auto scan = [&](unsigned long long from) {
                unsigned long long best = LDK_NONE;
                for (int j = lane; j < n; j += 64) {
                    if (((tb[j >> 2] >> (2 * (j & 3))) & 3u) == 1u) continue;      // not called at the marker (i itself is among these)
                    const uint32_t B = ci & sC[j];
                    const uint32_t ov = (uint32_t)__popc(B);
                    if ((int)ov < min_overlap) continue;                           // min_overlap >= 1: no division by zero
                    const uint32_t hj = sH[j];
                    const uint32_t d = (uint32_t)__popc(B & (hi_ ^ hj)) + 4u * (uint32_t)__popc(hi_ & hj & (ai ^ sA[j]));
                    const unsigned long long key = (unsigned long long)((d * 4096u) / ov) << 32 | (unsigned)j;
                    if (key >= from && key < best) best = key;
                }
                return best;
            };
            unsigned long long best = scan(0ull);
            int c = 0, s = 0;
            for (int t = 0; t < k; t++) {
                const unsigned long long win = ldk_wave_min(best);
                if (win == LDK_NONE) break;                           // fewer than k eligible: the same in every lane
                const int j = (int)(unsigned)win;
                const uint32_t code = (tb[j >> 2] >> (2 * (j & 3))) & 3u;
                c++;
                s += (int)(code - (code >> 1));                       // dosage: 0 -> 0, 2 -> 1, 3 -> 2
                if (t + 1 < k && (j & 63) == lane) best = scan(win + 1ull);
            }
            if (lane == 0) {
                uint32_t code;
                if (c >= min_votes) { code = ldk_code((2 * s + c) / (2 * c)); atomicAdd(&sCnt[0], 1); }
                else { code = fb; atomicAdd(&sCnt[1], 1); }
                atomicXor(&outw[wd], (1u ^ code) << q2);              // 01 -> code
            }
        }
    }
    __syncthreads();
    for (long b = tid; b < rb; b += LDK_THREADS) orow[b] = ((const uint8_t*)outw)[b];
    if (tid < 2) counts[r * 2 + tid] = sCnt[tid];
}

// out = the `rows` raw .bed rows that start at row `first` of `bed` (marker m0 of the file; row 0 of `bed` is marker h_lo, and `staged` rows
// lie there) with every missing genotype filled; counts[rows][2] = (by vote, by fallback); mcounts[rows][4] = the rows' counts from
// eagle_dev_bed_marker_counts; partners = L x l int32 on the device, every entry of the rows [m0, m0 + rows) either -1 or in
// [h_lo, h_lo + staged) (checked by the caller: the kernel indexes the staged rows with them).
extern "C" int eagle_dev_bed_impute_ldknn(eagle_ctx* ctx, const uint8_t* bed, long staged, long first, long rows, long m0, long h_lo, long n,
                                          const int32_t* partners, int l, int k, int min_votes, int min_overlap, const int32_t* mcounts,
                                          uint8_t* out, int32_t* counts, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (n <= 0 || n > EAGLE_LDKNN_MAX_N || l < 1 || l > EAGLE_LDKNN_MAX_PARTNERS || k < 1 || k > EAGLE_LDKNN_MAX_K || min_votes < 1 ||
        min_overlap < 1 || min_overlap > EAGLE_LDKNN_MAX_PARTNERS || first < 0 || first + rows > staged || h_lo < 0 || m0 != h_lo + first ||
        rows > 0x7fffffffL)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_impute_ldknn: bad shape");
    if (!ctx->attr_ldknn) {  // per device
        hipError_t e = hipFuncSetAttribute((const void*)k_bed_impute_ldknn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)ldk_lds_bytes(EAGLE_LDKNN_MAX_N));
        if (e != hipSuccess) return eagle_fail_hip(ctx, e, "hipFuncSetAttribute(k_bed_impute_ldknn)");
        ctx->attr_ldknn = true;
    }
    hipLaunchKernelGGL(k_bed_impute_ldknn, dim3((unsigned)rows), dim3(LDK_THREADS), ldk_lds_bytes(n), (hipStream_t)stream, bed, bed_row_bytes(n),
                       (int)n, first, m0, h_lo, partners, l, k, min_votes, min_overlap, mcounts, out, counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return eagle_fail_hip(ctx, e, __func__);
    return EAGLE_OK;
}
