// eagle_vcf.hip -- the sample fields of VCF data lines on the device (include/eagle_hip.h section 1b-vcf; the host side, which stages the
// text and decides which lines are kept, is eagle_vcf_to_bed in eagle_ingest.cpp).  Integer work only, no LDS row of size n, and nothing
// depends on how the file was cut into windows: a line is one workgroup's, whatever else the window holds.
//
//   k_vcf_fields ... one 256-thread workgroup per kept line.  table[2 l], table[2 l + 1] = [beg, end): the line's bytes from its first
//                    sample field to its end ('\r' excluded), offsets into the staged text.  The line is walked in segments of
//                    256 x 16 bytes from beg rounded down to 16: a thread loads its 16 bytes with one aligned 16-byte load (the
//                    CALLER pads the allocation to a multiple of 16 behind the text), forms the 16-bit mask of the tab bytes that lie in
//                    [beg, end) and popcounts it; an exclusive scan over the workgroup (wave shuffles, then the four wave totals
//                    through LDS) plus the running base of the segment gives every tab the ordinal of the field that starts behind
//                    it.  The thread that owns a tab decodes that field's GT, reading on from global memory (L2-hot: the workgroup
//                    has just loaded it) up to the first ':' or tab and never past end; thread 0 decodes field 0 at beg.  The 2-bit
//                    code goes to codes[l][ordinal] when ordinal < n.  cnt[l] = (fields found, missing, haploid, malformed) by a
//                    workgroup reduction: vector stores only, no atomics.
//   k_vcf_pack ..... codes[lines][n] -> the rows of a SNP-major .bed file, ceil(n/4) bytes each, back to back as in the file: BYTE
//                    stores, as k_bed_decode's reader uses byte loads, since the rows have no alignment.  Unused bit pairs are zero.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

typedef unsigned int vcf_u32x4 __attribute__((ext_vector_type(4)));

#define VCF_LAUNCH_CHECK(ctx)                                               \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

#define VCF_SEG 4096L   // bytes of a line one pass of the workgroup covers: 256 threads x 16

// The GT of the field that starts at text[s]: the bytes up to the first ':' or tab or `end`, cut at every '/' and '|'.  Returns the .bed
// code (hom_ref / hom_alt are the caller's two homozygous codes) and adds to the three counters.  Reads text[s .. end) only.
__device__ __forceinline__ int vcf_decode_gt(const uint8_t* __restrict__ text, long s, long end, int hom_ref, int hom_alt, int& nmiss, int& nhap,
                                             int& nmal) {
    int ntok = 0, len = 0, first = 0, ones = 0;
    bool all01 = true, alldot = true;
    for (long q = s;; q++) {
        int c = -1;   // the GT ends here
        if (q < end) {
            c = text[q];
            if (c == '\t' || c == ':') c = -1;
        }
        if (c < 0 || c == '/' || c == '|') {   // a token closes
            const bool is01 = len == 1 && (first == '0' || first == '1');
            all01 = all01 && is01;
            alldot = alldot && len == 1 && first == '.';
            ones += (is01 && first == '1') ? 1 : 0;
            ntok += ntok < 3 ? 1 : 0;
            len = 0;
            if (c < 0) break;
        } else {
            if (len == 0) first = c;
            len += len < 2 ? 1 : 0;
        }
    }
    if (all01 && ntok == 1) { nhap++; return ones ? hom_alt : hom_ref; }
    if (all01 && ntok == 2) return ones == 0 ? hom_ref : (ones == 2 ? hom_alt : 2);
    nmiss++;
    if (!alldot) nmal++;
    return 1;
}

__global__ __launch_bounds__(256) void k_vcf_fields(const uint8_t* __restrict__ text, const int64_t* __restrict__ table, long n, int hom_ref,
                                                    int hom_alt, uint8_t* __restrict__ codes, int32_t* __restrict__ cnt) {
    __shared__ int wsum[4];
    __shared__ int red[4][3];
    const long line = blockIdx.x;
    const long beg = table[2 * line], end = table[2 * line + 1];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint8_t* const row = codes + line * n;
    int nmiss = 0, nhap = 0, nmal = 0;
    long base = 0;   // tabs of the segments before this one
    if (t == 0) row[0] = (uint8_t)vcf_decode_gt(text, beg, end, hom_ref, hom_alt, nmiss, nhap, nmal);   // n >= 1
    for (long seg = beg & ~15L; seg < end; seg += VCF_SEG) {   // uniform over the workgroup
        const long p = seg + 16 * t;
        unsigned mask = 0;
        if (p < end) {
            const vcf_u32x4 v = *(const vcf_u32x4*)(text + p);
#pragma unroll
            for (int w = 0; w < 4; w++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (((v[w] >> (8 * j)) & 0xffu) == 9u) mask |= 1u << (4 * w + j);
            const int lo = beg > p ? (int)(beg - p) : 0;               // < 16: seg starts in beg's 16 bytes
            const int hi = end - p < 16 ? (int)(end - p) : 16;         // >= 1
            mask &= ((1u << hi) - 1u) & ~((1u << lo) - 1u);
        }
        const int c = __popc(mask);
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(incl, o, 64);
            if (lane >= o) incl += u;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int wbase = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int s = wsum[w];
            wbase += w < wave ? s : 0;
            tot += s;
        }
        __syncthreads();   // wsum is written again in the next segment
        long ord = base + wbase + (incl - c);   // tabs in front of this thread's bytes = the ordinal of the field they lie in
        while (mask) {
            const int i = __ffs(mask) - 1;
            mask &= mask - 1;
            ord++;
            const int code = vcf_decode_gt(text, p + i + 1, end, hom_ref, hom_alt, nmiss, nhap, nmal);
            if (ord < n) row[ord] = (uint8_t)code;
        }
        base += tot;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nmiss += __shfl_xor(nmiss, o, 64);
        nhap += __shfl_xor(nhap, o, 64);
        nmal += __shfl_xor(nmal, o, 64);
    }
    if (lane == 0) { red[wave][0] = nmiss; red[wave][1] = nhap; red[wave][2] = nmal; }
    __syncthreads();
    if (t < 4) {
        const long fields = base + 1;
        int v = fields > 0x7fffffffL ? 0x7fffffff : (int)fields;
        if (t > 0) v = red[0][t - 1] + red[1][t - 1] + red[2][t - 1] + red[3][t - 1];
        cnt[4 * line + t] = v;
    }
}

__global__ __launch_bounds__(256) void k_vcf_pack(const uint8_t* __restrict__ codes, long lines, long n, long rb, uint8_t* __restrict__ bed) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= lines * rb) return;
    const long line = i / rb, j = i - line * rb;
    const uint8_t* r = codes + line * n + 4 * j;
    const int m = n - 4 * j < 4 ? (int)(n - 4 * j) : 4;
    unsigned b = 0;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (q < m) b |= (unsigned)(r[q] & 3u) << (2 * q);
    bed[i] = (uint8_t)b;
}

// text: the staged window (device), readable up to the next multiple of 16 behind the largest table entry; table[2 lines] int64 (device);
// codes: lines x n bytes of scratch; cnt: lines x 4 int32.  a2_alt: EAGLE_VCF_A2_ALT set.
extern "C" int eagle_dev_vcf_fields(eagle_ctx* ctx, const uint8_t* text, const int64_t* table, long lines, long n, int a2_alt, uint8_t* codes,
                                    int32_t* cnt, void* stream) {
    if (lines <= 0) return EAGLE_OK;
    if (n <= 0 || lines > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "eagle_dev_vcf_fields: n must be positive, lines below 2^31");
    const int hom_ref = a2_alt ? 0 : 3, hom_alt = a2_alt ? 3 : 0;
    hipLaunchKernelGGL(k_vcf_fields, dim3((unsigned)lines), dim3(256), 0, (hipStream_t)stream, text, table, n, hom_ref, hom_alt, codes, cnt);
    VCF_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

extern "C" int eagle_dev_vcf_pack(eagle_ctx* ctx, const uint8_t* codes, long lines, long n, uint8_t* bed, void* stream) {
    if (lines <= 0) return EAGLE_OK;
    const long rb = (n + 3) / 4, blocks = (lines * rb + 255) / 256;
    if (n <= 0 || blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "eagle_dev_vcf_pack: n must be positive, lines x ceil(n/4) below 2^39");
    hipLaunchKernelGGL(k_vcf_pack, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, codes, lines, n, rb, bed);
    VCF_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}
