// eagle_qc.hip -- marker QC on the device: per-marker genotype counts and the row compaction of a marker subset.  All three kernels
// are HBM-bound streaming passes with integer arithmetic only (the statistics are made from the counts on the host, in fp64).
//
//   k_marker_counts ....... the int8 marker-major image Mt8 (rows x ld, values -1/0/+1, zero padding) -> int32 counts[rows][3] =
//                           (n0, n1, n2), the numbers of '0', '1', '2' characters of the marker's line.  Per row s = sum g and
//                           q = sum g^2 (v_dot4_i32_i8 against 0x01010101 and against the row itself), then n2 = (q + s) / 2,
//                           n0 = (q - s) / 2, n1 = n - n0 - n2: the zero padding adds to neither sum and needs no mask.
//   k_bed_marker_counts ... raw SNP-major .bed rows (ceil(n/4) bytes per marker, individual 4b+q at bits 2q of byte b) -> int32
//                           counts[rows][4] = (hom A1, het, hom A2, missing), popcounts on dwords of the two bit planes.
//   k_gather_rows_i8 ...... out[r] = src[map[r]] for r < nrows, zero rows up to rows_out: the Mt image of a marker subset.
//
// A row is owned by G = 16, 32 or 64 consecutive lanes of one wave (16 for the shortest rows, so that a 256-byte row does not idle
// three quarters of a wave); the G partial sums meet in a butterfly (__shfl_xor), after which every lane of the group holds the
// row's totals and lanes 0 .. 2 (0 .. 3) store one count each: vector stores only, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

typedef int qc_i32x4 __attribute__((ext_vector_type(4)));

#define QC_LAUNCH_CHECK(ctx)                                                \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

// lanes per row: the largest of 16, 32, 64 that the row's 16-byte (4-byte for .bed rows) pieces keep busy
static inline int qc_group(long pieces) { return pieces <= 16 ? 16 : (pieces <= 32 ? 32 : 64); }

template <int G>
__device__ __forceinline__ int qc_group_sum(int v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// nb16: 16-byte pieces read of every row = ceil(n / 16) (the bytes behind them are padding: zero)
template <int G>
__global__ __launch_bounds__(256) void k_marker_counts(const int8_t* __restrict__ Mt8, long rows, long n, long ld, long nb16,
                                                       int32_t* __restrict__ counts) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long row = t / G;
    const int lane = (int)(t % G);
    int s = 0, q = 0;
    if (row < rows) {
        const qc_i32x4* p = (const qc_i32x4*)(Mt8 + row * ld);
        long c = lane;
        for (; c + 3 * G < nb16; c += 4 * G) {  // four loads in flight per lane
            qc_i32x4 v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = __builtin_nontemporal_load(p + c + k * G);
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    s = __builtin_amdgcn_sdot4(v[k][j], 0x01010101, s, false);
                    q = __builtin_amdgcn_sdot4(v[k][j], v[k][j], q, false);
                }
        }
        for (; c < nb16; c += G) {
            const qc_i32x4 v = __builtin_nontemporal_load(p + c);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s = __builtin_amdgcn_sdot4(v[j], 0x01010101, s, false);
                q = __builtin_amdgcn_sdot4(v[j], v[j], q, false);
            }
        }
    }
    s = qc_group_sum<G>(s);
    q = qc_group_sum<G>(q);
    if (row < rows && lane < 3) {
        const int n2 = (q + s) >> 1, n0 = (q - s) >> 1;
        counts[row * 3 + lane] = lane == 0 ? n0 : (lane == 1 ? (int)n - n0 - n2 : n2);
    }
}

// The rows are BYTE-LOADED like k_bed_decode's: rb = ceil(n/4) has no alignment and the rows lie back to back as in the file.
template <int G>
__global__ __launch_bounds__(256) void k_bed_marker_counts(const uint8_t* __restrict__ bed, long rb, long rows, long n,
                                                           int32_t* __restrict__ counts) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long row = t / G;
    const int lane = (int)(t % G);
    int het = 0, hom2 = 0, miss = 0;
    if (row < rows) {
        const uint8_t* s = bed + row * rb;
        for (long b0 = 4L * lane; b0 < rb; b0 += 4L * G) {
            uint32_t x = 0;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (b0 + k < rb) x |= (uint32_t)s[b0 + k] << (8 * k);
            const long left = n - 4 * b0;                     // individuals of the file among this dword's 16 fields (> 0)
            if (left < 16) x &= (1u << (2 * left)) - 1u;      // the unused bit pairs of the row's last byte
            const uint32_t lo = x & 0x55555555u, hi = (x >> 1) & 0x55555555u;
            miss += __popc(lo & ~hi);                         // 01
            het += __popc(hi & ~lo);                          // 10
            hom2 += __popc(lo & hi);                          // 11
        }
    }
    het = qc_group_sum<G>(het);
    hom2 = qc_group_sum<G>(hom2);
    miss = qc_group_sum<G>(miss);
    if (row < rows && lane < 4) {
        const int hom1 = (int)n - het - hom2 - miss;          // 00 among the n fields of the file
        counts[row * 4 + lane] = lane == 0 ? hom1 : (lane == 1 ? het : (lane == 2 ? hom2 : miss));
    }
}

// one lane = 16 bytes of one output row; lanes16 = ld_out / 16
__global__ __launch_bounds__(256) void k_gather_rows_i8(const int8_t* __restrict__ src, long ld_src, const int32_t* __restrict__ map,
                                                        long nrows, long rows_out, int8_t* __restrict__ out, long ld_out, long lanes16) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows_out * lanes16) return;
    const long r = t / lanes16, c16 = (t - r * lanes16) * 16;
    qc_i32x4 v = {0, 0, 0, 0};
    if (r < nrows && c16 < ld_src) v = __builtin_nontemporal_load((const qc_i32x4*)(src + (long)map[r] * ld_src + c16));
    *(qc_i32x4*)(out + r * ld_out + c16) = v;
}

extern "C" int eagle_dev_marker_counts(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, int32_t* counts, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (n <= 0 || n > ld || ld % 16 || ((uintptr_t)Mt8 & 15) || n > 0x3fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "marker_counts: bad image shape");
    const long nb16 = (n + 15) / 16;
    const int G = qc_group(nb16);
    const long blocks = (rows * G + 255) / 256;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "marker_counts: too many rows");
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t s = (hipStream_t)stream;
    if (G == 16) hipLaunchKernelGGL(k_marker_counts<16>, grid, blk, 0, s, Mt8, rows, n, ld, nb16, counts);
    else if (G == 32) hipLaunchKernelGGL(k_marker_counts<32>, grid, blk, 0, s, Mt8, rows, n, ld, nb16, counts);
    else hipLaunchKernelGGL(k_marker_counts<64>, grid, blk, 0, s, Mt8, rows, n, ld, nb16, counts);
    QC_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

extern "C" int eagle_dev_bed_marker_counts(eagle_ctx* ctx, const uint8_t* bed, long rows, long n, int32_t* counts, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (n <= 0 || n > 0x3fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_marker_counts: bad shape");
    const long rb = bed_row_bytes(n);
    const int G = qc_group((rb + 3) / 4);
    const long blocks = (rows * G + 255) / 256;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_marker_counts: too many rows");
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t s = (hipStream_t)stream;
    if (G == 16) hipLaunchKernelGGL(k_bed_marker_counts<16>, grid, blk, 0, s, bed, rb, rows, n, counts);
    else if (G == 32) hipLaunchKernelGGL(k_bed_marker_counts<32>, grid, blk, 0, s, bed, rb, rows, n, counts);
    else hipLaunchKernelGGL(k_bed_marker_counts<64>, grid, blk, 0, s, bed, rb, rows, n, counts);
    QC_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// out (rows_out x ld_out) = the rows map[0 .. nrows) of src (every map[r] a row of src), then zero rows; columns beyond ld_src zero.
extern "C" int eagle_dev_gather_rows_i8(eagle_ctx* ctx, const int8_t* src, long ld_src, const int32_t* map, long nrows, long rows_out,
                                        int8_t* out, long ld_out, void* stream) {
    if (rows_out <= 0) return EAGLE_OK;
    if (nrows < 0 || nrows > rows_out || ld_src % 16 || ld_out % 16 || (((uintptr_t)src | (uintptr_t)out) & 15))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "gather_rows_i8: bad shape");
    const long lanes16 = ld_out / 16, blocks = (rows_out * lanes16 + 255) / 256;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "gather_rows_i8: too many rows");
    hipLaunchKernelGGL(k_gather_rows_i8, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, ld_src, map, nrows, rows_out, out,
                       ld_out, lanes16);
    QC_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}
