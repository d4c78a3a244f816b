// eagle_qc.hip -- marker and sample QC on the device: genotype counts per marker and per individual, the row compaction of a marker
// subset, the finish of the pairwise IBS counts and the Hardy-Weinberg exact test.  The counting kernels are HBM-bound streaming passes
// with integer arithmetic only (the statistics are made from the counts on the host, in fp64); k_hwe_exact is the one fp64 kernel.
//
//   k_marker_counts ....... the int8 marker-major image Mt8 (rows x ld, values -1/0/+1, zero padding) -> int32 counts[rows][3] =
//                           (n0, n1, n2), the numbers of '0', '1', '2' characters of the marker's line.  Per row s = sum g and
//                           q = sum g^2 (v_dot4_i32_i8 against 0x01010101 and against the row itself), then n2 = (q + s) / 2,
//                           n0 = (q - s) / 2, n1 = n - n0 - n2: the zero padding adds to neither sum and needs no mask.
//   k_bed_marker_counts ... raw SNP-major .bed rows (ceil(n/4) bytes per marker, individual 4b+q at bits 2q of byte b) -> int32
//                           counts[rows][4] = (hom A1, het, hom A2, missing), popcounts on dwords of the two bit planes.
//   k_gather_rows_i8 ...... out[r] = src[map[r]] for r < nrows, zero rows up to rows_out: the Mt image of a marker subset.
//   k_bed_sample_counts ... the same raw .bed rows -> int32 counts[n][4] per INDIVIDUAL, added to what the array holds (the column
//                           reduction of the rows k_bed_marker_counts reduces along).
//   k_ibs_finish .......... the int32 Gram accumulators D = M M^T and Q = (M o M)(M o M)^T (upper 256-tiles live) and L -> the full
//                           symmetric int32 matrices ibs0 = (Q - D) / 2 and hethet = L - Q_ii - Q_jj + Q_ij.
//   k_hwe_exact ........... int32 counts[L][stride] -> the exact Hardy-Weinberg p-value of every marker, one marker per thread.
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

// ------------------------------------------------------------------------------------------------------------------------------
// Per-individual counts of raw .bed rows.  A thread owns one byte column (four individuals) of a chunk of BSC_ROWS rows: consecutive
// lanes read consecutive bytes of a row (byte loads: rows have no alignment).  The three code planes of a byte -- bits 0, 2, 4, 6 of
// lo & ~hi (missing), hi & ~lo (het), lo & hi (hom A2) -- are spread to bits 0, 8, 16, 24 of a dword and added there, four 8-bit
// counters per plane, which are flushed into 32-bit counters every 255 rows.  hom A1 = rows of the chunk - the other three.  The
// chunk's sixteen totals are added to counts[n][4] with integer atomics: integer sums, so the result does not depend on the order.
// ------------------------------------------------------------------------------------------------------------------------------
#define BSC_ROWS 1020   // rows per block: 4 x 255
__device__ __forceinline__ uint32_t bsc_spread(uint32_t x) { return (x | (x << 6) | (x << 12) | (x << 18)) & 0x01010101u; }

__global__ __launch_bounds__(256) void k_bed_sample_counts(const uint8_t* __restrict__ bed, long rb, long rows, long n,
                                                           int32_t* __restrict__ counts) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;     // byte column
    if (b >= rb) return;
    const long r0 = (long)blockIdx.y * BSC_ROWS, r1 = r0 + BSC_ROWS < rows ? r0 + BSC_ROWS : rows;
    const long left = n - 4 * b;                              // individuals of the file among this byte's four fields (> 0)
    const uint32_t keep = left < 4 ? (1u << (2 * left)) - 1u : 0xffu;   // the unused bit pairs of a row's last byte are cleared
    int het[4] = {0, 0, 0, 0}, hom2[4] = {0, 0, 0, 0}, miss[4] = {0, 0, 0, 0};
    for (long ra = r0; ra < r1; ra += 255) {
        const long rbnd = ra + 255 < r1 ? ra + 255 : r1;
        uint32_t ph = 0, p2 = 0, pm = 0;
        const uint8_t* s = bed + ra * rb + b;
        for (long r = ra; r < rbnd; r++, s += rb) {
            const uint32_t x = (uint32_t)*s & keep;
            const uint32_t lo = x & 0x55u, hi = (x >> 1) & 0x55u;
            pm += bsc_spread(lo & ~hi);
            ph += bsc_spread(hi & ~lo);
            p2 += bsc_spread(lo & hi);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            het[q] += (int)((ph >> (8 * q)) & 0xffu);
            hom2[q] += (int)((p2 >> (8 * q)) & 0xffu);
            miss[q] += (int)((pm >> (8 * q)) & 0xffu);
        }
    }
    const int nr = (int)(r1 - r0);
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (q < left) {
            int32_t* c = counts + (4 * b + q) * 4;
            atomicAdd(c + 0, nr - het[q] - hom2[q] - miss[q]);
            atomicAdd(c + 1, het[q]);
            atomicAdd(c + 2, hom2[q]);
            atomicAdd(c + 3, miss[q]);
        }
}

// counts[n][4] (caller-zeroed before the first window of a file) += the counts of the individuals over `rows` raw .bed rows
extern "C" int eagle_dev_bed_sample_counts(eagle_ctx* ctx, const uint8_t* bed, long rows, long n, int32_t* counts, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (n <= 0 || n > 0x3fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_sample_counts: bad shape");
    const long rb = bed_row_bytes(n), chunks = (rows + BSC_ROWS - 1) / BSC_ROWS;
    if (chunks > 65535) return eagle_fail(ctx, EAGLE_ERR_ARG, "bed_sample_counts: too many rows in one window");
    hipLaunchKernelGGL(k_bed_sample_counts, dim3((unsigned)((rb + 255) / 256), (unsigned)chunks), dim3(256), 0, (hipStream_t)stream, bed, rb,
                       rows, n, counts);
    QC_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// One block per 32 x 32 tile on or above the diagonal (the tiling of k_mmt_finish): coalesced reads of the two int32 accumulators,
// coalesced writes of the two results and, through LDS, of their mirror images.  q_i = Q_ii lies in a diagonal 256-tile, which is live.
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ibs_finish(const int32_t* __restrict__ D, const int32_t* __restrict__ Q, long n, long ldc, int L,
                                                    int32_t* __restrict__ ibs0, int32_t* __restrict__ hethet) {
    const long bi = (long)blockIdx.y * 32, bj = (long)blockIdx.x * 32;
    if (bj < bi) return;
    __shared__ int32_t t0[32][33], t1[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long j = bj + tx;
    const int qj = j < n ? Q[j * ldc + j] : 0;
    for (int r = ty; r < 32; r += 8) {
        const long i = bi + r;
        int a = 0, h = 0;
        if (i < n && j < n) {
            const int q = Q[i * ldc + j], d = D[i * ldc + j];
            a = (q - d) >> 1;                       // opposite homozygotes: the difference is even and not negative
            h = L - Q[i * ldc + i] - qj + q;        // both heterozygous
            ibs0[i * n + j] = a;
            hethet[i * n + j] = h;
        }
        t0[r][tx] = a;
        t1[r][tx] = h;
    }
    __syncthreads();
    if (bj > bi)
        for (int r = ty; r < 32; r += 8) {
            const long jj = bj + r, ii = bi + tx;   // out[jj][ii] = the value at (ii, jj)
            if (ii < n && jj < n) {
                ibs0[jj * n + ii] = t0[tx][r];
                hethet[jj * n + ii] = t1[tx][r];
            }
        }
}

extern "C" int eagle_dev_ibs_finish(eagle_ctx* ctx, const int32_t* D32, const int32_t* Q32, long n, long n_pad, long L, int32_t* ibs0,
                                    int32_t* hethet, void* stream) {
    if (n <= 0 || n > n_pad || n_pad % 256 || L <= 0 || L > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "ibs_finish: bad shape");
    const unsigned nb = (unsigned)((n + 31) / 32);
    hipLaunchKernelGGL(k_ibs_finish, dim3(nb, nb), dim3(256), 0, (hipStream_t)stream, D32, Q32, n, n_pad, (int)L, ibs0, hethet);
    QC_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Hardy-Weinberg exact test, in the order the sample-QC section of eagle_hip.h fixes: every product, quotient and sum below is one
// correctly rounded fp64 operation (__dmul_rn / __ddiv_rn / __dadd_rn: nothing is contracted into an FMA), the integer factors are
// exact int64 products converted once.  hwe_walk visits mid first, then the leg below it (h = mid - 2, mid - 4, ...), then the leg
// above: with cut < 0 it returns the total and leaves P(n_AB) in *p_obs; with cut >= 0 it returns the sum of the terms <= cut, in the
// same order.  Two walks per marker and no array.  One marker per thread: the lanes of a wave run as long as their longest marker.
// ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double hwe_walk(long mid, long hr0, long hc0, long r, long n_ab, double cut, double* p_obs) {
    const bool tail = cut >= 0.0;
    double sum = (!tail || 1.0 <= cut) ? 1.0 : 0.0;
    double pobs = 1.0;                                   // P(mid): the value if n_AB == mid
    double p = 1.0;
    long a = hr0, b = hc0;
    for (long h = mid; h >= 2; h -= 2) {                 // P(h - 2) = P(h) h (h - 1) / (4 (hr + 1) (hc + 1))
        p = __ddiv_rn(__dmul_rn(p, (double)(h * (h - 1))), (double)(4 * (a + 1) * (b + 1)));
        a++; b++;
        if (h - 2 == n_ab) pobs = p;
        if (!tail || p <= cut) sum = __dadd_rn(sum, p);
    }
    p = 1.0; a = hr0; b = hc0;
    for (long h = mid; h <= r - 2; h += 2) {             // P(h + 2) = P(h) 4 hr hc / ((h + 2) (h + 1))
        p = __ddiv_rn(__dmul_rn(p, (double)(4 * a * b)), (double)((h + 2) * (h + 1)));
        a--; b--;
        if (h + 2 == n_ab) pobs = p;
        if (!tail || p <= cut) sum = __dadd_rn(sum, p);
    }
    if (p_obs) *p_obs = pobs;
    return sum;
}

__global__ __launch_bounds__(256) void k_hwe_exact(const int32_t* __restrict__ counts, long L, int stride, double* __restrict__ pout) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= L) return;
    const long n_aa = counts[m * stride], n_ab = counts[m * stride + 1], n_bb = counts[m * stride + 2];
    const long N = n_aa + n_ab + n_bb;
    if (N == 0) { pout[m] = 1.0; return; }
    const long hr = n_aa < n_bb ? n_aa : n_bb;
    const long r = 2 * hr + n_ab;                        // copies of the rare allele
    long mid = r * (2 * N - r) / (2 * N);                // floor of the expected heterozygotes, then up to the parity of r
    if ((mid ^ r) & 1) mid++;
    const long hr0 = (r - mid) / 2, hc0 = N - mid - hr0;
    double pobs;
    const double total = hwe_walk(mid, hr0, hc0, r, n_ab, -1.0, &pobs);
    const double tail = hwe_walk(mid, hr0, hc0, r, n_ab, pobs, nullptr);
    const double pv = __ddiv_rn(tail, total);
    pout[m] = pv > 1.0 ? 1.0 : pv;
}

// counts: device int32 [L][stride], stride 3 or 4, every count >= 0 and every row sum <= 2^30 (the caller's check)
extern "C" int eagle_dev_hwe_exact(eagle_ctx* ctx, const int32_t* counts, long L, int stride, double* p, void* stream) {
    if (L <= 0) return EAGLE_OK;
    if (stride != 3 && stride != 4) return eagle_fail(ctx, EAGLE_ERR_ARG, "hwe_exact: stride must be 3 or 4");
    const long blocks = (L + 255) / 256;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "hwe_exact: too many markers");
    hipLaunchKernelGGL(k_hwe_exact, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, counts, L, stride, p);
    QC_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}
