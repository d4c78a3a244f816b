// eagle_tdt.hip -- transmission disequilibrium test of parent-offspring trios (include/eagle_hip.h section 1b''''viii) on the bit planes
// of eagle_ibd.hip with the trio lists of eagle_mendel.hip.  Integer arithmetic but for the two fp64 operations of the key; plain HIP, no
// inline assembly.  The product of the flips, count1 and the per-flip maxima are k_maxt_tile / k_maxt_finish of eagle_maxt.hip.
//
//   k_tdt_trios<MARK> . one lane per trio, 64 list entries per wave, the three individuals gathered by index as in k_mendel_trios.  The
//                       lanes walk the words, form the words of rule 2 (tdt_words, eagle_host.h) and add eight popcounts into the six
//                       per-trio counts.  MARK: for each of the five kinds PT, PU, MT, MU, W the wave turns its 64 words into 64 per-bit
//                       totals by one ballot and one popcount per bit -- lane b keeps the total of bit b -- and adds them to marker[5 x +
//                       kind] with one 32-bit atomic per lane; a kind whose word is zero in every lane is skipped.  Nothing goes through
//                       LDS.  Lanes past the list hold zero words; bits past the last marker are masked through C.
//   k_tdt_finish ...... (PT, PU, MT, MU, W) of a marker -> d_obs = T - U, V = T + U, key_obs = fl(fl(d d) / V) or 0 where V = 0.
//   k_tdt_image ....... a wave takes 64 trios x one plane word (64 markers): every lane forms its trio's words, writes d of rule 2 for the
//                       64 markers as bytes into a 64 x 64 LDS tile (row = marker, column = trio: the 64 lanes write 64 consecutive
//                       bytes), and the wave stores the tile's rows as 16-byte pieces along the trio dimension of the marker-major image.
//                       Trios from T on are zero bytes; every byte of the band's rows up to ld is written.
//   k_tdt_signs ....... one thread = 16 trios of one flip: the bytes +-1 of rule 5 (tdt_sign, eagle_host.h), zeros from T on.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

typedef int tdt_i32x4 __attribute__((ext_vector_type(4)));

#define TDT_LAUNCH_CHECK(ctx)                                               \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

// The words of rule 2 of trio (c, f, m) at plane word w; f, m < 0: an unknown parent, whose words are zero.  live = false: all zero.
__device__ __forceinline__ TdtWords tdt_load(const uint64_t* __restrict__ A, const uint64_t* __restrict__ B, const uint64_t* __restrict__ Cc, long np,
                                             long L, long w, long c, long f, long m, bool live) {
    const long o = w * np, fi = f < 0 ? 0 : f, mi = m < 0 ? 0 : m;   // an unknown parent reads individual 0 and drops the words
    const uint64_t valid = mendel_word_mask(w, L);
    uint64_t ac = A[o + c], bc = B[o + c], cc = Cc ? Cc[o + c] : valid;
    uint64_t af = A[o + fi], bf = B[o + fi], cf = Cc ? Cc[o + fi] : valid;
    uint64_t am = A[o + mi], bm = B[o + mi], cm = Cc ? Cc[o + mi] : valid;
    if (f < 0) af = bf = cf = 0;
    if (m < 0) am = bm = cm = 0;
    if (!live) cc = 0;                                                // K = 0: every word of the trio is zero
    return tdt_words(ac, bc, cc & valid, af, bf, cf, am, bm, cm);
}

// trios: T x 3 int32 (child, father, mother; a parent may be -1).  out: T x 6 int32.  marker: L x 5 int32, zeroed by the caller (MARK).
template <bool MARK>
__global__ __launch_bounds__(64) void k_tdt_trios(const uint64_t* __restrict__ A, const uint64_t* __restrict__ B, const uint64_t* __restrict__ Cc, long np,
                                                  long L, long nwords, const int32_t* __restrict__ trios, long T, int32_t* __restrict__ out,
                                                  int32_t* __restrict__ marker) {
    const int lane = threadIdx.x;
    const long t = 64 * (long)blockIdx.x + lane;
    const bool live = t < T;
    const long c = live ? trios[3 * t] : 0, f = live ? trios[3 * t + 1] : -1, m = live ? trios[3 * t + 2] : -1;
    int n_k = 0, n_hf = 0, n_hm = 0, n_t = 0, n_u = 0, n_w = 0;
    for (long w = 0; w < nwords; w++) {
        const TdtWords x = tdt_load(A, B, Cc, np, L, w, c, f, m, live);
        const int pw = __popcll(x.w);
        n_k += __popcll(x.k);
        n_hf += __popcll(x.hf);
        n_hm += __popcll(x.hm);
        n_t += __popcll(x.pt) + __popcll(x.mt) + pw;
        n_u += __popcll(x.pu) + __popcll(x.mu) + pw;
        n_w += pw;
        if (MARK) {
            const uint64_t kind[5] = {x.pt, x.pu, x.mt, x.mu, x.w};
            const long at = 64 * w + lane;
#pragma unroll
            for (int q = 0; q < 5; q++) {
                if (__ballot(kind[q] != 0) == 0) continue;   // wave-uniform
                int mine = 0;
#pragma unroll 8
                for (int b = 0; b < 64; b++) {
                    const int cnt = __popcll(__ballot((kind[q] >> b) & 1ull));
                    if (lane == b) mine = cnt;
                }
                if (mine > 0 && at < L) atomicAdd(marker + 5 * at + q, mine);
            }
        }
    }
    if (live) {
        int32_t* row = out + 6 * t;
        row[0] = n_k; row[1] = n_hf; row[2] = n_hm; row[3] = n_t; row[4] = n_u; row[5] = n_w;
    }
}

__global__ __launch_bounds__(256) void k_tdt_finish(const int32_t* __restrict__ marker, long L, int64_t* __restrict__ dobs, int64_t* __restrict__ V,
                                                    double* __restrict__ keyobs) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= L) return;
    const int32_t* r = marker + 5 * m;
    const long tt = (long)r[0] + r[2] + r[4], uu = (long)r[1] + r[3] + r[4];
    const long d = tt - uu, v = tt + uu;
    const double dd = (double)d;
    dobs[m] = d;
    V[m] = v;
    keyobs[m] = v ? __ddiv_rn(__dmul_rn(dd, dd), (double)v) : 0.0;
}

// img: rows x ld int8, row r = marker m0 + r.  blockIdx.x = word of the band * tgroups + trio group; w0 = m0 / 64.
__global__ __launch_bounds__(64) void k_tdt_image(const uint64_t* __restrict__ A, const uint64_t* __restrict__ B, const uint64_t* __restrict__ Cc, long np,
                                                  long L, const int32_t* __restrict__ trios, long T, long w0, long rows, long tgroups,
                                                  int8_t* __restrict__ img, long ld) {
    __shared__ __attribute__((aligned(16))) int8_t tile[64 * 64];
    const int lane = threadIdx.x;
    const long wb = (long)blockIdx.x / tgroups, tg = (long)blockIdx.x - wb * tgroups;
    const long t = 64 * tg + lane;
    const bool live = t < T;
    const long c = live ? trios[3 * t] : 0, f = live ? trios[3 * t + 1] : -1, m = live ? trios[3 * t + 2] : -1;
    const TdtWords x = tdt_load(A, B, Cc, np, L, w0 + wb, c, f, m, live);
#pragma unroll 8
    for (int b = 0; b < 64; b++) tile[64 * b + lane] = (int8_t)tdt_d_bit(x, b);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int q = lane + 64 * i, b = q >> 2, piece = q & 3;   // four lanes store the 64 bytes of one marker row
        const long r = 64 * wb + b, col = 64 * tg + 16 * piece;
        if (r < rows && col < ld) *(tdt_i32x4*)(img + r * ld + col) = *(const tdt_i32x4*)(tile + 64 * b + 16 * piece);
    }
}

// op: [R][ldop] int8; lanes16 = ldop / 16
__global__ __launch_bounds__(256) void k_tdt_signs(const int32_t* __restrict__ fam, long T, uint64_t seed, long first, long R, long lanes16,
                                                   int8_t* __restrict__ op, long ldop) {
    const long x = (long)blockIdx.x * 256 + threadIdx.x;
    if (x >= R * lanes16) return;
    const long rr = x / lanes16, i0 = (x - rr * lanes16) * 16;
    tdt_i32x4 v = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const long t = i0 + j;
        if (t >= T) continue;
        const int8_t s = (int8_t)tdt_sign(seed, (uint64_t)(first + rr), (uint32_t)fam[t]);
        v[j >> 2] |= (int)((unsigned)(uint8_t)s << (8 * (j & 3)));
    }
    *(tdt_i32x4*)(op + rr * ldop + i0) = v;
}

// ------------------------------------------------------------------------------------------------------------------------------
// launchers (device pointers throughout)
// ------------------------------------------------------------------------------------------------------------------------------
static bool tdt_shape_ok(long n, long L, long T, int nplanes) {
    return n >= 1 && L > 0 && L <= 0x7fffffffL && T >= 1 && T <= MENDEL_MAX_TRIOS && (nplanes == 2 || nplanes == 3);
}

// planes: A, B (nplanes 2, the image) or A, B, C (3, the .bed file) of n individuals x L markers.  marker: L x 5 int32, ZEROED by the
// caller, or NULL.
extern "C" int eagle_dev_tdt_trios(eagle_ctx* ctx, const uint64_t* planes, int nplanes, long n, long L, const int32_t* trios, long T, int32_t* out,
                                   int32_t* marker, void* stream) {
    if (!tdt_shape_ok(n, L, T, nplanes)) return eagle_fail(ctx, EAGLE_ERR_ARG, "tdt_trios: bad shape");
    const long np = (n + 63) / 64 * 64, nwords = (L + 63) / 64;
    const size_t plane = (size_t)nwords * (size_t)np;
    const uint64_t* Cc = nplanes == 3 ? planes + 2 * plane : nullptr;
    const dim3 g((unsigned)((T + 63) / 64)), b(64);
    if (marker) hipLaunchKernelGGL((k_tdt_trios<true>), g, b, 0, (hipStream_t)stream, planes, planes + plane, Cc, np, L, nwords, trios, T, out, marker);
    else hipLaunchKernelGGL((k_tdt_trios<false>), g, b, 0, (hipStream_t)stream, planes, planes + plane, Cc, np, L, nwords, trios, T, out, marker);
    TDT_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

extern "C" int eagle_dev_tdt_finish(eagle_ctx* ctx, const int32_t* marker, long L, int64_t* dobs, int64_t* V, double* keyobs, void* stream) {
    if (L <= 0 || L > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "tdt_finish: bad shape");
    hipLaunchKernelGGL(k_tdt_finish, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, (hipStream_t)stream, marker, L, dobs, V, keyobs);
    TDT_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// The rows [m0, m0 + rows) of the image, m0 a multiple of 64 and m0 + rows <= L rounded up to 128; rows past L are zero (their bits are
// masked).  The grid is one-dimensional: words of the band x groups of 64 trios.
extern "C" int eagle_dev_tdt_image(eagle_ctx* ctx, const uint64_t* planes, int nplanes, long n, long L, const int32_t* trios, long T, long m0,
                                   long rows, int8_t* img, long ld, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    const long nwords = (L + 63) / 64, bw = (rows + 63) / 64, tgroups = (ld + 63) / 64;
    if (!tdt_shape_ok(n, L, T, nplanes) || T > TDT_MAX_FLIP_TRIOS || m0 < 0 || m0 % 64 || m0 / 64 + bw > nwords || ld < T || ld % 16 ||
        ((uintptr_t)img & 15))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "tdt_image: bad shape");
    if (bw * tgroups > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "tdt_image: too many blocks");
    const long np = (n + 63) / 64 * 64;
    const size_t plane = (size_t)nwords * (size_t)np;
    const uint64_t* Cc = nplanes == 3 ? planes + 2 * plane : nullptr;
    hipLaunchKernelGGL(k_tdt_image, dim3((unsigned)(bw * tgroups)), dim3(64), 0, (hipStream_t)stream, planes, planes + plane, Cc, np, L, trios, T, m0 / 64,
                       rows, tgroups, img, ld);
    TDT_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

extern "C" int eagle_dev_tdt_signs(eagle_ctx* ctx, const int32_t* fam, long T, uint64_t seed, long first, long R, int8_t* op, long ldop,
                                   void* stream) {
    if (T < 1 || T > TDT_MAX_FLIP_TRIOS || R < 1 || R > MAXT_RMAX || first < 1 || ldop < T || ldop % 16 || ((uintptr_t)op & 15))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "tdt_signs: bad shape");
    const long lanes16 = ldop / 16;
    hipLaunchKernelGGL(k_tdt_signs, dim3((unsigned)((R * lanes16 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fam, T, seed, first, R, lanes16, op,
                       ldop);
    TDT_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}
