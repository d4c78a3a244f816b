// eagle_epi.hip -- epistasis: the additive x additive interaction test between pairs of markers for an integer trait (include/eagle_hip.h
// section 1b''''ii), on the int8 MFMA (v_mfma_i32_32x32x32_i8).  Every sufficient statistic is an exact integer; the statistic itself is
// epi_stat of eagle_host.h, the same function on the device and in the CPU test binary.
//
//   per pair:  d = sum g_i g_j,  e = sum g_i^2 g_j,  f = sum g_i g_j^2,  h = sum g_i^2 g_j^2,  z = sum y g_i g_j
//   per marker (k_epi_marker): s = sum g, q = sum g^2, u = sum y g;  per trait (host): Y = sum y, T = sum y^2
//
// Tile (k_epi_tile).  A workgroup (256 threads, 4 waves) owns one tile pair: 128 A rows x 64 B rows of marker-major int8 images.  Per K
// chunk of 128 individuals it stages the 192 rows x 128 B in LDS once, in the swizzled rows of k_ld_tile (eagle_ld.hip).  Only g is
// staged.  The other operands are made in registers from the 16 bytes a lane has read:
//   g^2      = g & 0x01 in every byte (-1 = 0xff and +1 both give 1)
//   y_p o g  = digit plane p of y where g = +1, the negated plane where g = -1, zero where g = 0: a bytewise select by the masks
//              0xff * (g & 1) and 0xff * ((g >> 7) & 1).  y = d0 + 128 d1 + 128^2 d2 with digits in [-64, 63] (epi_digits), so both the
//              plane and its negative are int8; the six planes (three and their negatives) are read from global memory, 16 bytes a lane,
//              the same address in the 32 lanes of a half wave.
// Wave w multiplies the 32-row block w of A against the two 32-row blocks of B, seven products each (g.g, g^2.g, g.g^2, g^2.g^2 and
// g.(y_p o g), p = 0, 1, 2): 2 x 7 x 16 = 224 int32 accumulator registers a lane, beside 6 x 4 staging registers of the next chunk and the
// operands.  One wave per SIMD has 512.  Static LDS: 192 x 128 B = 24 KB; the epilogue's per-marker sums (192 x 24 B) and the reduction
// scratch lie over the dead tile.  |z_p| <= 64 n < 2^23 and the other sums are at most n: nothing leaves int32.
//
// Epilogue: z = z0 + 128 z1 + 128^2 z2 in int64, then epi_stat (128-bit integers, t53, six correctly rounded fp64 operations).
//   MODE 0 (loci)   stat[i * nloci + j] and mom[(i * nloci + j) * 5 ..] = (d, e, f, h, z) for every A row i and gathered row j < nloci.
//   MODE 1 (count)  per tile pair: the number of hits (stat >= min_stat), of defined pairs and the largest defined stat with its pair
//                   (ties: the smallest (i, j)) among the pairs i < j the gap rule does not skip.  A reduction in registers and LDS; thread
//                   0 stores: every word has one owner.
//   MODE 2 (fill)   the same pairs again for the tile pairs that have hits; a hit takes slot base[tile] + (an LDS counter) of the tables.
//                   The order inside a tile pair is arbitrary -- the host sorts the hits by (i, j) -- but no slot is shared: no global
//                   atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"
#include "eagle_lines.h"

static_assert(EPI_MAX_N == EAGLE_EPI_MAX_N && EPI_YMAX == EAGLE_EPI_YMAX, "eagle_host.h and eagle_hip.h state the same limits");

typedef int epi_i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned epi_u32x4 __attribute__((ext_vector_type(4)));
typedef int epi_i32x16 __attribute__((ext_vector_type(16)));

#define EPI_TM 128   /* A rows per workgroup */
#define EPI_TB 64    /* B rows per workgroup */
#define EPI_BK 128   /* individuals per staged chunk */
#define EPI_ROWS (EPI_TM + EPI_TB)

#define EPI_LAUNCH_CHECK(ctx)                                               \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

// msu[3 r ..] = (s, q, u) of row r: one wave per row, a lane takes 16 bytes at a time.  y: n int32.
__global__ __launch_bounds__(256) void k_epi_marker(const int8_t* __restrict__ Mt8, long rows, long n, long ld, const int32_t* __restrict__ y,
                                                    int64_t* __restrict__ msu) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                          // a whole wave
    long long s = 0, q = 0, u = 0;
    const int8_t* row = Mt8 + r * ld;
    for (long k0 = 16L * lane; k0 < n; k0 += 16 * 64) {
        const epi_i32x4 v = *(const epi_i32x4*)(row + k0);
#pragma unroll
        for (int b = 0; b < 16; b++) {
            const long k = k0 + b;
            if (k < n) {
                const int g = (int)(int8_t)(((unsigned)v[b >> 2] >> (8 * (b & 3))) & 0xffu);
                s += g;
                q += g & 1;
                u += (long long)y[k] * g;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off);
        q += __shfl_xor(q, off);
        u += __shfl_xor(u, off);
    }
    if (lane == 0) {
        msu[3 * r] = s;
        msu[3 * r + 1] = q;
        msu[3 * r + 2] = u;
    }
}

// (stat, i, j) b beats a: a has no pair yet, or b's stat is larger, or it ties with the smaller (i, j).  Neither stat is NaN.
__device__ __forceinline__ bool epi_beats(double sa, long ia, long ja, double sb, long ib, long jb) {
    if (ib < 0) return false;
    if (ia < 0) return true;
    return sb > sa || (sb == sa && (ib < ia || (ib == ia && jb < ja)));
}

struct EpiOut {
    // loci mode
    int nloci;
    double* stat;
    int64_t* mom;
    // pairs mode
    const int32_t* chrom;
    long gap;
    double min_stat;
    int32_t* tcount;        // 2 per tile pair: hits, defined
    double* tmax;           // 1 per tile pair
    int32_t* tmaxij;        // 2 per tile pair (-1, -1: none)
    const int64_t* base;    // fill: first slot of the tile pair
    int32_t* hit_ij;
    double* hit_stat;
    int64_t* hit_mom;
};

// A8: rowsA x ld, B8: rowsB x ldB, both zero from individual n on up to kbytes = ceil16(n); tiles[2 x] = (A tile of 128 rows, B tile of 64
// rows) of workgroup x; ydig: six planes of kpad bytes (digit 0, 1, 2 of y, then their negatives), zero from n on, kpad a multiple of 128
// at or beyond kbytes; msuA / msuB: (s, q, u) of the rows of A8 / B8.
template <int MODE>
__global__ __launch_bounds__(256) void k_epi_tile(const int8_t* __restrict__ A8, long rowsA, long ld, const int8_t* __restrict__ B8, long rowsB,
                                                  long ldB, long kbytes, const int32_t* __restrict__ tiles, const int8_t* __restrict__ ydig,
                                                  long kpad, EpiTrait trait, const int64_t* __restrict__ msuA, const int64_t* __restrict__ msuB,
                                                  EpiOut o) {
    constexpr int NCH = EPI_ROWS / 32;   // 16-byte pieces per thread and chunk
    __shared__ __attribute__((aligned(16))) int8_t tile[EPI_ROWS * EPI_BK];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const long arow0 = (long)tiles[2 * blockIdx.x] * EPI_TM, brow0 = (long)tiles[2 * blockIdx.x + 1] * EPI_TB;

    epi_i32x4 pre[NCH];
    auto fetch = [&](long k0) {
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int idx = tid + 256 * i, rr = idx >> 3;
            const long kb = k0 + 16 * (idx & 7);
            epi_i32x4 v = {0, 0, 0, 0};
            if (kb < kbytes) {
                if (rr >= EPI_TM) {
                    if (brow0 + (rr - EPI_TM) < rowsB) v = *(const epi_i32x4*)(B8 + (brow0 + (rr - EPI_TM)) * ldB + kb);
                } else if (arow0 + rr < rowsA) {
                    v = *(const epi_i32x4*)(A8 + (arow0 + rr) * ld + kb);
                }
            }
            pre[i] = v;
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int idx = tid + 256 * i, rr = idx >> 3, c = idx & 7;
            *(epi_i32x4*)(tile + rr * EPI_BK + ((c ^ ((rr >> 1) & 7)) << 4)) = pre[i];
        }
    };

    epi_i32x16 acc[2][7];
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
        for (int p = 0; p < 7; p++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[b][p][e] = 0;

    const int8_t* pa = tile + (32 * w + r) * EPI_BK;
    const int8_t* pb = tile + (EPI_TM + r) * EPI_BK;
    const int swz = (r >> 1) & 7;
    const epi_u32x4 one = {0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u};

    fetch(0);
    for (long k0 = 0; k0 < kbytes; k0 += EPI_BK) {
        put();
        __syncthreads();
        if (k0 + EPI_BK < kbytes) fetch(k0 + EPI_BK);
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
            const int lc = 2 * ks + h, ch = (lc ^ swz) << 4;
            const long ky = k0 + 16 * lc;                          // < kpad: kpad is a multiple of 128 at or beyond kbytes
            epi_u32x4 yp[3], yn[3];
#pragma unroll
            for (int p = 0; p < 3; p++) {
                yp[p] = *(const epi_u32x4*)(ydig + p * kpad + ky);
                yn[p] = *(const epi_u32x4*)(ydig + (3 + p) * kpad + ky);
            }
            const epi_u32x4 ua = *(const epi_u32x4*)(pa + ch);
            const epi_i32x4 a = (epi_i32x4)ua, a2 = (epi_i32x4)(ua & one);
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const epi_u32x4 ub = *(const epi_u32x4*)(pb + b * (32 * EPI_BK) + ch);
                const epi_u32x4 mnz = (ub & one) * 0xffu, mneg = ((ub >> 7) & one) * 0xffu, mpos = mnz & ~mneg;
                const epi_i32x4 bb = (epi_i32x4)ub, b2 = (epi_i32x4)(ub & one);
                acc[b][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bb, acc[b][0], 0, 0, 0);
                acc[b][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a2, bb, acc[b][1], 0, 0, 0);
                acc[b][2] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b2, acc[b][2], 0, 0, 0);
                acc[b][3] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a2, b2, acc[b][3], 0, 0, 0);
#pragma unroll
                for (int p = 0; p < 3; p++) {
                    const epi_i32x4 yg = (epi_i32x4)((yp[p] & mpos) | (yn[p] & mneg));
                    acc[b][4 + p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, yg, acc[b][4 + p], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // the tile is dead: (s, q, u) of its 192 rows, then the reduction scratch
    int64_t* sM = (int64_t*)tile;                                   // EPI_ROWS x 3 int64
    for (int x = tid; x < EPI_ROWS * 3; x += 256) {
        const int rr = x / 3, c = x - 3 * rr;
        int64_t v = 0;
        if (rr < EPI_TM) {
            if (arow0 + rr < rowsA) v = msuA[3 * (arow0 + rr) + c];
        } else if (brow0 + (rr - EPI_TM) < rowsB) {
            v = msuB[3 * (brow0 + (rr - EPI_TM)) + c];
        }
        sM[x] = v;
    }
    int* sCnt = (int*)(tile + EPI_ROWS * 24);                       // fill: the slot counter; count: 4 x (hits, defined)
    double* sBs = (double*)(tile + EPI_ROWS * 24 + 64);             // count: 4 x stat
    long long* sBij = (long long*)(tile + EPI_ROWS * 24 + 128);     // count: 4 x (i, j)
    if (MODE == 2 && tid == 0) sCnt[0] = 0;
    __syncthreads();

    int hits = 0, defd = 0;
    double bs = 0.0;
    long bi = -1, bj = -1;
#pragma unroll
    for (int b = 0; b < 2; b++) {
        const int jl = 32 * b + r;
        const long gj = brow0 + jl;
        const EpiMarker mj = {sM[3 * (EPI_TM + jl)], sM[3 * (EPI_TM + jl) + 1], sM[3 * (EPI_TM + jl) + 2]};
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int il = 32 * w + (e & 3) + 8 * (e >> 2) + 4 * h;
            const long gi = arow0 + il;
            if (gi >= rowsA) continue;
            if (MODE == 0) {
                if (jl >= o.nloci) continue;
            } else {
                if (gj >= rowsB || gi >= gj || !epi_pair_tested(gi, gj, o.chrom, o.gap)) continue;
            }
            const EpiMarker mi = {sM[3 * il], sM[3 * il + 1], sM[3 * il + 2]};
            const int64_t d = acc[b][0][e], ee = acc[b][1][e], f = acc[b][2][e], hh = acc[b][3][e];
            const int64_t z = (int64_t)acc[b][4][e] + 128 * (int64_t)acc[b][5][e] + 16384 * (int64_t)acc[b][6][e];
            const double st = epi_stat(trait, mi, mj, d, ee, f, hh, z, nullptr);
            if (MODE == 0) {
                const long at = gi * o.nloci + jl;
                o.stat[at] = st;
                if (o.mom) {
                    int64_t* m = o.mom + 5 * at;
                    m[0] = d; m[1] = ee; m[2] = f; m[3] = hh; m[4] = z;
                }
            } else if (st == st) {                                  // defined
                const bool hit = st >= o.min_stat;
                if (MODE == 1) {
                    defd++;
                    hits += hit;
                    if (epi_beats(bs, bi, bj, st, gi, gj)) { bs = st; bi = gi; bj = gj; }
                } else if (hit) {
                    const long at = o.base[blockIdx.x] + atomicAdd(&sCnt[0], 1);
                    o.hit_ij[2 * at] = (int32_t)gi;
                    o.hit_ij[2 * at + 1] = (int32_t)gj;
                    o.hit_stat[at] = st;
                    int64_t* m = o.hit_mom + 5 * at;
                    m[0] = d; m[1] = ee; m[2] = f; m[3] = hh; m[4] = z;
                }
            }
        }
    }
    if (MODE != 1) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        hits += __shfl_xor(hits, off);
        defd += __shfl_xor(defd, off);
        const double os = __shfl_xor(bs, off);
        const long oi = __shfl_xor(bi, off), oj = __shfl_xor(bj, off);
        if (epi_beats(bs, bi, bj, os, oi, oj)) { bs = os; bi = oi; bj = oj; }
    }
    if (lane == 0) {
        sCnt[2 * w] = hits;
        sCnt[2 * w + 1] = defd;
        sBs[w] = bs;
        sBij[2 * w] = bi;
        sBij[2 * w + 1] = bj;
    }
    __syncthreads();
    if (tid == 0) {
        for (int x = 1; x < 4; x++) {
            hits += sCnt[2 * x];
            defd += sCnt[2 * x + 1];
            if (epi_beats(bs, bi, bj, sBs[x], sBij[2 * x], sBij[2 * x + 1])) { bs = sBs[x]; bi = sBij[2 * x]; bj = sBij[2 * x + 1]; }
        }
        o.tcount[2 * blockIdx.x] = hits;
        o.tcount[2 * blockIdx.x + 1] = defd;
        o.tmax[blockIdx.x] = bs;
        o.tmaxij[2 * blockIdx.x] = (int32_t)bi;
        o.tmaxij[2 * blockIdx.x + 1] = (int32_t)bj;
    }
}

static bool epi_bad_image(const int8_t* p, long n, long ld) { return n <= 0 || n > ld || ld % 16 || ((uintptr_t)p & 15) || n > EPI_MAX_N; }

extern "C" int eagle_dev_epi_marker(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, const int32_t* y, int64_t* msu, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (epi_bad_image(Mt8, n, ld)) return eagle_fail(ctx, EAGLE_ERR_ARG, "epi_marker: bad image shape");
    const long blocks = (rows + 3) / 4;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "epi_marker: too many rows");
    hipLaunchKernelGGL(k_epi_marker, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, Mt8, rows, n, ld, y, msu);
    EPI_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

namespace {

int epi_fail(eagle_ctx* ctx, const char* who, const char* msg) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", who, msg);
    if (ctx) return eagle_fail(ctx, EAGLE_ERR_ARG, buf);
    snprintf(g_open_err, sizeof g_open_err, "%s", buf);
    return EAGLE_ERR_ARG;
}

// What both entry points put on the device for the trait: y, the six digit planes and (Y, T).
struct EpiTraitDev {
    DevBuf y, dig;
    long kpad = 0;
    EpiTrait t{0, 0, 0};
    int upload(eagle_ctx* ctx, const int32_t* yv, long n) {
        kpad = (n + EPI_BK - 1) / EPI_BK * EPI_BK;
        std::vector<int8_t> planes((size_t)6 * (size_t)kpad, 0);
        t.n = n;
        for (long k = 0; k < n; k++) {
            int8_t d[3];
            (void)epi_digits(yv[k], d);
            for (int p = 0; p < 3; p++) {
                planes[(size_t)p * kpad + k] = d[p];
                planes[(size_t)(3 + p) * kpad + k] = (int8_t)-d[p];
            }
            t.Y += yv[k];
            t.T += (int64_t)yv[k] * yv[k];
        }
        HIPCHK(ctx, y.alloc(sizeof(int32_t) * (size_t)n));
        HIPCHK(ctx, dig.alloc(planes.size()));
        HIPCHK(ctx, hipMemcpyAsync(y.p, yv, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(dig.p, planes.data(), planes.size(), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));       // `planes` leaves with this frame
        return EAGLE_OK;
    }
};

template <int MODE>
int epi_launch(eagle_ctx* ctx, const int8_t* A8, long rowsA, long ld, const int8_t* B8, long rowsB, long ldB, long n, const int32_t* tiles, long nt,
               EpiTraitDev& tr, const int64_t* msuA, const int64_t* msuB, const EpiOut& o) {
    if (nt <= 0) return EAGLE_OK;
    if (epi_bad_image(A8, n, ld) || epi_bad_image(B8, n, ldB)) return eagle_fail(ctx, EAGLE_ERR_ARG, "epi_tile: bad image shape");
    if (nt > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "epi_tile: too many tile pairs");
    hipLaunchKernelGGL((k_epi_tile<MODE>), dim3((unsigned)nt), dim3(256), 0, ctx->stream, A8, rowsA, ld, B8, rowsB, ldB, (n + 15) / 16 * 16, tiles,
                       tr.dig.as<int8_t>(), tr.kpad, tr.t, msuA, msuB, o);
    EPI_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

}  // namespace

// The loci's rows are gathered into a 64-row image as eagle_ld_dots gathers them; every 128-row tile of Mt then runs against it, where
// the image lies or window by window.
extern "C" int eagle_epistasis_loci(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const int32_t* y, const long* loci, long nloci,
                                    double max_memory_in_Gbytes, double* stat_out, int64_t* mom_out) {
    const char* who = "epistasis_loci";
    if (!f_name_ascii_Mt || !dims || !y || !loci || !stat_out) return epi_fail(ctx, who, "NULL argument");
    const long n = dims[0], L = dims[1];
    if (const char* bad = epi_arg_error(n, L, y)) return epi_fail(ctx, who, bad);
    if (const char* bad = epi_loci_arg_error(L, loci, nloci)) return epi_fail(ctx, who, bad);
    if (!ctx) return epi_fail(ctx, who, "no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long k = nloci;
    ImageLines lines;
    int rc = lines.open(ctx, f_name_ascii_Mt, L, n, max_memory_in_Gbytes);
    if (rc) return rc;
    const long ld = lines.ld();
    EpiTraitDev tr;
    if ((rc = tr.upload(ctx, y, n))) return rc;
    LociRows B;
    DevBuf msuB, stat, mom;
    HIPCHK(ctx, msuB.alloc(sizeof(int64_t) * 3 * 64));
    HIPCHK(ctx, stat.alloc(sizeof(double) * (size_t)L * (size_t)k));
    if (mom_out) HIPCHK(ctx, mom.alloc(sizeof(int64_t) * 5 * (size_t)L * (size_t)k));
    rc = B.gather(lines, loci, k);
    if (rc) return rc;
    rc = eagle_dev_epi_marker(ctx, B.rows(), 64, n, ld, tr.y.as<int32_t>(), msuB.as<int64_t>(), ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }

    const RowWindows ws = lines.disjoint(std::min(L, std::max(512L, lines.stream_rows())));
    const long ntmax = (ws.cap + EPI_TM - 1) / EPI_TM;
    std::vector<int32_t> tl((size_t)2 * ntmax, 0);
    for (long a = 0; a < ntmax; a++) tl[(size_t)2 * a] = (int32_t)a;
    DevBuf tiles, msuA;
    HIPCHK(ctx, tiles.alloc(sizeof(int32_t) * tl.size()));
    HIPCHK(ctx, msuA.alloc(sizeof(int64_t) * 3 * (size_t)ws.cap));
    HIPCHK(ctx, hipMemcpyAsync(tiles.p, tl.data(), sizeof(int32_t) * tl.size(), hipMemcpyHostToDevice, ctx->stream));
    rc = lines.each(ws, [&](const int8_t* img, long r0, long nr, long, long) {
        EpiOut o{};
        o.nloci = (int)k;
        o.stat = stat.as<double>() + r0 * k;
        o.mom = mom_out ? mom.as<int64_t>() + 5 * r0 * k : nullptr;
        const int mrc = eagle_dev_epi_marker(ctx, img, nr, n, ld, tr.y.as<int32_t>(), msuA.as<int64_t>(), ctx->stream);
        return mrc ? mrc : epi_launch<0>(ctx, img, nr, ld, B.rows(), 64, ld, n, tiles.as<int32_t>(), (nr + EPI_TM - 1) / EPI_TM, tr,
                                         msuA.as<int64_t>(), msuB.as<int64_t>(), o);
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(stat_out, stat.p, sizeof(double) * (size_t)L * (size_t)k, hipMemcpyDeviceToHost, ctx->stream));
    if (mom_out) HIPCHK(ctx, hipMemcpyAsync(mom_out, mom.p, sizeof(int64_t) * 5 * (size_t)L * (size_t)k, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));       // `map` and `tl` leave with this frame
    return EAGLE_OK;
}

// Two passes over the upper triangle of tile pairs (A tile a of 128 rows, B tile b of 64 rows, b >= 2 a: the others hold no i < j).
extern "C" int eagle_epistasis_pairs(eagle_ctx* ctx, const char* f_name_ascii_Mt, const long dims[2], const int32_t* y, const int32_t* chrom, long gap,
                                     double min_stat, double max_memory_in_Gbytes, int32_t* hit_ij, double* hit_stat, int64_t* hit_mom, long hit_cap,
                                     long* nhits_out, long* ntested_out, eagle_epi_max* max_out) {
    const char* who = "epistasis_pairs";
    if (!f_name_ascii_Mt || !dims || !y || !nhits_out || !ntested_out || !max_out) return epi_fail(ctx, who, "NULL argument");
    const long n = dims[0], L = dims[1];
    if (const char* bad = epi_arg_error(n, L, y)) return epi_fail(ctx, who, bad);
    if (const char* bad = epi_pairs_arg_error(gap, min_stat, hit_cap, hit_ij && hit_stat && hit_mom)) return epi_fail(ctx, who, bad);
    const long nta = (L + EPI_TM - 1) / EPI_TM, ntb = (L + EPI_TB - 1) / EPI_TB;
    long nt = 0;
    for (long a = 0; a < nta; a++) nt += ntb - 2 * a;
    if (nt > 0x3fffffffL) return epi_fail(ctx, who, "too many markers for an all-pairs pass (2^30 tile pairs or more): prune or filter first");
    if (!ctx) return epi_fail(ctx, who, "no context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const GenoEntry* src = nullptr;
    int rc = eagle_get_resident(ctx, f_name_ascii_Mt, L, n, max_memory_in_Gbytes, host_threads(), &src);
    if (rc == EAGLE_STREAM || (rc == EAGLE_OK && !src))
        return epi_fail(ctx, who, "the image is not resident and does not fit max_memory_in_Gbytes: prune or filter the markers first "
                                   "(a streamed all-pairs pass does not exist)");
    if (rc != EAGLE_OK) return rc;
    const long ld = src->ld;
    EpiTraitDev tr;
    if ((rc = tr.upload(ctx, y, n))) return rc;
    std::vector<int32_t> tl((size_t)2 * nt);
    {
        size_t x = 0;
        for (long a = 0; a < nta; a++)
            for (long b = 2 * a; b < ntb; b++) { tl[x++] = (int32_t)a; tl[x++] = (int32_t)b; }
    }
    DevBuf tiles, msu, d_chrom, tcount, tmax, tmaxij;
    HIPCHK(ctx, tiles.alloc(sizeof(int32_t) * tl.size()));
    HIPCHK(ctx, msu.alloc(sizeof(int64_t) * 3 * (size_t)L));
    HIPCHK(ctx, tcount.alloc(sizeof(int32_t) * 2 * (size_t)nt));
    HIPCHK(ctx, tmax.alloc(sizeof(double) * (size_t)nt));
    HIPCHK(ctx, tmaxij.alloc(sizeof(int32_t) * 2 * (size_t)nt));
    HIPCHK(ctx, hipMemcpyAsync(tiles.p, tl.data(), sizeof(int32_t) * tl.size(), hipMemcpyHostToDevice, ctx->stream));
    if (chrom) {
        HIPCHK(ctx, d_chrom.alloc(sizeof(int32_t) * (size_t)L));
        HIPCHK(ctx, hipMemcpyAsync(d_chrom.p, chrom, sizeof(int32_t) * (size_t)L, hipMemcpyHostToDevice, ctx->stream));
    }
    EpiOut o{};
    o.chrom = chrom ? d_chrom.as<int32_t>() : nullptr;
    o.gap = gap;
    o.min_stat = min_stat;
    o.tcount = tcount.as<int32_t>();
    o.tmax = tmax.as<double>();
    o.tmaxij = tmaxij.as<int32_t>();
    rc = eagle_dev_epi_marker(ctx, src->dev, L, n, ld, tr.y.as<int32_t>(), msu.as<int64_t>(), ctx->stream);
    if (!rc) rc = epi_launch<1>(ctx, src->dev, L, ld, src->dev, L, ld, n, tiles.as<int32_t>(), nt, tr, msu.as<int64_t>(), msu.as<int64_t>(), o);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    std::vector<int32_t> h_count((size_t)2 * nt), h_ij((size_t)2 * nt);
    std::vector<double> h_max((size_t)nt);
    HIPCHK(ctx, hipMemcpyAsync(h_count.data(), tcount.p, sizeof(int32_t) * h_count.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(h_max.data(), tmax.p, sizeof(double) * h_max.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(h_ij.data(), tmaxij.p, sizeof(int32_t) * h_ij.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    long total = 0, tested = 0;
    eagle_epi_max best = {-1, -1, 0.0};
    std::vector<int32_t> tl2;
    std::vector<int64_t> base;
    for (long x = 0; x < nt; x++) {
        const long i = h_ij[(size_t)2 * x], j = h_ij[(size_t)2 * x + 1];
        if (i >= 0 && (best.i < 0 || h_max[(size_t)x] > best.stat ||
                       (h_max[(size_t)x] == best.stat && (i < best.i || (i == best.i && j < best.j))))) {
            best.i = i; best.j = j; best.stat = h_max[(size_t)x];
        }
        tested += h_count[(size_t)2 * x + 1];
        if (h_count[(size_t)2 * x] > 0) {
            tl2.push_back(tl[(size_t)2 * x]);
            tl2.push_back(tl[(size_t)2 * x + 1]);
            base.push_back(total);
            total += h_count[(size_t)2 * x];
        }
    }
    if (best.i < 0) {
        const uint64_t nanbits = 0x7ff8000000000000ull;
        memcpy(&best.stat, &nanbits, sizeof best.stat);
    }
    *nhits_out = total;
    *ntested_out = tested;
    *max_out = best;
    if (total == 0 || total > hit_cap) return EAGLE_OK;

    DevBuf tiles2, d_base, d_ij, d_stat, d_mom;
    HIPCHK(ctx, tiles2.alloc(sizeof(int32_t) * tl2.size()));
    HIPCHK(ctx, d_base.alloc(sizeof(int64_t) * base.size()));
    HIPCHK(ctx, d_ij.alloc(sizeof(int32_t) * 2 * (size_t)total));
    HIPCHK(ctx, d_stat.alloc(sizeof(double) * (size_t)total));
    HIPCHK(ctx, d_mom.alloc(sizeof(int64_t) * 5 * (size_t)total));
    HIPCHK(ctx, hipMemcpyAsync(tiles2.p, tl2.data(), sizeof(int32_t) * tl2.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_base.p, base.data(), sizeof(int64_t) * base.size(), hipMemcpyHostToDevice, ctx->stream));
    o.base = d_base.as<int64_t>();
    o.hit_ij = d_ij.as<int32_t>();
    o.hit_stat = d_stat.as<double>();
    o.hit_mom = d_mom.as<int64_t>();
    rc = epi_launch<2>(ctx, src->dev, L, ld, src->dev, L, ld, n, tiles2.as<int32_t>(), (long)base.size(), tr, msu.as<int64_t>(), msu.as<int64_t>(), o);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    std::vector<int32_t> r_ij((size_t)2 * total);
    std::vector<double> r_stat((size_t)total);
    std::vector<int64_t> r_mom((size_t)5 * total);
    HIPCHK(ctx, hipMemcpyAsync(r_ij.data(), d_ij.p, sizeof(int32_t) * r_ij.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(r_stat.data(), d_stat.p, sizeof(double) * r_stat.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(r_mom.data(), d_mom.p, sizeof(int64_t) * r_mom.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<long> order((size_t)total);
    std::iota(order.begin(), order.end(), 0L);
    std::sort(order.begin(), order.end(), [&](long a, long b) {
        return r_ij[(size_t)2 * a] != r_ij[(size_t)2 * b] ? r_ij[(size_t)2 * a] < r_ij[(size_t)2 * b] : r_ij[(size_t)2 * a + 1] < r_ij[(size_t)2 * b + 1];
    });
    for (long x = 0; x < total; x++) {
        const size_t s = (size_t)order[(size_t)x];
        hit_ij[2 * x] = r_ij[2 * s];
        hit_ij[2 * x + 1] = r_ij[2 * s + 1];
        hit_stat[x] = r_stat[s];
        memcpy(hit_mom + 5 * x, r_mom.data() + 5 * s, sizeof(int64_t) * 5);
    }
    return EAGLE_OK;
}
