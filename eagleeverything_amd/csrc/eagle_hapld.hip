// eagle_hapld.hip -- pairwise haplotype frequencies by EM, Lewontin's D' and the haplotype r^2 between markers at most `window` <= 256
// apart (include/eagle_hip.h section 1b''''vii): eagle_ld.hip's band tile with four integer products per block pair and an fp64 epilogue
// whose order of operations is fixed.  Every number is an exact integer until that epilogue, and every fp64 operation in it is one
// correctly rounded multiplication, addition, subtraction or division (hl_mul .. hl_div below, compiled with contraction off), so nothing
// becomes an FMA and the numpy restatement (r_api.hap_ld_host) gives the same bits.
//
//   Per pair i < j four int32 sums over the individuals:  d = sum g_i g_j,  e = sum g_i^2 g_j^2,  f = sum g_i^2 g_j,  h = sum g_i g_j^2.
//   With s and q of both markers (k_marker_counts, k_ld_sq) they give the nine cells of the genotype table, the four known haplotype
//   counts and x, the number of double heterozygotes, whose phase the EM resolves (the rule is the header's).
//
// k_hapld_tile<NB>.  k_ld_tile's geometry: a workgroup (256 threads, 4 waves) owns TM = 128 consecutive markers, K chunks of 128
// individuals, LDS rows of 128 B with logical 16-byte chunk c of row r at physical chunk c ^ ((r >> 1) & 7), v_mfma_i32_32x32x32_i8.
// Wave w multiplies the 32-row block w of the tile (A) against the blocks w + o, 0 <= o < NB = floor((window + 31) / 32) + 1 (B).  Only the
// genotype image is staged: the g^2 operand of either side is made in registers as x & 0x01010101 per dword (g^2 of -1 / 0 / +1 = 0xff,
// 0x00, 0x01), the way k_group_tile makes it, and each block pair takes four products: g.g (d), g^2.g^2 (e), g^2.g (f), g.g^2 (h).
//   Registers set the shape.  Four products x 16 int32 x NB = 576 accumulator registers per lane at NB = 9; one wave per SIMD has 512.
//   The block offsets are therefore walked in GROUPS of at most HL_G = 3 (192 accumulator registers; the 10 x 4 staging registers of the
//   next chunk, the operands and the epilogue's fp64 state come on top), and the K loop runs once per group INSIDE the workgroup: the
//   mask words of neighbouring block offsets overlap, so a group per workgroup would need global atomics.  The later passes read A and B
//   from L2.  The compiler's report for gfx950 (-Rpass-analysis=kernel-resource-usage) at HL_G = 3: 230 VGPRs + 128 AGPRs at NB = 2,
//   256 + 194 at NB = 3, 256 + 212 .. 215 at NB = 4 .. 9 (471 of the 512 at NB = 9), ScratchSize 0 and no VGPR spill in all eight
//   instantiations.  Groups of 4 would leave NB = 9 at three passes (4 + 4 + 1) and have 64 accumulators more to place; not compiled.
//   The element loop of the epilogue is NOT unrolled: sixteen copies of the EM per offset are more than the unroller takes, and the
//   accumulators of a partly unrolled loop are indexed in memory (832 bytes of scratch in the first version of this file).
//   LDS per workgroup, static: the 128 A rows and the 32 (G + 3) B rows the four waves need for G offsets, (128 + 32 (HL_G + 3)) x 128 B =
//   40 KiB, s and q of the 128 + 32 (NB - 1) <= 384 staged markers (3 KiB) and two planes of 128 x 8 mask half words (8 KiB) that live
//   across the groups: 52,224 B.  The registers, not LDS, keep it at one workgroup (one wave a SIMD) per compute unit.
//   Loads are k_ld_tile's: plain 16-byte global loads into registers for chunk c + 1 before the MFMAs of chunk c, written to LDS after
//   them.  Rows at or beyond `rows` and bytes at or beyond ceil16(n) are staged as zeros and never read.
//   Epilogue, per group: every lane runs the rule for its accumulator elements inside the band, one after the other; the lanes of a wave
//   iterate until the slowest pair of the wave stops (a wave's loop ends when no lane is live).  The two verdict bits are ORed into the
//   tile's mask words in LDS and leave once, after the last group, by plain 8-byte vector stores; the two fp64 band entries of the pair
//   are written by the lane that owns it.  Every output word has one owning workgroup: no global atomics but the four integer totals
//   (one 64-bit vector atomic add per wave and total; integer adds in any order give one result).
//   A launch works on the `crows` markers it OWNS (the tile rows below crows: only their words are written and counted) out of the
//   `rows` >= crows markers it holds: the markers behind the owned ones are the partners of the last of them (the host's row windows).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

typedef int hl_i32x4 __attribute__((ext_vector_type(4)));
typedef int hl_i32x16 __attribute__((ext_vector_type(16)));

#define HL_TM 128   /* markers per workgroup */
#define HL_BK 128   /* individuals (bytes of a row) per staged chunk */
#define HL_G 3      /* block offsets per pass over K */
#define HL_TROWS (HL_TM + 32 * (HL_G + 3))   /* staged rows of a pass */
#define HL_SQ_ROWS (HL_TM + 32 * 8)          /* markers whose s and q a tile may need: NB - 1 <= 8 */

// The rule's fp64 operations, one rounding each.  hipcc contracts a * b + c into an FMA by default, and the __dmul_rn / __dadd_rn of the
// HIP headers are plain operators that contract like any other once they are inlined (a product feeding a sum is enough: k + x t here),
// so contraction is switched off for the rest of this file and the four operations are spelled out.
#pragma clang fp contract(off)
__device__ __forceinline__ double hl_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double hl_add(double a, double b) { return a + b; }
__device__ __forceinline__ double hl_sub(double a, double b) { return a - b; }
__device__ __forceinline__ double hl_div(double a, double b) { return a / b; }

struct HapLdRule {
    long n;
    double tol, fg_cut, dprime_cut;
    int max_iter, window;
};

// The rule of include/eagle_hip.h section 1b''''vii for one pair of polymorphic markers.  Returns the stop code.
__device__ __forceinline__ int hapld_pair(const HapLdRule& R, int si, int qi, int sj, int qj, int d, int e, int f, int h, double& dprime,
                                          double& r2h, double& pmin) {
    const long long n = R.n, E = e, F = f, H = h, D = d;
    const long long n22 = (E + F + H + D) / 4, n00 = (E - F - H + D) / 4, n20 = (E - F + H - D) / 4, n02 = (E + F - H - D) / 4;
    const long long n12 = (qj + sj - E - F) / 2, n10 = (qj - sj - E + F) / 2, n21 = (qi + si - E - H) / 2, n01 = (qi - si - E + H) / 2;
    const long long x = n - qi - qj + E;
    const double kBB = (double)(2 * n22 + n21 + n12), kBA = (double)(2 * n20 + n21 + n10), kAB = (double)(2 * n02 + n01 + n12),
                 kAA = (double)(2 * n00 + n01 + n10);
    const long long bi = n + si, bj = n + sj;
    const double T = (double)(2 * n);
    const double pi = hl_div((double)bi, T), qi_ = hl_div((double)(2 * n - bi), T);
    const double pj = hl_div((double)bj, T), qj_ = hl_div((double)(2 * n - bj), T);
    const double pipj = hl_mul(pi, pj), piqj = hl_mul(pi, qj_), qipj = hl_mul(qi_, pj), qiqj = hl_mul(qi_, qj_);
    double pBB, pBA, pAB, pAA;
    int code = 0;
    if (x == 0) {
        pBB = hl_div(kBB, T);
        pBA = hl_div(kBA, T);
        pAB = hl_div(kAB, T);
        pAA = hl_div(kAA, T);
    } else {
        pBB = pipj; pBA = piqj; pAB = qipj; pAA = qiqj;
        const double xd = (double)x;
        for (int it = 1;; it++) {
            const double u = hl_mul(pBB, pAA), v = hl_mul(pBA, pAB), den = hl_add(u, v);
            const double t = den > 0.0 ? hl_div(u, den) : 0.5;
            const double xt = hl_mul(xd, t), xo = hl_sub(xd, xt);
            const double nBB = hl_div(hl_add(kBB, xt), T);
            const double delta = fabs(hl_sub(nBB, pBB));
            pBB = nBB;
            pAA = hl_div(hl_add(kAA, xt), T);
            pBA = hl_div(hl_add(kBA, xo), T);
            pAB = hl_div(hl_add(kAB, xo), T);
            if (delta <= R.tol) break;
            if (it == R.max_iter) { code = 1; break; }
        }
    }
    const double Dh = hl_sub(pBB, pipj);
    const double dmax = Dh >= 0.0 ? (piqj < qipj ? piqj : qipj) : (pipj < qiqj ? pipj : qiqj);
    double dp = hl_div(Dh, dmax);
    dp = dp > 1.0 ? 1.0 : (dp < -1.0 ? -1.0 : dp);
    dprime = dp;
    r2h = hl_div(hl_mul(Dh, Dh), hl_mul(hl_mul(pi, qi_), hl_mul(pj, qj_)));
    const double m1 = pBB < pBA ? pBB : pBA, m2 = pAB < pAA ? pAB : pAA;
    pmin = m1 < m2 ? m1 : m2;
    return code;
}

// One pass over K for the G block offsets g0 .. g0 + G - 1 of the tile at row0, and their epilogue.  tile: HL_TROWS rows x 128 B; rows
// [0, 128) are the A rows, row 128 + x is tile row 32 g0 + x.  sSQ: (s, q) of the tile's markers; sR / sT: 128 x 8 mask half words.
template <int G>
__device__ __forceinline__ void hapld_group(int8_t* tile, const int* sSQ, unsigned* sR, unsigned* sT, const int8_t* __restrict__ Mt8, long rows,
                                            long crows, long ld, long kbytes, long row0, int g0, const HapLdRule& R,
                                            double* __restrict__ dprime, double* __restrict__ r2, unsigned (&cnt)[4]) {
    constexpr int RU = HL_TM + 32 * (G + 3);     // rows this group stages
    constexpr int NCH = RU / 32;                 // 16-byte pieces per thread and chunk: RU * 8 / 256
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, hh = lane >> 5;

    hl_i32x4 pre[NCH];
    auto fetch = [&](long k0) {
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int idx = tid + 256 * i, rr = idx >> 3;
            const long kb = k0 + 16 * (idx & 7);
            const long g = row0 + (rr < HL_TM ? rr : 32 * g0 + rr - HL_TM);
            hl_i32x4 v = {0, 0, 0, 0};
            if (kb < kbytes && g < rows) v = *(const hl_i32x4*)(Mt8 + g * ld + kb);
            pre[i] = v;
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int idx = tid + 256 * i, rr = idx >> 3, c = idx & 7;
            *(hl_i32x4*)(tile + rr * HL_BK + ((c ^ ((rr >> 1) & 7)) << 4)) = pre[i];
        }
    };

    // products: 0 g.g = d, 1 g^2.g^2 = e, 2 g^2.g = f, 3 g.g^2 = h  (first factor: the A marker i)
    hl_i32x16 acc[G][4];
#pragma unroll
    for (int b = 0; b < G; b++)
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[b][p][e] = 0;

    const int8_t* pa = tile + (32 * w + r) * HL_BK;
    const int8_t* pb = tile + (HL_TM + 32 * w + r) * HL_BK;
    const int swz = (r >> 1) & 7;

    fetch(0);
    for (long k0 = 0; k0 < kbytes; k0 += HL_BK) {
        put();
        __syncthreads();
        if (k0 + HL_BK < kbytes) fetch(k0 + HL_BK);
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
            const int ch = ((2 * ks + hh) ^ swz) << 4;
            const hl_i32x4 a = *(const hl_i32x4*)(pa + ch);
            const hl_i32x4 a2 = a & 0x01010101;                     // g^2 of -1 / 0 / +1
#pragma unroll
            for (int b = 0; b < G; b++) {
                const hl_i32x4 bb = *(const hl_i32x4*)(pb + b * (32 * HL_BK) + ch);
                const hl_i32x4 b2 = bb & 0x01010101;
                acc[b][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bb, acc[b][0], 0, 0, 0);
                acc[b][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a2, b2, acc[b][1], 0, 0, 0);
                acc[b][2] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a2, bb, acc[b][2], 0, 0, 0);
                acc[b][3] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b2, acc[b][3], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // accumulator element e of offset b: marker i = 32 w + (e & 3) + 8 (e >> 2) + 4 h of the tile (the A row), j = 32 (g0 + w + b) + r
#pragma unroll
    for (int b = 0; b < G; b++) {
        const int jl = 32 * (g0 + w + b) + r;
        const int sj = sSQ[2 * jl], qj = sSQ[2 * jl + 1];
        const long long bj = R.n + sj;
        const bool jok = row0 + jl < rows && R.n >= 2 && bj > 0 && bj < 2 * R.n;
        // e is not unrolled: sixteen copies of the EM per offset are more code than the unroller takes, and a partly unrolled loop
        // would index the accumulators in memory.  The element is picked by a chain of selects on the wave-uniform e instead.
#pragma unroll 1
        for (int e = 0; e < 16; e++) {
            int pd = 0, pe = 0, pf = 0, ph = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                pd = k == e ? acc[b][0][k] : pd;
                pe = k == e ? acc[b][1][k] : pe;
                pf = k == e ? acc[b][2][k] : pf;
                ph = k == e ? acc[b][3][k] : ph;
            }
            const int il = 32 * w + (e & 3) + 8 * (e >> 2) + 4 * hh, o = jl - il;
            const long gi = row0 + il;
            if (o < 1 || o > R.window || gi >= crows) continue;
            const int si = sSQ[2 * il], qi = sSQ[2 * il + 1];
            const long long bi = R.n + si;
            double dp = -2.0, rh = -1.0;
            if (jok && bi > 0 && bi < 2 * R.n) {
                double pmin;
                const int code = hapld_pair(R, si, qi, sj, qj, pd, pe, pf, ph, dp, rh, pmin);
                const bool rec = pmin > R.fg_cut, str = fabs(dp) >= R.dprime_cut;
                const int at = il * 8 + ((o - 1) >> 5);
                const unsigned bit = 1u << ((o - 1) & 31);
                if (rec) atomicOr(&sR[at], bit);
                if (str) atomicOr(&sT[at], bit);
                cnt[0]++;
                cnt[1] += (unsigned)code;
                cnt[2] += rec;
                cnt[3] += str;
            }
            if (dprime) dprime[gi * R.window + (o - 1)] = dp;
            if (r2) r2[gi * R.window + (o - 1)] = rh;
        }
    }
}

// kbytes = ceil16(n).  recomb / strong: crows x wpr uint64; dprime / r2: crows x window fp64; each may be null.  counts: 4 totals, ADDED to.
template <int NB>
__global__ __launch_bounds__(256) void k_hapld_tile(const int8_t* __restrict__ Mt8, long rows, long crows, long ld, long kbytes,
                                                    const int32_t* __restrict__ sq, HapLdRule R, uint64_t* __restrict__ recomb,
                                                    uint64_t* __restrict__ strong, int wpr, double* __restrict__ dprime,
                                                    double* __restrict__ r2, unsigned long long* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) int8_t tile[HL_TROWS * HL_BK];
    __shared__ int sSQ[2 * HL_SQ_ROWS];
    __shared__ unsigned sR[HL_TM * 8], sT[HL_TM * 8];
    const int tid = threadIdx.x;
    const long row0 = (long)blockIdx.x * HL_TM;
    for (int x = tid; x < HL_TM * 8; x += 256) sR[x] = sT[x] = 0u;
    for (int x = tid; x < HL_SQ_ROWS; x += 256) {
        const long g = row0 + x;
        sSQ[2 * x] = g < rows ? sq[2 * g] : 0;
        sSQ[2 * x + 1] = g < rows ? sq[2 * g + 1] : 0;
    }
    __syncthreads();
    unsigned cnt[4] = {0u, 0u, 0u, 0u};
    // the NB block offsets in groups of HL_G = 3, the last one shorter
#define HL_GROUP(G0)                                                                                                               \
    if constexpr (NB > G0)                                                                                                         \
        hapld_group<(NB - G0 < HL_G ? NB - G0 : HL_G)>(tile, sSQ, sR, sT, Mt8, rows, crows, ld, kbytes, row0, G0, R, dprime, r2, cnt);
    HL_GROUP(0) HL_GROUP(3) HL_GROUP(6)
#undef HL_GROUP
#pragma unroll
    for (int c = 0; c < 4; c++) {
        unsigned v = cnt[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((tid & 63) == 0 && v) atomicAdd(&counts[c], (unsigned long long)v);
    }
    __syncthreads();
    for (int x = tid; x < HL_TM * wpr; x += 256) {
        const int il = x / wpr, wd = x - il * wpr;
        const long gi = row0 + il;
        if (gi >= crows) continue;
        if (recomb) recomb[gi * wpr + wd] = (uint64_t)sR[il * 8 + 2 * wd] | ((uint64_t)sR[il * 8 + 2 * wd + 1] << 32);
        if (strong) strong[gi * wpr + wd] = (uint64_t)sT[il * 8 + 2 * wd] | ((uint64_t)sT[il * 8 + 2 * wd + 1] << 32);
    }
}

// Mt8 / sq: the first OWNED marker of the launch and the rows - 1 behind it; the outputs: that marker's row.
extern "C" int eagle_dev_hap_ld(eagle_ctx* ctx, const int8_t* Mt8, long rows, long crows, long n, long ld, const int32_t* sq, long window,
                                double tol, int max_iter, double fg_cut, double dprime_cut, uint64_t* recomb, uint64_t* strong,
                                long words_per_row, double* dprime, double* r2, uint64_t* counts, void* stream) {
    if (crows <= 0) return EAGLE_OK;
    if (!Mt8 || !sq || !counts || crows > rows || n <= 0 || n > ld || ld % 16 || ((uintptr_t)Mt8 & 15) || n > 0x3fffffffL)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "hap_ld: bad image shape");
    if (window < 1 || window > 256 || words_per_row != (window + 63) / 64 || !(tol > 0.0 && tol < 1.0) || max_iter < 1 ||
        !(fg_cut >= 0.0 && fg_cut <= 1.0) || !(dprime_cut >= 0.0 && dprime_cut <= 1.0))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "hap_ld: bad window, tolerance, cut or mask width");
    const long blocks = (crows + HL_TM - 1) / HL_TM;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "hap_ld: too many rows");
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t s = (hipStream_t)stream;
    const long kbytes = (n + 15) / 16 * 16;
    const int nb = (int)((window + 31) / 32) + 1;
    const HapLdRule R = {n, tol, fg_cut, dprime_cut, max_iter, (int)window};
#define HL_CASE(NB)                                                                                                                     \
    case NB:                                                                                                                            \
        hipLaunchKernelGGL((k_hapld_tile<NB>), grid, blk, 0, s, Mt8, rows, crows, ld, kbytes, sq, R, recomb, strong, (int)words_per_row, \
                           dprime, r2, (unsigned long long*)counts);                                                                    \
        break;
    switch (nb) {
        HL_CASE(2) HL_CASE(3) HL_CASE(4) HL_CASE(5) HL_CASE(6) HL_CASE(7) HL_CASE(8) HL_CASE(9)
    }
#undef HL_CASE
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return eagle_fail_hip(ctx, e, __func__);
    return EAGLE_OK;
}
