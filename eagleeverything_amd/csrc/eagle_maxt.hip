// eagle_maxt.hip -- max(T) permutation testing of every marker against one trait (include/eagle_hip.h section 1b''''vi): for R
// arrangements t' of an integer trait the exact d_m(t') = N sum g t' - S_m T of every marker, how often |d_m(t')| reaches the observed
// |d_m(t)| (count1), and per arrangement the largest key = fl(fl(d d) / V_m) with the lowest marker that attains it.  All sums are
// integers; the key is two correctly rounded fp64 operations on exact operands, so r_api.maxt_host gives the same words.
//
//   k_maxt_keys .......... key64(r, j) of the seeded rule for a block of permutations, padded to a power of two with all-ones keys.
//   k_maxt_sort_local /
//   k_maxt_sort_global ... a bitonic sort of every row of that block, ascending: the steps with a partner distance below MX_SORT_C run on
//                          MX_SORT_C keys in LDS, the longer ones one launch each in global memory.  The keys are distinct, so the result
//                          does not depend on the method; the low 16 bits of the sorted row are the index table pi_r.
//   k_maxt_operand ....... gathers the trait through pi (the sorted keys, an uploaded table, or the identity for the observed pass) into
//                          the int8 operand [P][R][ld]: plane p holds digit p of the sign-magnitude base-128 digits (maxt_digits of
//                          eagle_host.h), unused individuals and the bytes from n on are zero, every byte is written.
//   k_maxt_sv ............ (n0, n1, n2) of eagle_dev_group_counts with `used` as the one group -> S_m = n2 - n0, V_m = N (n2 + n0) - S_m^2.
//   k_maxt_tile<P, RB> ... the int8 image x the operand on v_mfma_i32_32x32x32_i8 with k_group_tile's staging: a workgroup (256 threads, 4
//                          waves) owns 128 markers x RW = 32 RB permutations over all n; per chunk of 128 individuals it stages the 128
//                          marker rows and the P RW operand rows, 128 B each, in LDS -- logical 16-byte chunk c of row r at physical chunk
//                          c ^ ((r >> 1) & 7), the loads of chunk c + 1 issued before the MFMAs of chunk c, rows and bytes out of range
//                          staged as zeros.  Wave w multiplies marker block w against the P RB operand blocks: 16 P RB accumulators a
//                          lane.  Epilogue: c = c0 + 128 c1 + 16384 c2 in int64, d, then the ballot of |d| >= |d_obs| over the 32
//                          permutations of a half wave adds to count1 with one integer atomic per marker, and the tile's best (key,
//                          marker) per permutation goes through a shuffle and LDS to one partial per tile and permutation.  No L x R
//                          array exists.  With OBS the operand is the trait itself and the epilogue stores d_obs and key_obs instead.
//   k_maxt_finish ........ per permutation the largest partial over all tiles in marker order, ties to the lower marker.
//
// The grid is laid out with the permutation blocks fastest, so the workgroups that run together read the same 128 marker rows and the
// image comes from HBM once per call; the operand (P R ld bytes) is re-read by every marker tile from the caches.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

typedef int mx_i32x4 __attribute__((ext_vector_type(4)));
typedef int mx_i32x16 __attribute__((ext_vector_type(16)));

#define MX_TM 128        /* markers per workgroup */
#define MX_BK 128        /* individuals (bytes of a row) per staged chunk */
#define MX_SORT_C 2048   /* keys of a bitonic chunk in LDS */

#define MX_LAUNCH_CHECK(ctx)                                                \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

// ------------------------------------------------------------------------------------------------------------------------------
// permutation stage
// ------------------------------------------------------------------------------------------------------------------------------
// keys[rr][j], rr < nr, j < NP2: key64(r_first + rr, j) for j < N, all ones behind (they sort to the end).  strata_u: the stratum of u_j or NULL
__global__ __launch_bounds__(256) void k_maxt_keys(uint64_t seed, long r_first, long nr, long N, long NP2, const uint16_t* __restrict__ strata_u,
                                                   uint64_t* __restrict__ keys) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nr * NP2) return;
    const long rr = t / NP2, j = t - rr * NP2;
    keys[t] = j < N ? maxt_key64(seed, (uint64_t)(r_first + rr), (uint64_t)j, strata_u ? strata_u[j] : 0u) : ~0ull;
}

// One workgroup = one chunk of C = min(MX_SORT_C, NP2) consecutive keys of one row.  Runs the bitonic steps (k, j) for k = k_first, 2
// k_first, ..., k_last and j = min(k / 2, C / 2), ..., 1: all of them pair keys inside the chunk.  The direction of a pair comes from the
// index within the ROW, so a chunk is one piece of the row's network.
__global__ __launch_bounds__(256) void k_maxt_sort_local(uint64_t* __restrict__ keys, long NP2, int C, long k_first, long k_last) {
    __shared__ uint64_t s[MX_SORT_C];
    const long base = (long)blockIdx.x * C;              // chunks of a row are consecutive, rows are consecutive: base = row NP2 + chunk C
    const long in_row = base & (NP2 - 1);
    for (int i = threadIdx.x; i < C; i += 256) s[i] = keys[base + i];
    __syncthreads();
    for (long k = k_first; k <= k_last; k <<= 1) {
        int j = (int)(k >> 1 < (long)(C >> 1) ? k >> 1 : (long)(C >> 1));
        for (; j > 0; j >>= 1) {
            for (int p = threadIdx.x; p < (C >> 1); p += 256) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const bool asc = ((in_row + i) & k) == 0;
                const uint64_t a = s[i], b = s[l];
                if ((a > b) == asc) { s[i] = b; s[l] = a; }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < C; i += 256) keys[base + i] = s[i];
}

// one step (k, j) with j >= MX_SORT_C over nr rows: one thread per pair
__global__ __launch_bounds__(256) void k_maxt_sort_global(uint64_t* __restrict__ keys, long nr, long NP2, long k, long j) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x, half = NP2 >> 1;
    if (t >= nr * half) return;
    const long rr = t / half, p = t - rr * half;
    const long i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
    uint64_t* row = keys + rr * NP2;
    const bool asc = (i & k) == 0;
    const uint64_t a = row[i], b = row[l];
    if ((a > b) == asc) { row[i] = b; row[l] = a; }
}

// ------------------------------------------------------------------------------------------------------------------------------
// operand stage: one thread = 16 individuals of one arrangement, all P planes.  rank[i] = the position k of individual i (in the order
// the arrangement fills: sigma's for the seeded rule, u's otherwise) or -1 = not used; the value at position k is tu[src], src = the low
// 16 bits of keys[rr][k], or perm[rr][k], or k itself when both are NULL.  op: [P][Rtot][ld], rows r0 .. r0 + nr written.
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_maxt_operand(const uint64_t* __restrict__ keys, long NP2, const int32_t* __restrict__ perm, long N,
                                                      const int32_t* __restrict__ rank, const int32_t* __restrict__ tu, long n, long ld, long lanes16,
                                                      int P, long Rtot, long r0, long nr, int8_t* __restrict__ op) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nr * lanes16) return;
    const long rr = t / lanes16, i0 = (t - rr * lanes16) * 16;
    mx_i32x4 v[3] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const long i = i0 + j;
        const int k = i < n ? rank[i] : -1;
        if (k < 0) continue;
        const long src = keys ? (long)(keys[rr * NP2 + k] & 0xffffu) : (perm ? (long)perm[rr * N + k] : (long)k);
        int8_t d[3];
        maxt_digits(tu[src], d);
#pragma unroll
        for (int p = 0; p < 3; p++) v[p][j >> 2] |= (int)(uint8_t)d[p] << (8 * (j & 3));
    }
    for (int p = 0; p < P; p++) *(mx_i32x4*)(op + ((long)p * Rtot + r0 + rr) * ld + i0) = v[p];
}

// counts[rows][1][3] -> S, V
__global__ __launch_bounds__(256) void k_maxt_sv(const int32_t* __restrict__ counts, long rows, long N, int32_t* __restrict__ S, int64_t* __restrict__ V) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= rows) return;
    const long s = (long)counts[3 * m + 2] - counts[3 * m], q = (long)counts[3 * m + 2] + counts[3 * m];
    S[m] = (int32_t)s;
    V[m] = N * q - s * s;
}

// ------------------------------------------------------------------------------------------------------------------------------
// the tile.  kbytes = ceil16(n).  op: [P][Rstride][ldop]; the workgroup's permutations are perm0 .. perm0 + 32 RB, live below R.
// S, V, dobs, keyobs, count1 are indexed by the marker's row within this image tile (the caller offsets them to the window); parg gets
// row_base + that row.  pkey / parg: [tiles][R], tile index tile_base + (blockIdx.x / nPB).
// ------------------------------------------------------------------------------------------------------------------------------
template <int P, int RB, bool OBS>
__global__ __launch_bounds__(256) void k_maxt_tile(const int8_t* __restrict__ Mt8, long rows, long ld, long kbytes, const int8_t* __restrict__ op,
                                                   long ldop, long R, long Rstride, long N, long T, const int32_t* __restrict__ S,
                                                   const int64_t* __restrict__ V, int64_t* __restrict__ dobs, double* __restrict__ keyobs,
                                                   int32_t* __restrict__ count1, double* __restrict__ pkey, int32_t* __restrict__ parg, long tile_base,
                                                   long row_base, int nPB) {
    constexpr int NBT = P * RB, RW = 32 * RB;
    constexpr int TB = MX_TM + 32 * NBT;
    constexpr int NCH = TB / 32;   // 16-byte pieces per thread and chunk: TB * 8 / 256
    __shared__ __attribute__((aligned(16))) int8_t tile[TB * MX_BK];
    __shared__ double sk[4][RW];
    __shared__ int sa[4][RW];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const long tl = blockIdx.x / nPB;
    const long row0 = tl * MX_TM, perm0 = (long)(blockIdx.x - tl * nPB) * RW;

    mx_i32x4 pre[NCH];
    auto fetch = [&](long k0) {
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int idx = tid + 256 * i, rr = idx >> 3;
            const long kb = k0 + 16 * (idx & 7);
            mx_i32x4 v = {0, 0, 0, 0};
            if (kb < kbytes) {
                if (rr >= MX_TM) {
                    const int q = rr - MX_TM, p = q / RW;
                    const long pr = perm0 + (q - p * RW);
                    if (pr < R) v = *(const mx_i32x4*)(op + ((long)p * Rstride + pr) * ldop + kb);
                } else if (row0 + rr < rows) v = *(const mx_i32x4*)(Mt8 + (row0 + rr) * ld + kb);
            }
            pre[i] = v;
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int idx = tid + 256 * i, rr = idx >> 3, c = idx & 7;
            *(mx_i32x4*)(tile + rr * MX_BK + ((c ^ ((rr >> 1) & 7)) << 4)) = pre[i];
        }
    };

    mx_i32x16 acc[NBT];
#pragma unroll
    for (int x = 0; x < NBT; x++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[x][e] = 0;

    const int8_t* pa = tile + (32 * w + r) * MX_BK;
    const int8_t* pb = tile + (MX_TM + r) * MX_BK;
    const int swz = (r >> 1) & 7;

    fetch(0);
    for (long k0 = 0; k0 < kbytes; k0 += MX_BK) {
        put();
        __syncthreads();
        if (k0 + MX_BK < kbytes) fetch(k0 + MX_BK);
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
            const int ch = ((2 * ks + h) ^ swz) << 4;
            const mx_i32x4 a = *(const mx_i32x4*)(pa + ch);
#pragma unroll
            for (int x = 0; x < NBT; x++) {
                const mx_i32x4 bb = *(const mx_i32x4*)(pb + x * (32 * MX_BK) + ch);
                acc[x] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bb, acc[x], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // accumulator element e of block x = p RB + b: marker 32 w + (e & 3) + 8 (e >> 2) + 4 h of the tile, plane p, permutation perm0 + 32 b + r
    double bestk[RB];
    int besta[RB];
#pragma unroll
    for (int b = 0; b < RB; b++) { bestk[b] = -1.0; besta[b] = INT_MAX; }
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const long gi = row0 + 32 * w + (e & 3) + 8 * (e >> 2) + 4 * h;
        const bool valid = gi < rows;
        const long Sm = valid ? (long)S[gi] : 0, Vm = valid ? (long)V[gi] : 0;
        long dob = 0;
        if (!OBS && valid) { dob = dobs[gi]; dob = dob < 0 ? -dob : dob; }
        int cnt = 0;
#pragma unroll
        for (int b = 0; b < RB; b++) {
            long c = acc[b][e];
            if (P > 1) c += 128L * acc[(P > 1 ? RB : 0) + b][e];
            if (P > 2) c += 16384L * acc[(P > 2 ? 2 * RB : 0) + b][e];
            const long d = N * c - Sm * T;
            const bool live = valid && perm0 + 32 * b + r < R;
            const double dd = (double)d;
            const double key = Vm ? __ddiv_rn(__dmul_rn(dd, dd), (double)Vm) : 0.0;
            if (OBS) {
                if (live) { dobs[gi] = d; keyobs[gi] = key; }
            } else {
                const unsigned long long mask = __ballot(live && (d < 0 ? -d : d) >= dob);
                cnt += __popc((unsigned)(h ? mask >> 32 : mask & 0xffffffffull));
                if (live && key > bestk[b]) { bestk[b] = key; besta[b] = (int)gi; }   // e ascending = marker ascending: a tie keeps the lower
            }
        }
        if (!OBS && r == 0 && valid && cnt) atomicAdd(count1 + gi, cnt);
    }
    if (OBS) return;
#pragma unroll
    for (int b = 0; b < RB; b++) {
        const double ok = __shfl_xor(bestk[b], 32);
        const int oa = __shfl_xor(besta[b], 32);
        if (ok > bestk[b] || (ok == bestk[b] && oa < besta[b])) { bestk[b] = ok; besta[b] = oa; }
        if (h == 0) { sk[w][32 * b + r] = bestk[b]; sa[w][32 * b + r] = besta[b]; }
    }
    __syncthreads();
    if (tid < RW && perm0 + tid < R) {
        double k = sk[0][tid];
        int a = sa[0][tid];
#pragma unroll
        for (int ww = 1; ww < 4; ww++)                      // the waves' markers ascend with ww
            if (sk[ww][tid] > k) { k = sk[ww][tid]; a = sa[ww][tid]; }
        const long o = (tile_base + tl) * R + perm0 + tid;
        pkey[o] = k;
        parg[o] = (int32_t)(row_base + a);
    }
}

// one thread = one permutation; the tiles lie in marker order
__global__ __launch_bounds__(256) void k_maxt_finish(const double* __restrict__ pkey, const int32_t* __restrict__ parg, long ntiles, long R,
                                                     double* __restrict__ maxkey, int32_t* __restrict__ argmax) {
    const long rr = (long)blockIdx.x * 256 + threadIdx.x;
    if (rr >= R) return;
    double k = -1.0;
    int32_t a = 0;
    for (long tl = 0; tl < ntiles; tl++) {
        const double v = pkey[tl * R + rr];
        if (v > k) { k = v; a = parg[tl * R + rr]; }
    }
    maxkey[rr] = k;
    argmax[rr] = a;
}

// ------------------------------------------------------------------------------------------------------------------------------
// launchers (device pointers throughout)
// ------------------------------------------------------------------------------------------------------------------------------
static long mx_blocks(long threads) { return (threads + 255) / 256; }

// keys: nr x NP2 uint64 (NP2 = the power of two >= N, at least 2); on return every row is sorted ascending
extern "C" int eagle_dev_maxt_permutations(eagle_ctx* ctx, uint64_t seed, long r_first, long nr, long N, long NP2, const uint16_t* strata_u,
                                           uint64_t* keys, void* stream) {
    if (nr <= 0) return EAGLE_OK;
    if (N < 1 || N > MAXT_MAX_N || NP2 < N || NP2 < 2 || NP2 > 65536 || (NP2 & (NP2 - 1)) || r_first < 1 || nr * NP2 > (1L << 36))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "maxt_permutations: bad shape");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_maxt_keys, dim3((unsigned)mx_blocks(nr * NP2)), dim3(256), 0, s, seed, r_first, nr, N, NP2, strata_u, keys);
    const int C = (int)(NP2 < MX_SORT_C ? NP2 : MX_SORT_C);
    const dim3 lgrid((unsigned)(nr * NP2 / C)), ggrid((unsigned)mx_blocks(nr * (NP2 >> 1)));
    hipLaunchKernelGGL(k_maxt_sort_local, lgrid, dim3(256), 0, s, keys, NP2, C, 2L, (long)C);
    for (long k = 2L * C; k <= NP2; k <<= 1) {
        for (long j = k >> 1; j >= C; j >>= 1) hipLaunchKernelGGL(k_maxt_sort_global, ggrid, dim3(256), 0, s, keys, nr, NP2, k, j);
        hipLaunchKernelGGL(k_maxt_sort_local, lgrid, dim3(256), 0, s, keys, NP2, C, k, k);
    }
    MX_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// op: [P][Rtot][ld] int8, ld = a multiple of 16 >= n; rows r0 .. r0 + nr of every plane are written whole.  keys (row stride NP2) or perm
// (row stride N) or neither (the identity) gives the sources; rank[n], tu[N].
extern "C" int eagle_dev_maxt_operand(eagle_ctx* ctx, const uint64_t* keys, long NP2, const int32_t* perm, long N, const int32_t* rank,
                                      const int32_t* tu, long n, long ld, int P, long Rtot, long r0, long nr, int8_t* op, void* stream) {
    if (nr <= 0) return EAGLE_OK;
    if (n <= 0 || n > ld || ld % 16 || ((uintptr_t)op & 15) || P < 1 || P > 3 || r0 < 0 || r0 + nr > Rtot || N < 1 || N > n)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "maxt_operand: bad shape");
    const long lanes16 = ld / 16;
    hipLaunchKernelGGL(k_maxt_operand, dim3((unsigned)mx_blocks(nr * lanes16)), dim3(256), 0, (hipStream_t)stream, keys, NP2, perm, N, rank, tu, n, ld,
                       lanes16, P, Rtot, r0, nr, op);
    MX_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

extern "C" int eagle_dev_maxt_sv(eagle_ctx* ctx, const int32_t* counts, long rows, long N, int32_t* S, int64_t* V, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    hipLaunchKernelGGL(k_maxt_sv, dim3((unsigned)mx_blocks(rows)), dim3(256), 0, (hipStream_t)stream, counts, rows, N, S, V);
    MX_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// The permutation width of a workgroup with P planes: 128 for one plane, 64 for two and three (4, 4 and 6 operand blocks a wave).
extern "C" int eagle_dev_maxt_width(int P) { return P == 1 ? 128 : 64; }

template <int P, int RB>
static void mx_launch(bool obs, dim3 grid, hipStream_t s, const int8_t* Mt8, long rows, long ld, long kbytes, const int8_t* op, long ldop, long R,
                      long Rstride, long N, long T, const int32_t* S, const int64_t* V, int64_t* dobs, double* keyobs, int32_t* count1, double* pkey,
                      int32_t* parg, long tile_base, long row_base, int nPB) {
    if (obs)
        hipLaunchKernelGGL((k_maxt_tile<P, 1, true>), grid, dim3(256), 0, s, Mt8, rows, ld, kbytes, op, ldop, R, Rstride, N, T, S, V, dobs, keyobs,
                           count1, pkey, parg, tile_base, row_base, nPB);
    else
        hipLaunchKernelGGL((k_maxt_tile<P, RB, false>), grid, dim3(256), 0, s, Mt8, rows, ld, kbytes, op, ldop, R, Rstride, N, T, S, V, dobs, keyobs,
                           count1, pkey, parg, tile_base, row_base, nPB);
}

// One pass of the tile over `rows` marker rows of an image.  obs != 0: op holds the trait itself as its one arrangement (R = 1) and
// dobs / keyobs are written; else dobs is read, count1 is added to and the partials of the tiles tile_base .. are written.
extern "C" int eagle_dev_maxt_tile(eagle_ctx* ctx, int obs, const int8_t* Mt8, long rows, long n, long ld, const int8_t* op, long ldop, int P, long R,
                                   long Rstride, long N, long T, const int32_t* S, const int64_t* V, int64_t* dobs, double* keyobs, int32_t* count1,
                                   double* pkey, int32_t* parg, long tile_base, long row_base, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (n <= 0 || n > MAXT_MAX_N || n > ld || ld % 16 || ((uintptr_t)Mt8 & 15) || n > ldop || ldop % 16 || ((uintptr_t)op & 15) || P < 1 || P > 3 ||
        R < 1 || R > Rstride || (obs && R != 1) || N < 1 || N > n)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "maxt_tile: bad shape");
    const int RW = obs ? 32 : eagle_dev_maxt_width(P);
    const long nPB = (R + RW - 1) / RW, blocks = (rows + MX_TM - 1) / MX_TM * nPB;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "maxt_tile: too many tiles");
    const dim3 grid((unsigned)blocks);
    const long kbytes = (n + 15) / 16 * 16;
    hipStream_t s = (hipStream_t)stream;
    if (P == 1) mx_launch<1, 4>(obs != 0, grid, s, Mt8, rows, ld, kbytes, op, ldop, R, Rstride, N, T, S, V, dobs, keyobs, count1, pkey, parg, tile_base, row_base, (int)nPB);
    else if (P == 2) mx_launch<2, 2>(obs != 0, grid, s, Mt8, rows, ld, kbytes, op, ldop, R, Rstride, N, T, S, V, dobs, keyobs, count1, pkey, parg, tile_base, row_base, (int)nPB);
    else mx_launch<3, 2>(obs != 0, grid, s, Mt8, rows, ld, kbytes, op, ldop, R, Rstride, N, T, S, V, dobs, keyobs, count1, pkey, parg, tile_base, row_base, (int)nPB);
    MX_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

extern "C" int eagle_dev_maxt_finish(eagle_ctx* ctx, const double* pkey, const int32_t* parg, long ntiles, long R, double* maxkey, int32_t* argmax,
                                     void* stream) {
    if (R <= 0 || ntiles <= 0) return eagle_fail(ctx, EAGLE_ERR_ARG, "maxt_finish: bad shape");
    hipLaunchKernelGGL(k_maxt_finish, dim3((unsigned)mx_blocks(R)), dim3(256), 0, (hipStream_t)stream, pkey, parg, ntiles, R, maxkey, argmax);
    MX_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}
