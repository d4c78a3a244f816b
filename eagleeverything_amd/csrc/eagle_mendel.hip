// eagle_mendel.hip -- Mendel errors of a trio list and exhaustive parentage assignment (include/eagle_hip.h section 1b'''viii) on the bit
// planes of eagle_ibd.hip.  Integer arithmetic only; plain HIP, no inline assembly.
//
//   Planes.  A = hom A1, B = hom A2 and, from the .bed file only, C = called: one uint64 per individual per 64 panel markers, word w of
//   individual i at plane[w * np + i] (eagle_ibd.hip).  On the image route every marker is called, so C is the mask of the word's panel
//   markers (mendel_word_mask): bits past the last marker must not become hets of the child.
//
//   k_mendel_trios<MARK> . one lane per trio, 64 list entries per wave, the three individuals gathered by index.  The lanes walk the words,
//                          form the error word of rule 3 (mendel_error_word, eagle_host.h) and add six popcounts.  MARK: the wave turns its
//                          64 error words into 64 per-bit totals by one ballot and one popcount per bit -- lane b keeps the total of bit b
//                          -- and adds them to the marker array with one 32-bit atomic per lane; a word without an error in any lane is
//                          skipped.  Nothing goes through LDS.
//   k_plane_gather ....... the words of an index list into a compact word-major sub-plane (index -1: zero words), so that 64 consecutive
//                          candidates are 512 consecutive bytes.
//   k_parentage .......... a wave takes one offspring, 64 consecutive dams (one a lane) and PAR_SB sires; the four waves of a workgroup
//                          take 4 PAR_SB consecutive sires.  Per word the child's and the sires' words are wave-uniform loads and
//                          x, u, v of rule 3 wave-uniform values; a lane loads its dam's A and B word once for all PAR_SB sires and adds
//                          popcount(x | u & B_d | v & A_d) to each.  The .bed route adds the overlap word C_c & C_s & C_d.  Every lane
//                          keeps its two smallest keys (e << 32 | ordinal) with their overlap counts; the wave reduces them by shuffles,
//                          the workgroup through LDS, and each workgroup writes its two to the partial array.
//   k_parentage_finish ... one wave per offspring merges the partials and writes rule 6's two rows.  No atomics: keys are unique inside
//                          an offspring, so the minimum does not depend on the order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

#define MENDEL_LAUNCH_CHECK(ctx)                                            \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) return eagle_fail_hip(ctx, e__, __func__);   \
    } while (0)

#define PAR_SB 4                  // sires per lane: a dam word is loaded once for all of them
#define PAR_WAVES 4               // waves of a workgroup; it takes PAR_SB * PAR_WAVES sires
#define PAR_NONE 0xffffffffffffffffull

// trios: T x 3 int32 (child, father, mother; a parent may be -1).  out: T x 6 int32.  marker: L int32, zeroed by the caller (MARK).
template <bool MARK>
__global__ __launch_bounds__(64) void k_mendel_trios(const uint64_t* __restrict__ A, const uint64_t* __restrict__ B, const uint64_t* __restrict__ Cc,
                                                     long np, long L, long nwords, const int32_t* __restrict__ trios, long T,
                                                     int32_t* __restrict__ out, int32_t* __restrict__ marker) {
    const int lane = threadIdx.x;
    const long t = 64 * (long)blockIdx.x + lane;
    const bool live = t < T;
    const long c = live ? trios[3 * t] : 0, f = live ? trios[3 * t + 1] : -1, m = live ? trios[3 * t + 2] : -1;
    const long fi = f < 0 ? 0 : f, mi = m < 0 ? 0 : m;   // an unknown parent reads individual 0 and drops the words
    int n_cf = 0, e_cf = 0, n_cm = 0, e_cm = 0, n_trio = 0, e = 0;
    for (long w = 0; w < nwords; w++) {
        const long o = w * np;
        const uint64_t valid = mendel_word_mask(w, L);
        const uint64_t ac = A[o + c], bc = B[o + c], cc = Cc ? Cc[o + c] : valid;
        uint64_t af = A[o + fi], bf = B[o + fi], cf = Cc ? Cc[o + fi] : valid;
        uint64_t am = A[o + mi], bm = B[o + mi], cm = Cc ? Cc[o + mi] : valid;
        if (f < 0) af = bf = cf = 0;
        if (m < 0) am = bm = cm = 0;
        uint64_t E = mendel_error_word(ac, bc, cc, af, bf, am, bm);
        if (!live) E = 0;
        n_cf += __popcll(cc & cf);
        e_cf += __popcll((ac & bf) | (bc & af));
        n_cm += __popcll(cc & cm);
        e_cm += __popcll((ac & bm) | (bc & am));
        n_trio += __popcll(cc & cf & cm);
        e += __popcll(E);
        if (MARK) {
            if (__ballot(E != 0) == 0) continue;         // wave-uniform
            int mine = 0;
#pragma unroll 8
            for (int b = 0; b < 64; b++) {
                const int cnt = __popcll(__ballot((E >> b) & 1ull));
                if (lane == b) mine = cnt;
            }
            const long x = 64 * w + lane;
            if (mine > 0 && x < L) atomicAdd(marker + x, mine);
        }
    }
    if (live) {
        int32_t* row = out + 6 * t;
        row[0] = n_cf; row[1] = e_cf; row[2] = n_cm; row[3] = e_cm; row[4] = n_trio; row[5] = e;
    }
}

// src: nplanes planes of nwords x np words; dst: nplanes planes of nwords x cp words, cp = cnt rounded up to 64.  grid (cp / 64, nwords).
__global__ __launch_bounds__(64) void k_plane_gather(const uint64_t* __restrict__ src, long np, long nwords, int nplanes, const int32_t* __restrict__ idx,
                                                     long cnt, long cp, uint64_t* __restrict__ dst) {
    const long k = 64 * (long)blockIdx.x + threadIdx.x, w = blockIdx.y;
    if (k >= cp) return;
    const long i = k < cnt ? (long)idx[k] : -1;
    for (int p = 0; p < nplanes; p++)
        dst[(size_t)p * (size_t)nwords * (size_t)cp + (size_t)(w * cp + k)] = i >= 0 ? src[(size_t)p * (size_t)nwords * (size_t)np + (size_t)(w * np + i)] : 0ull;
}

struct ParBest { uint64_t k1, k2; int32_t n1, n2; };   // the two smallest keys, k1 <= k2, with their overlap counts

__device__ __forceinline__ void par_push(ParBest& s, uint64_t k, int32_t n) {
    if (k < s.k1) { s.k2 = s.k1; s.n2 = s.n1; s.k1 = k; s.n1 = n; }
    else if (k < s.k2) { s.k2 = k; s.n2 = n; }
}

__device__ __forceinline__ void par_merge(ParBest& s, const ParBest& o) {
    par_push(s, o.k1, o.n1);
    par_push(s, o.k2, o.n2);                            // o.k2 >= o.k1: nothing of o is lost
}

__device__ __forceinline__ void par_wave_reduce(ParBest& s) {
    for (int d = 32; d >= 1; d >>= 1) {
        ParBest o;
        o.k1 = __shfl_xor((unsigned long long)s.k1, d, 64);
        o.k2 = __shfl_xor((unsigned long long)s.k2, d, 64);
        o.n1 = __shfl_xor(s.n1, d, 64);
        o.n2 = __shfl_xor(s.n2, d, 64);
        par_merge(s, o);
    }
}

// The gathered sub-planes: O of the offspring [o0 + blockIdx.y] (leading dimension op), S of the sires (sp), D of the dams (dp); each A
// then B then, with BED, C.  sidx / didx: the lists' individuals, used to leave out s == c, d == c and s == d; ns / nd = 0: one unknown
// parent (zero words; its C word counts as called everywhere for the overlap).  blockIdx.x = sire group * dtiles + dam tile.
// part_k / part_n: per offspring of the chunk, 2 * gridDim.x entries.
template <bool BED>
__global__ __launch_bounds__(64 * PAR_WAVES) void k_parentage(const uint64_t* __restrict__ O, long op, const uint64_t* __restrict__ S, long sp,
                                                              const uint64_t* __restrict__ D, long dp, long L, long nwords,
                                                              const int32_t* __restrict__ oidx, const int32_t* __restrict__ sidx,
                                                              const int32_t* __restrict__ didx, long o0, long ns, long nd, long dtiles,
                                                              int min_overlap, int allow_self, uint64_t* __restrict__ part_k,
                                                              int32_t* __restrict__ part_n) {
    __shared__ uint64_t sh_k[2 * PAR_WAVES];
    __shared__ int32_t sh_n[2 * PAR_WAVES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long sg = (long)blockIdx.x / dtiles, dt = (long)blockIdx.x - sg * dtiles;
    const long oc = o0 + blockIdx.y;
    const long nse = ns > 0 ? ns : 1, nde = nd > 0 ? nd : 1;
    const long s0 = (sg * PAR_WAVES + wave) * PAR_SB;   // the wave's first sire: wave-uniform; s0 + PAR_SB <= sp by the padding of sp
    const long d = 64 * dt + lane;                       // the lane's dam: d < dp
    const size_t oplane = (size_t)nwords * (size_t)op, splane = (size_t)nwords * (size_t)sp, dplane = (size_t)nwords * (size_t)dp;
    int e[PAR_SB], ov[PAR_SB];
#pragma unroll
    for (int k = 0; k < PAR_SB; k++) e[k] = ov[k] = 0;
    if (s0 < nse) {                                      // wave-uniform: a wave past the last sire has no candidate
        for (long w = 0; w < nwords; w++) {
            const uint64_t ac = O[w * op + oc], bc = O[oplane + w * op + oc];
            const uint64_t cc = BED ? O[2 * oplane + w * op + oc] : mendel_word_mask(w, L);
            const uint64_t ad = D[w * dp + d], bd = D[dplane + w * dp + d];
            uint64_t cd = 0;
            if (BED) cd = nd > 0 ? D[2 * dplane + w * dp + d] : ~0ull;
#pragma unroll
            for (int k = 0; k < PAR_SB; k++) {
                const uint64_t as = S[w * sp + s0 + k], bs = S[splane + w * sp + s0 + k];
                const MendelXUV t = mendel_xuv(ac, bc, cc, as, bs);
                e[k] += __popcll(t.x | (t.u & bd) | (t.v & ad));
                if (BED) {
                    const uint64_t cs = ns > 0 ? S[2 * splane + w * sp + s0 + k] : ~0ull;
                    ov[k] += __popcll(cc & cs & cd);
                }
            }
        }
    }
    ParBest best = {PAR_NONE, PAR_NONE, -1, -1};
    const int32_t c = oidx[oc];
    const int32_t dam = (nd > 0 && d < nd) ? didx[d] : -1;
#pragma unroll
    for (int k = 0; k < PAR_SB; k++) {
        const long s = s0 + k;
        if (s >= nse || d >= nde) continue;
        const int32_t sire = ns > 0 ? sidx[s] : -1;
        const int n = BED ? ov[k] : (int)L;
        if (sire == c || dam == c || n < min_overlap) continue;
        if (!allow_self && sire == dam && sire >= 0) continue;
        par_push(best, ((uint64_t)(uint32_t)e[k] << 32) | (uint64_t)parentage_ordinal(s, d, nd), n);
    }
    par_wave_reduce(best);
    if (lane == 0) {
        sh_k[2 * wave] = best.k1; sh_k[2 * wave + 1] = best.k2;
        sh_n[2 * wave] = best.n1; sh_n[2 * wave + 1] = best.n2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ParBest all = {sh_k[0], sh_k[1], sh_n[0], sh_n[1]};
        for (int v = 1; v < PAR_WAVES; v++) {
            const ParBest o = {sh_k[2 * v], sh_k[2 * v + 1], sh_n[2 * v], sh_n[2 * v + 1]};
            par_merge(all, o);
        }
        const size_t at = 2 * ((size_t)blockIdx.y * (size_t)gridDim.x + (size_t)blockIdx.x);
        part_k[at] = all.k1; part_k[at + 1] = all.k2;
        part_n[at] = all.n1; part_n[at + 1] = all.n2;
    }
}

// One wave per offspring of the chunk: nparts pairs of partials -> best[(o0 + blockIdx.x) * 8 ...] = (sire, dam, e, n_trio) twice.
__global__ __launch_bounds__(64) void k_parentage_finish(const uint64_t* __restrict__ part_k, const int32_t* __restrict__ part_n, long nparts,
                                                         const int32_t* __restrict__ sidx, const int32_t* __restrict__ didx, long ns, long nd,
                                                         long o0, int32_t* __restrict__ best_out) {
    const int lane = threadIdx.x;
    const size_t base = 2 * (size_t)blockIdx.x * (size_t)nparts;
    ParBest best = {PAR_NONE, PAR_NONE, -1, -1};
    for (long p = lane; p < 2 * nparts; p += 64) par_push(best, part_k[base + p], part_n[base + p]);
    par_wave_reduce(best);
    if (lane < 2) {
        const uint64_t key = lane == 0 ? best.k1 : best.k2;
        const int32_t n = lane == 0 ? best.n1 : best.n2;
        int32_t* row = best_out + 8 * (o0 + (long)blockIdx.x) + 4 * lane;
        if (key == PAR_NONE) {
            row[0] = row[1] = row[2] = row[3] = -1;
        } else {
            const long ord = (long)(key & 0xffffffffull), nde = nd > 0 ? nd : 1;
            row[0] = ns > 0 ? sidx[ord / nde] : -1;
            row[1] = nd > 0 ? didx[ord % nde] : -1;
            row[2] = (int32_t)(key >> 32);
            row[3] = n;
        }
    }
}

// planes: A, B (nplanes 2, the image) or A, B, C (3, the .bed file) of n individuals x L markers.  trios: T x 3 (device); out: T x 6;
// marker: L int32, ZEROED by the caller, or NULL.
extern "C" int eagle_dev_mendel_trios(eagle_ctx* ctx, const uint64_t* planes, int nplanes, long n, long L, const int32_t* trios, long T, int32_t* out,
                                      int32_t* marker, void* stream) {
    if (n < 1 || L <= 0 || L > 0x7fffffffL || T < 1 || T > MENDEL_MAX_TRIOS || (nplanes != 2 && nplanes != 3))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "mendel_trios: bad shape");
    const long np = (n + 63) / 64 * 64, nwords = (L + 63) / 64;
    const size_t plane = (size_t)nwords * (size_t)np;
    const uint64_t* Cc = nplanes == 3 ? planes + 2 * plane : nullptr;
    const dim3 g((unsigned)((T + 63) / 64)), b(64);
    if (marker) hipLaunchKernelGGL((k_mendel_trios<true>), g, b, 0, (hipStream_t)stream, planes, planes + plane, Cc, np, L, nwords, trios, T, out, marker);
    else hipLaunchKernelGGL((k_mendel_trios<false>), g, b, 0, (hipStream_t)stream, planes, planes + plane, Cc, np, L, nwords, trios, T, out, marker);
    MENDEL_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}

// dst: nplanes x nwords x cp words, cp = eagle_parentage_pad(cnt).  idx: cnt indices in [-1, n) (device).
extern "C" int eagle_dev_plane_gather(eagle_ctx* ctx, const uint64_t* planes, int nplanes, long n, long L, const int32_t* idx, long cnt, uint64_t* dst,
                                      void* stream) {
    const long nwords = (L + 63) / 64;
    if (n < 1 || L <= 0 || L > 0x7fffffffL || cnt < 1 || cnt > 0x7fffffffL || nwords > 65535L * 65535L || (nplanes != 2 && nplanes != 3))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "plane_gather: bad shape");
    const long np = (n + 63) / 64 * 64, cp = (cnt + 63) / 64 * 64;
    for (long w0 = 0; w0 < nwords; w0 += 65535) {        // gridDim.y holds 65535 words
        const long nw = nwords - w0 < 65535 ? nwords - w0 : 65535;
        // the launch sees the planes from word w0 on: the plane stride stays that of the whole planes
        hipLaunchKernelGGL(k_plane_gather, dim3((unsigned)(cp / 64), (unsigned)nw), dim3(64), 0, (hipStream_t)stream, planes + w0 * np, np, nwords, nplanes,
                           idx, cnt, cp, dst + w0 * cp);
        MENDEL_LAUNCH_CHECK(ctx);
    }
    return EAGLE_OK;
}

// The number of partial pairs per offspring that eagle_dev_parentage writes for ns sires and nd dams (0 = one unknown parent).
extern "C" long eagle_parentage_parts(long ns, long nd) {
    const long nse = ns > 0 ? ns : 1, nde = nd > 0 ? nd : 1;
    return ((nse + PAR_SB * PAR_WAVES - 1) / (PAR_SB * PAR_WAVES)) * ((nde + 63) / 64);
}

// The offspring [o0, o0 + no) of the gathered offspring planes (no <= 65535): the partials of the chunk, then their merge into best
// (n_o x 8 int32, device).  O / S / D: the gathered sub-planes of the three lists (k_plane_gather), idx arrays on the device.
extern "C" int eagle_dev_parentage(eagle_ctx* ctx, const uint64_t* O, long n_o, const uint64_t* S, long ns, const uint64_t* D, long nd, int nplanes, long L,
                                   const int32_t* oidx, const int32_t* sidx, const int32_t* didx, long o0, long no, int min_overlap, int allow_self,
                                   uint64_t* part_k, int32_t* part_n, int32_t* best, void* stream) {
    const long nse = ns > 0 ? ns : 1, nde = nd > 0 ? nd : 1;
    if (L <= 0 || L > 0x7fffffffL || n_o < 1 || o0 < 0 || no < 1 || no > 65535 || o0 + no > n_o || ns < 0 || nd < 0 || (ns == 0 && nd == 0) ||
        nse * nde > 0x7fffffffL || (nplanes != 2 && nplanes != 3))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "parentage: bad shape");
    const long nwords = (L + 63) / 64, op = (n_o + 63) / 64 * 64, sp = (nse + 63) / 64 * 64, dp = (nde + 63) / 64 * 64;
    const long dtiles = dp / 64, nparts = eagle_parentage_parts(ns, nd);
    const dim3 g((unsigned)nparts, (unsigned)no), b(64 * PAR_WAVES);
    hipStream_t s = (hipStream_t)stream;
    if (nplanes == 3)
        hipLaunchKernelGGL((k_parentage<true>), g, b, 0, s, O, op, S, sp, D, dp, L, nwords, oidx, sidx, didx, o0, ns, nd, dtiles, min_overlap, allow_self,
                           part_k, part_n);
    else
        hipLaunchKernelGGL((k_parentage<false>), g, b, 0, s, O, op, S, sp, D, dp, L, nwords, oidx, sidx, didx, o0, ns, nd, dtiles, min_overlap, allow_self,
                           part_k, part_n);
    MENDEL_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_parentage_finish, dim3((unsigned)no), dim3(64), 0, s, part_k, part_n, nparts, sidx, didx, ns, nd, o0, best);
    MENDEL_LAUNCH_CHECK(ctx);
    return EAGLE_OK;
}
