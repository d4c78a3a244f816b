// eagle_admix.hip -- one EM step of the admixture model (include/eagle_hip.h section 1b''''v): for K ancestral populations the ancestry
// fractions Q (n x K) of the individuals and the allele frequencies F (L x K) of the populations, from the int8 marker-major image Mt8
// (rows x ld, values -1/0/+1, dosage d = value + 1).
//
//   k_admix_f<UPDATE> ... a wave owns 16 markers and walks the individuals 16 at a time: F' of its markers (UPDATE) and its share of the
//                         log-likelihood, one partial per 16-marker tile.
//   k_admix_q ........... the transposed tile: a wave owns 16 individuals and one marker range and walks the range's markers 16 at a time:
//                         T' (k x individual) into the partials buffer part[S][n16][16].
//   k_admix_ll_finish ... the tiles' likelihood partials added in one fixed order.
//   k_admix_q_finish .... the ranges of part added in order, q t / (2 L), the floor and the row normalisation.
//
// Both tile kernels keep Q and F as 16-column padded fp64 images (Q16: n16 x 16, F16: L16 x 16; columns >= K and rows beyond n / L zero)
// and form p = sum_k q f and pbar = sum_k q (1 - f) on v_mfma_f64_16x16x4_f64 with ceil(K / 4) instructions each (A: lane holds
// [row = lane & 15][k = lane >> 4]; B: [k = lane >> 4][col = lane & 15]; C/D: col = lane & 15, row = (lane >> 4) + 4 reg).  A lane
// turns its four entries into A = d / p and B = (2 - d) / pbar; C register r is then, as it lies, the B operand of the reduction
// indices 4 r .. 4 r + 3, so the second product (sum over individuals in k_admix_f, over markers in k_admix_q) is four more
// instructions per term with no lane movement and no LDS.  Individuals >= n and markers >= L are masked to A = B = 0 in the lane:
// neither kernel relies on what the image holds there.  Rows beyond the window are not read (the row index is clamped).
//
// Two kernels, not one fused through an LDS transpose: the F tile wants the accumulator to live across the walk over individuals, the Q
// tile across the walk over markers, and a fused tile would have to spill one of the two to memory per 16 x 16 block.  Recomputing p
// costs ceil(K / 4) * 2 instructions against the 16 divisions and logarithms a tile needs anyway.
// No atomics, no inline assembly, no block barrier: the waves of a workgroup share nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_host.h"
#include "eagle_internal.h"

typedef double ax_f64x4 __attribute__((ext_vector_type(4)));

#define AX_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ double ax_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The lane's four (A, B) of a 16 x 16 tile from its p and pbar; live[r] = the entry exists, d[r] its dosage.
__device__ __forceinline__ void ax_ratios(const ax_f64x4& P, const ax_f64x4& Pb, const bool live[4], const int d[4], ax_f64x4& A, ax_f64x4& B) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const double p = live[r] ? P[r] : 1.0, pb = live[r] ? Pb[r] : 1.0;
        A[r] = live[r] ? (double)d[r] / p : 0.0;
        B[r] = live[r] ? (double)(2 - d[r]) / pb : 0.0;
    }
}

// Mt8: the rows [row0, row0 + rows) of the image, row0 a multiple of 16.  Fin / Fout: F16 of the whole panel.  llpart[tile]: the
// likelihood of the markers 16 tile .. 16 tile + 15 (global tile index).
template <bool UPDATE>
__global__ __launch_bounds__(256) void k_admix_f(const int8_t* __restrict__ Mt8, long row0, long rows, long n, long ld, int K,
                                                 const double* __restrict__ Q16, const double* __restrict__ Fin, double* __restrict__ Fout,
                                                 double* __restrict__ llpart) {
    const int lane = threadIdx.x & 63, j = lane & 15, k = lane >> 4;
    const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long m0 = tile * 16;                                                  // window-relative
    if (m0 >= rows) return;                                                     // the whole wave; no block barrier follows
    const int ks = (K + 3) >> 2;
    const bool mlive = m0 + j < rows;
    const long mrow = mlive ? m0 + j : rows - 1;
    const int8_t* grow = Mt8 + mrow * ld;
    // B operands of the first products, fixed for the walk: F'[kk = 4 s + k][marker j] and its complement, zero from K on
    double fB[4], fbB[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int kk = 4 * s + k;
        const double f = Fin[(row0 + m0 + j) * 16 + kk];                        // F16 is padded to L16 rows: in bounds, zero beyond L
        fB[s] = f;
        fbB[s] = (kk < K && mlive) ? 1.0 - f : 0.0;
    }
    ax_f64x4 sa = {0.0, 0.0, 0.0, 0.0}, sb = {0.0, 0.0, 0.0, 0.0};
    double ll = 0.0;
    for (long i0 = 0; i0 < n; i0 += 16) {
        ax_f64x4 P = {0.0, 0.0, 0.0, 0.0}, Pb = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; s++) {
            if (s >= ks) break;                                                 // uniform
            const double q = Q16[(i0 + j) * 16 + 4 * s + k];
            P = AX_MFMA(q, fB[s], P);
            Pb = AX_MFMA(q, fbB[s], Pb);
        }
        const int4 gw = *(const int4*)(grow + i0);                              // 16 bytes of the lane's own row; ld and i0 are multiples of 16
        const int w[4] = {gw.x, gw.y, gw.z, gw.w};
        bool live[4];
        int d[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {                                           // individual i0 + k + 4 r: byte k of word r
            live[r] = mlive && i0 + k + 4 * r < n;
            d[r] = (int)(int8_t)(w[r] >> (8 * k)) + 1;
        }
        ax_f64x4 A, B;
        ax_ratios(P, Pb, live, d, A, B);
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (live[r]) ll += (d[r] ? (double)d[r] * log(P[r]) : 0.0) + (d[r] != 2 ? (double)(2 - d[r]) * log(Pb[r]) : 0.0);
        if (UPDATE) {
#pragma unroll
            for (int r = 0; r < 4; r++) {                                       // A operand: Q[individual i0 + 4 r + k][population j]
                const double qa = Q16[(i0 + 4 * r + k) * 16 + j];
                sa = AX_MFMA(qa, A[r], sa);
                sb = AX_MFMA(qa, B[r], sb);
            }
        }
    }
    ll = ax_wave_sum(ll);
    if (lane == 0) llpart[row0 / 16 + tile] = ll;
    if (UPDATE && mlive) {
#pragma unroll
        for (int r = 0; r < 4; r++) {                                           // sa[r] = (population k + 4 r, marker j)
            const int kk = k + 4 * r;
            const long at = (row0 + m0 + j) * 16 + kk;
            const double f = Fin[at];
            const double a = f * sa[r], b = (1.0 - f) * sb[r], t = a + b;
            double fn = t > 0.0 ? a / t : f;
            fn = fn < EAGLE_ADMIX_EPS ? EAGLE_ADMIX_EPS : (fn > 1.0 - EAGLE_ADMIX_EPS ? 1.0 - EAGLE_ADMIX_EPS : fn);
            Fout[at] = kk < K ? fn : 0.0;
        }
    }
}

// grid = (tiles of 16 individuals, S ranges).  A wave walks the markers of its range that the window [row0, row0 + rows) holds; where
// the window starts inside the range it takes the accumulator up from part, and it always leaves it there.
__global__ __launch_bounds__(64) void k_admix_q(const int8_t* __restrict__ Mt8, long row0, long rows, long n, long L, long ld, int K,
                                                long range_len, const double* __restrict__ Q16, const double* __restrict__ F16,
                                                double* __restrict__ part) {
    const int lane = threadIdx.x, j = lane & 15, k = lane >> 4;
    const long i0 = (long)blockIdx.x * 16, n16 = (long)gridDim.x * 16, s = blockIdx.y;
    const long rlo = s * range_len, rhi = rlo + range_len < L ? rlo + range_len : L;
    const long lo = rlo > row0 ? rlo : row0, hi = rhi < row0 + rows ? rhi : row0 + rows;
    if (lo >= hi) return;
    const int ks = (K + 3) >> 2;
    const bool ilive = i0 + j < n;
    double qB[4];                                                               // B operands of the first products: Q'[kk = 4 s + k][individual j]
#pragma unroll
    for (int t = 0; t < 4; t++) qB[t] = Q16[(i0 + j) * 16 + 4 * t + k];
    double* mine = part + ((size_t)s * (size_t)n16 + (size_t)i0) * 16;         // [individual][population]
    ax_f64x4 acc;
#pragma unroll
    for (int r = 0; r < 4; r++) acc[r] = lo > rlo ? mine[j * 16 + k + 4 * r] : 0.0;
    for (long m0 = lo; m0 < hi; m0 += 16) {                                     // m0 is a multiple of 16 on every route
        ax_f64x4 P = {0.0, 0.0, 0.0, 0.0}, Pb = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t >= ks) break;                                                 // uniform
            const int kk = 4 * t + k;
            const bool fl = m0 + j < L;
            const double f = F16[(m0 + j) * 16 + kk];
            P = AX_MFMA(f, qB[t], P);
            Pb = AX_MFMA((kk < K && fl) ? 1.0 - f : 0.0, qB[t], Pb);
        }
        bool live[4];
        int d[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {                                           // marker m0 + k + 4 r, individual i0 + j: consecutive bytes across j
            const long m = m0 + k + 4 * r;
            live[r] = ilive && m < hi;
            const long mr = m < hi ? m : hi - 1;
            d[r] = (int)Mt8[(mr - row0) * ld + i0 + j] + 1;
        }
        ax_f64x4 A, B;
        ax_ratios(P, Pb, live, d, A, B);
#pragma unroll
        for (int r = 0; r < 4; r++) {                                           // A operand: F[marker m0 + 4 r + k][population j] and its complement
            const long m = m0 + 4 * r + k;
            const double f = F16[m * 16 + j];
            acc = AX_MFMA(f, A[r], acc);
            acc = AX_MFMA((j < K && m < L) ? 1.0 - f : 0.0, B[r], acc);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) mine[j * 16 + k + 4 * r] = acc[r];            // acc[r] = (population k + 4 r, individual j)
}

// One workgroup: thread t adds the partials t, t + 256, ... in that order, then the 256 sums are added pairwise in a fixed tree.
__global__ __launch_bounds__(256) void k_admix_ll_finish(const double* __restrict__ llpart, long tiles, double* __restrict__ out) {
    __shared__ double sh[256];
    double v = 0.0;
    for (long t = threadIdx.x; t < tiles; t += 256) v += llpart[t];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

// One thread per individual: t_k = sum over the ranges in order, q'_k = max(q_k t_k / (2 L), eps), then the row divided by its sum
// (k = 0, 1, ... in order).
__global__ __launch_bounds__(256) void k_admix_q_finish(const double* __restrict__ part, int S, long n, long n16, long L, int K,
                                                        const double* __restrict__ Qin, double* __restrict__ Qout) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double q[EAGLE_ADMIX_KMAX], sum = 0.0;
    const double twoL = 2.0 * (double)L;
#pragma unroll
    for (int kk = 0; kk < EAGLE_ADMIX_KMAX; kk++) {
        double t = 0.0;
        for (int s = 0; s < S; s++) t += part[((size_t)s * (size_t)n16 + (size_t)i) * 16 + kk];
        double v = Qin[i * 16 + kk] * t / twoL;
        v = v > EAGLE_ADMIX_EPS ? v : EAGLE_ADMIX_EPS;
        q[kk] = kk < K ? v : 0.0;
        sum += q[kk];
    }
#pragma unroll
    for (int kk = 0; kk < EAGLE_ADMIX_KMAX; kk++) Qout[i * 16 + kk] = q[kk] / sum;
}

// One row window [row0, row0 + rows) of one pass.  update = 0: the likelihood partials only.
extern "C" int eagle_dev_admix_window(eagle_ctx* ctx, const int8_t* Mt8, long row0, long rows, long n, long L, long ld, int K, int update,
                                      const double* Q16, const double* Fin, double* Fout, double* llpart, double* part, int S, long range_len,
                                      void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (n <= 0 || n > 0x3fffffffL || (n + 15) / 16 * 16 > ld || (ld & 15) || ((uintptr_t)Mt8 & 15) || (row0 & 15) || row0 < 0 || row0 + rows > L ||
        ((rows & 15) && row0 + rows != L))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "admixture: bad image shape");
    if (K < 1 || K > EAGLE_ADMIX_KMAX || S < 1 || range_len < 16 || (range_len & 15)) return eagle_fail(ctx, EAGLE_ERR_ARG, "admixture: bad plan");
    const long blocks = ((rows + 15) / 16 + 3) / 4, itiles = (n + 15) / 16;
    if (blocks > 0x7fffffffL || S > 65535) return eagle_fail(ctx, EAGLE_ERR_ARG, "admixture: too many rows");
    hipStream_t s = (hipStream_t)stream;
    if (update) {
        hipLaunchKernelGGL(k_admix_f<true>, dim3((unsigned)blocks), dim3(256), 0, s, Mt8, row0, rows, n, ld, K, Q16, Fin, Fout, llpart);
        hipLaunchKernelGGL(k_admix_q, dim3((unsigned)itiles, (unsigned)S), dim3(64), 0, s, Mt8, row0, rows, n, L, ld, K, range_len, Q16, Fin, part);
    } else {
        hipLaunchKernelGGL(k_admix_f<false>, dim3((unsigned)blocks), dim3(256), 0, s, Mt8, row0, rows, n, ld, K, Q16, Fin, Fout, llpart);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return eagle_fail_hip(ctx, e, __func__);
    return EAGLE_OK;
}

// The end of a pass: ll_out = the sum of the tiles' partials; with update, Qout from part and Qin.
extern "C" int eagle_dev_admix_finish(eagle_ctx* ctx, long n, long L, int K, int update, const double* llpart, double* ll_out, const double* part,
                                      int S, const double* Qin, double* Qout, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const long n16 = (n + 15) / 16 * 16;
    hipLaunchKernelGGL(k_admix_ll_finish, dim3(1), dim3(256), 0, s, llpart, (L + 15) / 16, ll_out);
    if (update)
        hipLaunchKernelGGL(k_admix_q_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, S, n, n16, L, K, Qin, Qout);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return eagle_fail_hip(ctx, e, __func__);
    return EAGLE_OK;
}
