// eagle_glmm.hip -- the saddlepoint p-value of a marker's score under the logistic mixed model (include/eagle_hip.h section 1d'''): for
// every marker m the covariate-adjusted genotype G~ = g - X (X'DX)^-1 X'D g, the score T = g'(y - mu), its null variance V* = G~'D G~
// and, where |z| exceeds the cutoff, the two roots of K'(zeta) = +-|q| of the cumulant generating function of sum G~_i (y_i - mu_i)
// with the deviates r* the host turns into tail probabilities.
//
//   k_glmm_spa ... the int8 marker-major image Mt8 (rows x ld, values -1/0/+1) + the staged covariates X16 (n64 x 16 fp64, one 128-byte
//                  row per individual, columns >= c zero) + P4 (n64 x 4 fp64: mu, 1 - mu, D = mu (1 - mu), r = y - mu; from individual n
//                  on 1/2, 1/2, 0, 0) + A16 (16 x 16 fp64: (X'DX)^-1, zero outside c x c) + vara[rows] or NULL
//                  ->  stat[rows][7] = (T, V*, z, zeta_up, r*_up, zeta_lo, r*_lo), info[rows][2] = (code, evaluations).
//
// One wave owns one marker from the first pass to the result, four markers per 256-thread workgroup; the waves of a workgroup share
// nothing and meet at no barrier (their evaluation counts differ), so a marker's result depends on its row and the staged operands alone.
//
// First pass, two sweeps over the individuals in chunks of 64.  Sweep 1, one lane = one individual: D g goes to the wave's LDS, T and
// sum D g^2 to the lane's accumulators; then sixteen v_mfma_f64_16x16x4_f64 per chunk, step s taking the individuals 4 s + k with
// A = x_j (lane = (j = lane & 15, k = lane >> 4)) and B = D g of individual k in every column: every column of the 16 x 16 result is
// s = X'D g (C/D: col = lane & 15, row = (lane >> 4) + 4 reg), the matrix pipe does the reduction over individuals.  beta = A16 s is
// one row per lane.  Sweep 2: G~_i = g_i - x_i' beta, V* = sum D G~^2 and max |G~|.
// One evaluation of (K, K', K'') at zeta is one sweep: a lane recomputes G~ of its individual (c FMAs against beta in LDS; G~ is NOT
// kept: n x 8 bytes per wave does not fit LDS at n = 10,000 and there is no other place that is a wave's own), takes one exp and one
// log1p, and three butterfly sums over the wave finish it.  Every lane holds the same sums, so the root search that follows is the
// same scalar code in every lane and needs no broadcast.
// No atomics, no inline assembly, no block barrier; lane 0 of the wave is the one owner of the marker's nine output words.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

typedef double gs_f64x2 __attribute__((ext_vector_type(2)));
typedef double gs_f64x4 __attribute__((ext_vector_type(4)));

#define GS_P 16               /* padded covariate count */
#define GS_CHUNK 64           /* individuals per chunk = lanes */
#define GS_DEGENERATE 0x1p-40 /* V* must exceed this fraction of sum D g^2, K'(+-zeta_max) pass the target by this fraction of it */
#define GS_ZETA_RANGE 500.0   /* |zeta G~_i| never exceeds it */
#define GS_NEAR_ZERO 1e-4     /* |zeta| sqrt(V*) below which r* is the normal deviate */

struct GsWave {
    double dg[GS_CHUNK];
    double s[GS_P];
    double beta[GS_P];
};

struct GsArgs {
    const int8_t* row;        // the marker's image row
    long n;
    const double* X16;
    const gs_f64x4* P4;
    int c2;                   // pairs of covariate columns read per individual: (c + 1) / 2
};

// LDS traffic between the lanes of ONE wave: its DS operations complete in order, so only the compiler has to be held.
__device__ __forceinline__ void gs_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double gs_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double gs_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// G~ of individual i < n64 whose genotype is gi (0 from individual n on, where the row of X16 is zero as well: G~ = 0).
__device__ __forceinline__ double gs_gtilde(const GsArgs& a, const GsWave& S, long i, double gi) {
    const gs_f64x2* xr = (const gs_f64x2*)(a.X16 + i * GS_P);
    double gt = gi;
    for (int t = 0; t < a.c2; t++) {
        const gs_f64x2 q = xr[t];
        gt = fma(-q[0], S.beta[2 * t], gt);
        gt = fma(-q[1], S.beta[2 * t + 1], gt);
    }
    return gt;
}

__device__ __forceinline__ double gs_geno(const GsArgs& a, long i) { return i < a.n ? (double)(a.row[i] + 1) : 0.0; }

// (K, K', K'') at zeta, the same bits in every lane.  Per individual with a = zeta G~, nu = 1 - mu for a >= 0 and mu else,
// e = exp(-|a|), u = 1 - e, den = 1 - nu u:  K += nu |a| + log1p(-nu u),  K' += sign(a) D G~ u / den,  K'' += D G~^2 e / den^2.
__device__ __forceinline__ void gs_eval(const GsArgs& a, const GsWave& S, int lane, double zeta, double& K0, double& K1, double& K2) {
    double k0 = 0.0, k1 = 0.0, k2 = 0.0;
    for (long i0 = 0; i0 < a.n; i0 += GS_CHUNK) {
        const long i = i0 + lane;                                              // < n64: X16 and P4 are padded to it
        const double gt = gs_gtilde(a, S, i, gs_geno(a, i));
        const gs_f64x4 p = a.P4[i];
        const double av = zeta * gt, ab = fabs(av);
        const double nu = av >= 0.0 ? p[1] : p[0];
        const double e = exp(-ab), u = 1.0 - e, inv = 1.0 / fma(-nu, u, 1.0);
        const double dgt = p[2] * gt;
        k0 += fma(nu, ab, log1p(-nu * u));
        k1 += (av >= 0.0 ? dgt : -dgt) * u * inv;
        k2 += dgt * gt * e * inv * inv;
    }
    K0 = gs_wave_sum(k0);
    K1 = gs_wave_sum(k1);
    K2 = gs_wave_sum(k2);
}

struct GsTail {
    double zeta, rstar;
    int code;                 // 0 solved, 1 max_iter, 5 unreachable (the caller decides between code 3 and + 256)
};

// The root of K' = target (sgn = its sign, +-1) by the rule of section 1d''' 5 and its deviate r*.
__device__ GsTail gs_tail(const GsArgs& a, const GsWave& S, int lane, double target, double sgn, double zmax, double Vs, double tol, int max_iter,
                          int& ev) {
    const double nan = __builtin_nan("");
    GsTail R = {nan, nan, 0};
    double K0, K1, K2;
    double lo = 0.0, hi = sgn * zmax;                                          // K'(lo) - target is on the zero side, K'(hi) - target beyond
    gs_eval(a, S, lane, hi, K0, K1, K2);
    ev++;
    int used = 1;
    if (!(sgn * (K1 - target) > GS_DEGENERATE * fabs(target))) { R.code = 5; return R; }     // at the edge of the support: not reachable
    const double rv = sqrt(Vs);
    double zeta = 0.0, f = -target, k2 = Vs;                                   // K'(0) = 0 and K''(0) = V* need no evaluation
    K0 = 0.0;
    for (;;) {
        double zn = zeta - f / k2;
        if (!(sgn * (zn - lo) >= 0.0 && sgn * (hi - zn) >= 0.0)) zn = 0.5 * (lo + hi);   // a NaN step bisects as well
        const double delta = zn - zeta;
        zeta = zn;
        if (used >= max_iter) { R.code = 1; return R; }
        gs_eval(a, S, lane, zeta, K0, K1, K2);
        ev++;
        used++;
        f = K1 - target;
        k2 = K2;
        if (sgn * f > 0.0) hi = zeta;
        else lo = zeta;
        if (fabs(delta) * rv <= tol) break;
    }
    R.zeta = zeta;
    if (fabs(zeta) * rv < GS_NEAR_ZERO) {
        R.rstar = target / rv;
    } else {
        const double w = sgn * sqrt(2.0 * (zeta * target - K0)), v = zeta * sqrt(k2);
        R.rstar = w + log(v / w) / w;
    }
    return R;
}

__global__ __launch_bounds__(256) void k_glmm_spa(const int8_t* __restrict__ Mt8, long rows, long n, long ld, const double* __restrict__ X16,
                                                  const gs_f64x4* __restrict__ P4, const double* __restrict__ A16, int c,
                                                  const double* __restrict__ vara, double cutoff, double tol, int max_iter,
                                                  double* __restrict__ stat, int32_t* __restrict__ info) {
    __shared__ GsWave sh[4];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long m = (long)blockIdx.x * 4 + wv;
    if (m >= rows) return;                                                     // the whole wave; no block barrier follows
    GsWave& S = sh[wv];
    const GsArgs a = {Mt8 + m * ld, n, X16, P4, (c + 1) / 2};
    const int j = lane & 15, k = lane >> 4;
    const double nan = __builtin_nan("");

    // ---- first pass, sweep 1: T, sum D g^2 and s = X'D g
    double tt = 0.0, s2 = 0.0;
    gs_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (long i0 = 0; i0 < n; i0 += GS_CHUNK) {
        const long i = i0 + lane;
        const double gi = gs_geno(a, i);
        const gs_f64x4 p = P4[i];
        const double dg = p[2] * gi;
        tt = fma(gi, p[3], tt);
        s2 = fma(dg, gi, s2);
        S.dg[lane] = dg;
        gs_sync();
#pragma unroll 4
        for (int s = 0; s < GS_CHUNK / 4; s++) {                               // individuals 4 s + k, covariate j
            const int kk = 4 * s + k;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(X16[(i0 + kk) * GS_P + j], S.dg[kk], acc, 0, 0, 0);
        }
        gs_sync();
    }
    const double T = gs_wave_sum(tt), S2 = gs_wave_sum(s2);
    if (j == 0) {
#pragma unroll
        for (int q = 0; q < 4; q++) S.s[k + 4 * q] = acc[q];
    }
    gs_sync();
    if (lane < GS_P) {
        double b = 0.0;
#pragma unroll
        for (int t = 0; t < GS_P; t++) b = fma(A16[lane * GS_P + t], S.s[t], b);
        S.beta[lane] = b;
    }
    gs_sync();
    // ---- sweep 2: V* and max |G~|
    double vs = 0.0, gm = 0.0;
    for (long i0 = 0; i0 < n; i0 += GS_CHUNK) {
        const long i = i0 + lane;
        const double gt = gs_gtilde(a, S, i, gs_geno(a, i));
        vs = fma(P4[i][2] * gt, gt, vs);
        gm = fmax(gm, fabs(gt));
    }
    const double Vs = gs_wave_sum(vs), gmax = gs_wave_max(gm);

    double z = nan, zu = nan, ru = nan, zl = nan, rl = nan;
    int code = 0, ev = 0;
    const double V = vara ? vara[m] : Vs;
    if (!(Vs > GS_DEGENERATE * S2) || !(V > 0.0 && V < __builtin_inf())) {
        code = 2;
    } else {
        z = T / sqrt(V);
        const double q = z * sqrt(Vs);
        if (fabs(z) <= cutoff) {
            code = 4;
        } else {
            const double aq = fabs(q), zmax = GS_ZETA_RANGE / gmax;
            const bool up_first = T > 0.0;                                     // the observed side first
            GsTail t1 = gs_tail(a, S, lane, up_first ? aq : -aq, up_first ? 1.0 : -1.0, zmax, Vs, tol, max_iter, ev);
            GsTail t2 = {nan, nan, 0};
            if (t1.code == 5) {
                code = 3;
            } else if (t1.code) {
                code = t1.code;
            } else {
                t2 = gs_tail(a, S, lane, up_first ? -aq : aq, up_first ? -1.0 : 1.0, zmax, Vs, tol, max_iter, ev);
                if (t2.code == 5) {                                            // contributes no probability
                    code = 256;
                    t2.zeta = up_first ? -zmax : zmax;
                    t2.rstar = up_first ? -__builtin_inf() : __builtin_inf();
                } else {
                    code = t2.code;
                }
            }
            if ((code & 255) == 0) {
                zu = up_first ? t1.zeta : t2.zeta;
                ru = up_first ? t1.rstar : t2.rstar;
                zl = up_first ? t2.zeta : t1.zeta;
                rl = up_first ? t2.rstar : t1.rstar;
            }
        }
    }
    if (lane == 0) {
        double* o = stat + 7 * m;
        o[0] = T;
        o[1] = Vs;
        o[2] = z;
        o[3] = zu;
        o[4] = ru;
        o[5] = zl;
        o[6] = rl;
        info[2 * m] = code;
        info[2 * m + 1] = ev;
    }
}

// X16: n64 x 16 fp64, P4: n64 x 4 fp64, n64 = n rounded up to 64, both as the head of this file describes them; A16: 16 x 16 fp64;
// vara: rows fp64 or NULL.
extern "C" int eagle_dev_glmm_spa(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, const double* X16, const double* P4,
                                  const double* A16, int c, const double* vara, double cutoff, double tol, int max_iter, double* stat, int32_t* info,
                                  void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (n <= 0 || n > ld || n > 0x3fffffffL || ((uintptr_t)X16 & 15) || ((uintptr_t)P4 & 31))
        return eagle_fail(ctx, EAGLE_ERR_ARG, "glmm_spa: bad image shape");
    if (c < 1 || c > GS_P - 1 || !(cutoff >= 0.0) || !(tol > 0.0 && tol < 1.0) || max_iter < 1 || max_iter > 1000)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "glmm_spa: bad search parameters");
    const long blocks = (rows + 3) / 4;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "glmm_spa: too many rows");
    hipLaunchKernelGGL(k_glmm_spa, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, Mt8, rows, n, ld, X16, (const gs_f64x4*)P4, A16, c,
                       vara, cutoff, tol, max_iter, stat, info);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return eagle_fail_hip(ctx, e, __func__);
    return EAGLE_OK;
}
