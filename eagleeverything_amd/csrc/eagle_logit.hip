// eagle_logit.hip -- logistic regression of a binary trait on covariates and one marker at a time (include/eagle_hip.h section
// 1b''''iv): for every marker m the fit of  logit P(y_i = 1) = x_i' beta + g_im gamma  over the used individuals, by Newton steps from
// the covariates-only fit, with the score test of gamma = 0 from the first evaluation and Firth's penalised fit on demand.
//
//   k_logit_irls<FIRTH_MODE> ... the int8 marker-major image Mt8 (rows x ld, values -1/0/+1) + the staged covariates X16 (n64 x 16 fp64,
//                                 one 128-byte row per individual, columns >= c zero, rows of unused individuals zero) + valid_y (n64
//                                 bytes: 0 = not used, 2 = control, 3 = case) + beta0[c]  ->  stat[rows][4] = (gamma, se, score, loglik),
//                                 info[rows][2] = (code, evaluations).  FIRTH_MODE 0 = maximum likelihood, 1 = Firth, 2 = fallback.
//
// One wave owns one marker from the first evaluation to the result, four markers per 256-thread workgroup; the waves of a workgroup
// share nothing and meet at no barrier (their iteration counts differ), so a marker's result depends on its row, X16, valid_y and
// beta0 alone.  Parameter j < c is covariate j; parameter c = p - 1, the LAST one, is gamma, whose column g = image value + 1 is read
// from the image row and exists nowhere else.  p is padded to 16 with zero columns.
//
// One evaluation at beta walks the individuals in chunks of 64.
//   Part A, one lane = one individual of the chunk: eta = x' beta (16 FMAs, beta broadcast from LDS), e = exp(-|eta|), mu, w = mu (1 -
//   mu), the residual y - mu and the log-likelihood term, each once per individual; w, the residual and g go to the wave's LDS.
//   Part B, lane = (j = lane & 15, k = lane >> 4): sixteen v_mfma_f64_16x16x4_f64 per chunk, step s taking the individuals 4 s + k with
//   A = w x_j and B = x_j, accumulate I = sum w x x' in four fp64 accumulators per lane (C/D: col = lane & 15, row = (lane >> 4) + 4 reg):
//   the matrix pipe does the reduction over individuals.  U rides beside it as one FMA per lane and step (residual x_j), and its four
//   partial sums per j are added in the order k = 0, 1, 2, 3 at the end: a fixed order.
// The Cholesky factor of I (lower triangle, in LDS, one column per step, lanes over rows and over the trailing block), the two
// triangular solves (a lane per unknown, the pivot's value by a lane shuffle) and, for Firth, I^-1 (sixteen solves, four at a time in
// the four 16-lane groups) are the wave's own fp64 work.  Firth's second pass repeats part A with h = w x' I^-1 x (the lower triangle
// of I^-1 broadcast from LDS against the lane's row in registers) and accumulates U* as U is accumulated; it has no MFMA.
// No atomics, no inline assembly, no block barrier; lane 0 of the wave is the one owner of the marker's six output words.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eagle_hip.h"
#include "eagle_ctx.h"
#include "eagle_internal.h"

typedef double lg_f64x2 __attribute__((ext_vector_type(2)));
typedef double lg_f64x4 __attribute__((ext_vector_type(4)));

#define LG_P 16            /* padded parameter count */
#define LG_CHUNK 64        /* individuals per chunk = lanes */
#define LG_ETA_MAX 40.0    /* |eta| beyond which ML reports separation */
#define LG_STEP_MAX 5.0    /* cap of max |delta_j| */
#define LG_PIVOT_REL 0x1p-40 /* a Cholesky pivot must exceed this fraction of its diagonal entry of I */

struct LgWave {
    double Im[LG_P * LG_P];    // I, then its Cholesky factor in the lower triangle
    double Inv[LG_P * LG_P];   // I^-1 (Firth), zero outside p x p
    double w[LG_CHUNK], r[LG_CHUNK], g[LG_CHUNK], u[LG_CHUNK];
    double beta[LG_P];
};

struct LgArgs {
    const int8_t* row;         // the marker's image row
    long n;
    const double* X16;
    const uint8_t* vy;
    const double* beta0;
    int c, p;
    double tol;
    int max_iter;
};

struct LgResult {
    double gamma, se, score, ll;
    int code, ev;
};

// LDS traffic between the lanes of ONE wave: its DS operations complete in order, so only the compiler has to be held.
__device__ __forceinline__ void lg_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double lg_nanmax(double a, double b) { return (a > b || a != a) ? a : b; }   // NaN wins

__device__ __forceinline__ double lg_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int W>
__device__ __forceinline__ double lg_max(double v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v = lg_nanmax(v, __shfl_xor(v, o));
    return v;
}

// One pass over the individuals at S.beta.  STAR = false: I -> acc (the MFMA accumulators), U -> the return value (U_j in every lane
// with lane & 15 = j), the log-likelihood and max |eta| over the used individuals.  STAR = true (Firth's second pass, S.Inv = I^-1):
// U* only.
template <bool STAR>
__device__ __forceinline__ double lg_pass(const LgArgs& a, LgWave& S, int lane, lg_f64x4& acc, double& ll_out, double& mx_out) {
    const int j = lane & 15, k = lane >> 4, c = a.c;
    double uacc = 0.0, ll = 0.0, mx = 0.0;
    acc = lg_f64x4{0.0, 0.0, 0.0, 0.0};
    double bj[LG_P];
#pragma unroll
    for (int t = 0; t < LG_P; t++) bj[t] = S.beta[t];
    const double bg = S.beta[c];
    for (long i0 = 0; i0 < a.n; i0 += LG_CHUNK) {
        {   // part A: this lane's individual
            const long i = i0 + lane;                                          // < n64: X16 and vy are padded to it
            const double gi = i < a.n ? (double)(a.row[i] + 1) : 0.0;
            const int v = a.vy[i];
            const lg_f64x2* xr = (const lg_f64x2*)(a.X16 + i * LG_P);
            double x[LG_P];
#pragma unroll
            for (int t = 0; t < LG_P / 2; t++) {
                const lg_f64x2 q = xr[t];
                x[2 * t] = q[0];
                x[2 * t + 1] = q[1];
            }
            double eta = gi * bg;                                              // column c of X16 is zero: bj[c] meets zeros
#pragma unroll
            for (int t = 0; t < LG_P; t++) eta = fma(x[t], bj[t], eta);
            const double e = exp(-fabs(eta)), d = 1.0 / (1.0 + e);
            const double mu = eta >= 0.0 ? d : e * d;
            const bool used = (v & 2) != 0;
            const double y = (double)(v & 1);
            double w = used ? e * d * d : 0.0;
            double r = used ? ((v & 1) ? (eta >= 0.0 ? e * d : d) : -mu) : 0.0;   // y - mu without cancellation
            if (!STAR) {
                if (used) {
                    ll += y * eta - (fmax(eta, 0.0) + log1p(e));
                    mx = lg_nanmax(fabs(eta), mx);
                }
            } else {
                // h = w x~' I^-1 x~ from the lower triangle of I^-1; x~ = x with g in place c (x[c] = 0)
                double q = 0.0, qc = 0.0;
#pragma unroll
                for (int jj = 0; jj < LG_P; jj++) {
                    double t = 0.5 * S.Inv[jj * LG_P + jj] * x[jj];
#pragma unroll
                    for (int kk = 0; kk < jj; kk++) t = fma(S.Inv[jj * LG_P + kk], x[kk], t);
                    q = fma(x[jj], t, q);
                    qc = fma(S.Inv[c * LG_P + jj], x[jj], qc);                 // row c: columns < c, the rest meets zeros of x
                }
                const double h = w * (2.0 * q + gi * (2.0 * qc + gi * S.Inv[c * LG_P + c]));
                r = used ? r + h * (0.5 - mu) : 0.0;
            }
            S.w[lane] = w;
            S.r[lane] = r;
            S.g[lane] = gi;
        }
        lg_sync();
#pragma unroll 4
        for (int s = 0; s < LG_CHUNK / 4; s++) {   // part B: individuals 4 s + k, parameter j
            const int kk = 4 * s + k;
            double xv = a.X16[(i0 + kk) * LG_P + j];
            if (j == c) xv = S.g[kk];
            if (!STAR) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(S.w[kk] * xv, xv, acc, 0, 0, 0);
            uacc = fma(S.r[kk], xv, uacc);
        }
        lg_sync();
    }
    S.u[lane] = uacc;
    lg_sync();
    const double U = ((S.u[j] + S.u[16 + j]) + S.u[32 + j]) + S.u[48 + j];
    lg_sync();
    if (!STAR) {
        ll_out = lg_wave_sum(ll);
        mx_out = lg_max<64>(mx);
    }
    return U;
}

// In-place Cholesky of the p x p lower triangle of A; d0 = this lane's original diagonal entry A[j][j], j = lane & 15.  False when a
// pivot is not above LG_PIVOT_REL of its diagonal entry or not finite (the same verdict in every lane: all read the same words).
__device__ __forceinline__ bool lg_chol(double* A, int p, int lane, double d0) {
    for (int j = 0; j < p; j++) {
        const double d = A[j * LG_P + j], dj = __shfl(d0, j);
        if (!(d > dj * LG_PIVOT_REL) || !(d < __builtin_inf())) return false;
        const double l = sqrt(d);
        lg_sync();
        if (lane == j) A[j * LG_P + j] = l;
        else if (lane > j && lane < p) A[lane * LG_P + j] = A[lane * LG_P + j] / l;
        lg_sync();
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int e = lane + 64 * t, i = e >> 4, kk = e & 15;
            if (kk > j && i >= kk && i < p) A[i * LG_P + kk] -= A[i * LG_P + j] * A[kk * LG_P + j];
        }
        lg_sync();
    }
    return true;
}

// L L' x = b inside every 16-lane group: lane i = lane & 15 holds b_i and returns x_i (lanes i >= p return what they brought).
__device__ __forceinline__ double lg_solve(const double* Lm, int p, int lane, double b) {
    const int i = lane & 15, base = lane & 48;
    for (int j = 0; j < p; j++) {
        const double y = __shfl(b, base | j) / Lm[j * LG_P + j];
        if (i == j) b = y;
        else if (i > j && i < p) b -= Lm[i * LG_P + j] * y;
    }
    for (int j = p - 1; j >= 0; j--) {
        const double x = __shfl(b, base | j) / Lm[j * LG_P + j];
        if (i == j) b = x;
        else if (i < j) b -= Lm[j * LG_P + i] * x;
    }
    return b;
}

template <bool FIRTH>
__device__ void lg_fit(const LgArgs& a, LgWave& S, int lane, LgResult& R, bool keep_score) {
    const int j = lane & 15, k = lane >> 4, c = a.c, p = a.p;
    const double nan = __builtin_nan("");
    if (lane < LG_P) S.beta[lane] = lane < c ? a.beta0[lane] : 0.0;
    lg_sync();
    R.gamma = R.se = R.ll = nan;
    if (!keep_score) R.score = nan;
    R.code = 1;
    R.ev = 0;
    while (R.ev < a.max_iter) {
        lg_f64x4 acc;
        double ll, mx;
        double U = lg_pass<false>(a, S, lane, acc, ll, mx);
        R.ev++;
#pragma unroll
        for (int q = 0; q < 4; q++) S.Im[(k + 4 * q) * LG_P + j] = acc[q];
        lg_sync();
        const double d0 = S.Im[j * LG_P + j];
        lg_sync();
        if (!lg_chol(S.Im, p, lane, d0)) { R.code = 2; break; }
        const double lgg = S.Im[c * LG_P + c];
        if (R.ev == 1 && !keep_score) {
            const double ug = __shfl(U, c);
            R.score = (ug * ug) / (lgg * lgg);
        }
        if (!FIRTH && mx > LG_ETA_MAX) { R.code = 3; break; }
        if (FIRTH) {
#pragma unroll 1
            for (int t = 0; t < 4; t++) {                                      // I^-1, columns 4 t + k
                const int e = 4 * t + k;
                const double b = lg_solve(S.Im, p, lane, j == e ? 1.0 : 0.0);
                S.Inv[j * LG_P + e] = (j < p && e < p) ? b : 0.0;
            }
            lg_sync();
            double ll2, mx2;
            U = lg_pass<true>(a, S, lane, acc, ll2, mx2);
        }
        double delta = lg_solve(S.Im, p, lane, U);
        if (j >= p) delta = 0.0;
        const double md = lg_max<16>(fabs(delta));
        if (md > LG_STEP_MAX) delta *= LG_STEP_MAX / md;
        if (lane < LG_P) S.beta[lane] += delta;
        lg_sync();
        if (md <= a.tol) {
            R.code = 0;
            R.gamma = S.beta[c];
            R.se = 1.0 / lgg;
            R.ll = ll;
            break;
        }
    }
    lg_sync();
}

template <int FIRTH_MODE>
__global__ __launch_bounds__(256) void k_logit_irls(const int8_t* __restrict__ Mt8, long rows, long n, long ld, const double* __restrict__ X16,
                                                    const uint8_t* __restrict__ vy, const double* __restrict__ beta0, int p, double tol,
                                                    int max_iter, double* __restrict__ stat, int32_t* __restrict__ info) {
    __shared__ LgWave sh[4];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long m = (long)blockIdx.x * 4 + wv;
    if (m >= rows) return;                                                     // the whole wave; no block barrier follows
    LgWave& S = sh[wv];
    const LgArgs a = {Mt8 + m * ld, n, X16, vy, beta0, p - 1, p, tol, max_iter};
    LgResult R;
    if (FIRTH_MODE == 1) {
        lg_fit<true>(a, S, lane, R, false);
        R.code += 256;
    } else {
        lg_fit<false>(a, S, lane, R, false);
        if (FIRTH_MODE == 2 && R.code != 0 && !(R.code == 2 && R.ev == 1)) {   // restart from (beta0, 0); the score is the first one's
            lg_fit<true>(a, S, lane, R, true);
            R.code += 256;
        }
    }
    if (lane == 0) {
        stat[4 * m] = R.gamma;
        stat[4 * m + 1] = R.se;
        stat[4 * m + 2] = R.score;
        stat[4 * m + 3] = R.ll;
        info[2 * m] = R.code;
        info[2 * m + 1] = R.ev;
    }
}

// X16: n64 x 16 fp64 and valid_y: n64 bytes, n64 = n rounded up to 64, both zero from individual n on; the rows of X16 of individuals
// with valid_y = 0 are zero as well (the caller's staging: eagle_logistic).  beta0: c = p - 1 fp64.
extern "C" int eagle_dev_logistic(eagle_ctx* ctx, const int8_t* Mt8, long rows, long n, long ld, const double* X16, const uint8_t* valid_y,
                                  const double* beta0, int p, int firth, double tol, int max_iter, double* stat, int32_t* info, void* stream) {
    if (rows <= 0) return EAGLE_OK;
    if (n <= 0 || n > ld || n > 0x3fffffffL || ((uintptr_t)X16 & 15)) return eagle_fail(ctx, EAGLE_ERR_ARG, "logistic: bad image shape");
    if (p < 2 || p > LG_P || firth < 0 || firth > 2 || !(tol > 0.0 && tol < 1.0) || max_iter < 1 || max_iter > 1000)
        return eagle_fail(ctx, EAGLE_ERR_ARG, "logistic: bad fit parameters");
    const long blocks = (rows + 3) / 4;
    if (blocks > 0x7fffffffL) return eagle_fail(ctx, EAGLE_ERR_ARG, "logistic: too many rows");
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t s = (hipStream_t)stream;
    if (firth == 0) hipLaunchKernelGGL(k_logit_irls<0>, grid, blk, 0, s, Mt8, rows, n, ld, X16, valid_y, beta0, p, tol, max_iter, stat, info);
    else if (firth == 1) hipLaunchKernelGGL(k_logit_irls<1>, grid, blk, 0, s, Mt8, rows, n, ld, X16, valid_y, beta0, p, tol, max_iter, stat, info);
    else hipLaunchKernelGGL(k_logit_irls<2>, grid, blk, 0, s, Mt8, rows, n, ld, X16, valid_y, beta0, p, tol, max_iter, stat, info);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return eagle_fail_hip(ctx, e, __func__);
    return EAGLE_OK;
}
